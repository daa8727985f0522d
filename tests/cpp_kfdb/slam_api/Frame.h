// Test infrastructure: model of ORB_SLAM2::Frame holding only what the KeyFrameDatabase adapter reads (include/Frame.h:
// mnId, mBowVec).
#ifndef ORBGPU_TEST_KFDB_FRAME_H
#define ORBGPU_TEST_KFDB_FRAME_H
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"

namespace ORB_SLAM2 {

class Frame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};

}  // namespace ORB_SLAM2

#endif
