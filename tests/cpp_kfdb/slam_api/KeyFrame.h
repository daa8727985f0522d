// Test infrastructure: model of ORB_SLAM2::KeyFrame holding only what the KeyFrameDatabase adapter reads
// (include/KeyFrame.h: mnId, mBowVec, GetConnectedKeyFrames, GetBestCovisibilityKeyFrames).  The covisibility graph is
// whatever the test wires into the two public vectors.
#ifndef ORBGPU_TEST_KFDB_KEYFRAME_H
#define ORBGPU_TEST_KFDB_KEYFRAME_H
#include <set>
#include <vector>

#include "Thirdparty/DBoW2/DBoW2/BowVector.h"

namespace ORB_SLAM2 {

class KeyFrame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;

    std::vector<KeyFrame*> connected;         // test wiring
    std::vector<KeyFrame*> best_covisibles;   // test wiring, best first

    std::set<KeyFrame*> GetConnectedKeyFrames() { return std::set<KeyFrame*>(connected.begin(), connected.end()); }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
        if ((int)best_covisibles.size() < N) return best_covisibles;
        return std::vector<KeyFrame*>(best_covisibles.begin(), best_covisibles.begin() + N);
    }
};

}  // namespace ORB_SLAM2

#endif
