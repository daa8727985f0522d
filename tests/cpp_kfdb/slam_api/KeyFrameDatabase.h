// Test infrastructure: the declaration of ORB_SLAM2::KeyFrameDatabase with the reference's member signatures and
// members (include/KeyFrameDatabase.h:42-70), over the models in this directory.
#ifndef ORBGPU_TEST_KFDB_KEYFRAMEDATABASE_H
#define ORBGPU_TEST_KFDB_KEYFRAMEDATABASE_H
#include <list>
#include <mutex>
#include <set>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "ORBVocabulary.h"

namespace ORB_SLAM2 {

class KeyFrame;
class Frame;

class KeyFrameDatabase {
public:
    KeyFrameDatabase(const ORBVocabulary& voc);

    void add(KeyFrame* pKF);
    void erase(KeyFrame* pKF);
    void clear();

    std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore);
    std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F);

protected:
    const ORBVocabulary* mpVoc;
    std::vector<std::list<KeyFrame*> > mvInvertedFile;
    std::mutex mMutex;
};

}  // namespace ORB_SLAM2

#endif
