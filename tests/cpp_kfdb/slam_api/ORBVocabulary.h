// Test infrastructure: the vocabulary type the KeyFrameDatabase declaration names.  The adapter only keeps its address;
// the test uses the host mirror's class, whose score() it also drives.
#ifndef ORBGPU_TEST_KFDB_ORBVOCABULARY_H
#define ORBGPU_TEST_KFDB_ORBVOCABULARY_H
#include "../../../orb-slam-birdview_amd/host/ORBVocabulary.h"
#endif
