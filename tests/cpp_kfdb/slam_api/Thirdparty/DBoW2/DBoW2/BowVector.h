// Test infrastructure: model of DBoW2::BowVector (Thirdparty/DBoW2/DBoW2/BowVector.h): the std::map<WordId, WordValue>
// it is.
#ifndef ORBGPU_TEST_KFDB_BOWVECTOR_H
#define ORBGPU_TEST_KFDB_BOWVECTOR_H
#include <map>

namespace DBoW2 {

typedef unsigned int WordId;
typedef double WordValue;

class BowVector : public std::map<WordId, WordValue> {};

}  // namespace DBoW2

#endif
