/* TEST-ONLY mock of the KeyFrame members KeyFrameDatabase reads and writes (names and types as in
 * ORB_SLAM2/include/KeyFrame.h). */
#ifndef KEYFRAME_H
#define KEYFRAME_H
#include <map>
#include <set>
#include <vector>
#include "ORBVocabulary.h"
namespace DBoW2 {
typedef std::map<unsigned int, double> BowVector;
}
namespace ORB_SLAM2 {
class KeyFrame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
    // Variables used by the keyframe database
    long unsigned int mnLoopQuery = 0;
    int mnLoopWords = 0;
    float mLoopScore = 0;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;
    // the covisibility graph, set by the test
    std::set<KeyFrame*> mConnected;
    std::vector<KeyFrame*> mOrdered;  // best covisibility first
    std::set<KeyFrame*> GetConnectedKeyFrames() { return mConnected; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
        if ((int)mOrdered.size() < N) return mOrdered;
        return std::vector<KeyFrame*>(mOrdered.begin(), mOrdered.begin() + N);
    }
};
}  // namespace ORB_SLAM2
#endif
