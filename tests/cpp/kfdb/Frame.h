/* TEST-ONLY mock of the Frame members KeyFrameDatabase::DetectRelocalizationCandidates reads. */
#ifndef FRAME_H
#define FRAME_H
#include "KeyFrame.h"
namespace ORB_SLAM2 {
class Frame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};
}  // namespace ORB_SLAM2
#endif
