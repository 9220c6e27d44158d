/* TEST-ONLY stand-in for ORB_SLAM2/include/ORBVocabulary.h: KeyFrameDatabase only keeps the pointer. */
#ifndef ORBVOCABULARY_H
#define ORBVOCABULARY_H
namespace ORB_SLAM2 {
class ORBVocabulary {};
}  // namespace ORB_SLAM2
#endif
