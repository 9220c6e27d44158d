/*
 * KeyFrameDatabase.h -- drop-in replacement of ORB_SLAM2/include/KeyFrameDatabase.h with the reference's class
 * surface (KeyFrameDatabase.h:42-70). The inverted file becomes a device-resident database of the keyframes'
 * BowVectors (orbdb_* of orbslam_amd.h): one query scores the query BowVector against every keyframe, and the
 * candidate selection of DetectLoopCandidates / DetectRelocalizationCandidates runs over its result
 * (KeyFrameDatabase_amd.cc).
 *
 * Sizes: ORBAMD_KFDB_CAPACITY keyframes (default 8192) of at most ORBAMD_KFDB_WORDS BowVector entries (default
 * 2048, at most 4096), on device ORBAMD_DEVICE (default 0); the storage (capacity x words x 12 B) is allocated
 * by the first add.
 */
#ifndef KEYFRAMEDATABASE_H
#define KEYFRAMEDATABASE_H

#include <list>
#include <mutex>
#include <set>
#include <unordered_map>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "ORBVocabulary.h"
#include "orbslam_amd.h"

namespace ORB_SLAM2 {

class KeyFrame;
class Frame;

class KeyFrameDatabase {
public:
    KeyFrameDatabase(const ORBVocabulary& voc);
    ~KeyFrameDatabase();
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    void add(KeyFrame* pKF);

    void erase(KeyFrame* pKF);

    void clear();

    // Loop Detection
    std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore);

    // Relocalization
    std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F);

protected:
    // Associated vocabulary
    const ORBVocabulary* mpVoc;

    // The device database (instead of the inverted file) and its keys' keyframes
    orbdb_handle* mpDb;
    std::unordered_map<uint64_t, KeyFrame*> mKeyToKF;

    // Mutex
    std::mutex mMutex;
};

}  // namespace ORB_SLAM2

#endif
