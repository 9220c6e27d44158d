/*
 * KeyFrameDatabase_amd.cc -- MI355X definitions of ORB_SLAM2::KeyFrameDatabase (KeyFrameDatabase.cc:33-309).
 *
 * add / erase / clear keep the keyframes' BowVectors in the device database (orbdb_add / orbdb_erase /
 * orbdb_clear) instead of the inverted file. DetectLoopCandidates / DetectRelocalizationCandidates make one
 * orbdb_query: per keyframe the number of words shared with the query (what the inverted-file walk counts into
 * mnLoopWords / mnRelocWords, :86-104, :207-222), ORBVocabulary::score of the pair (:133, :249) and the smallest
 * common word, which with the insertion order gives lKFsSharingWords' order. The selection is
 * orbdb_select_candidates (:107-196, :224-308). The KeyFrame members the reference writes are written here too:
 * mnLoopQuery, mnLoopWords, mLoopScore / mnRelocQuery, mnRelocWords, mRelocScore; a connected keyframe that
 * shares a word keeps its mnLoopQuery and ends with mnLoopWords = 1, as the reference's reset-then-count leaves
 * it. (A second query with the mnId of the previous one is treated as a new query.)
 *
 * Without a usable device nothing is stored and both Detect* return no candidates; the status is logged
 * (orbamd_status.h), never thrown.
 */
#include "KeyFrameDatabase.h"

#include <cstdlib>
#include <cstring>

#include "orbamd_status.h"

namespace ORB_SLAM2 {

namespace {

int env_int(const char* name, int def) {
    const char* s = getenv(name);
    return s && *s ? atoi(s) : def;
}

void flatten(const DBoW2::BowVector& bv, std::vector<uint32_t>& w, std::vector<double>& v) {
    w.clear();
    v.clear();
    w.reserve(bv.size());
    v.reserve(bv.size());
    for (DBoW2::BowVector::const_iterator it = bv.begin(); it != bv.end(); ++it) {  // ascending word id
        w.push_back(it->first);
        v.push_back(it->second);
    }
}

/* one query's entries in insertion order */
struct QueryResult {
    std::vector<KeyFrame*> kf;
    std::vector<int32_t> ncommon;
    std::vector<float> score;
    std::vector<uint32_t> first;
};

}  // namespace

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary& voc) : mpVoc(&voc), mpDb(nullptr) {
    amd::StatusOk(orbdb_create(env_int("ORBAMD_DEVICE", 0), env_int("ORBAMD_KFDB_CAPACITY", 8192),
                               env_int("ORBAMD_KFDB_WORDS", 2048), ORBDB_SCORING_L1, &mpDb),
                  "orbdb_create");
}

KeyFrameDatabase::~KeyFrameDatabase() { orbdb_destroy(mpDb); }

void KeyFrameDatabase::add(KeyFrame* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpDb) return;
    std::vector<uint32_t> w;
    std::vector<double> v;
    flatten(pKF->mBowVec, w, v);
    const uint64_t key = amd::KeyFrameKey(pKF, pKF->mnId);
    if (amd::StatusOk(orbdb_add(mpDb, key, w.data(), v.data(), (int)w.size(), nullptr), "orbdb_add")) mKeyToKF[key] = pKF;
}

void KeyFrameDatabase::erase(KeyFrame* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpDb) return;
    const uint64_t key = amd::KeyFrameKey(pKF, pKF->mnId);
    amd::StatusOk(orbdb_erase(mpDb, key, nullptr), "orbdb_erase");
    mKeyToKF.erase(key);
}

void KeyFrameDatabase::clear() {
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpDb) return;
    amd::StatusOk(orbdb_clear(mpDb, nullptr), "orbdb_clear");
    mKeyToKF.clear();
}

namespace {

/* orbdb_query of `bv` under the database's mutex (held by the caller) */
bool run_query(orbdb_handle* db, const std::unordered_map<uint64_t, KeyFrame*>& by_key, const DBoW2::BowVector& bv,
               QueryResult& r) {
    if (!db) return amd::StatusOk(ORBX_EDEVICE, "orbdb_query (no database)");
    std::vector<uint32_t> w;
    std::vector<double> v;
    flatten(bv, w, v);
    int n = 0;
    if (!amd::StatusOk(orbdb_entries(db, 0, nullptr, nullptr, &n), "orbdb_entries")) return false;
    std::vector<uint64_t> keys(n);
    r.ncommon.resize(n);
    r.score.resize(n);
    r.first.resize(n);
    if (!amd::StatusOk(orbdb_query(db, w.data(), v.data(), (int)w.size(), n, keys.data(), r.ncommon.data(),
                                   r.score.data(), r.first.data(), &n, nullptr),
                       "orbdb_query"))
        return false;
    r.kf.resize(n);
    for (int i = 0; i < n; i++) {
        std::unordered_map<uint64_t, KeyFrame*>::const_iterator it = by_key.find(keys[i]);
        r.kf[i] = it == by_key.end() ? nullptr : it->second;
        if (!r.kf[i]) r.ncommon[i] = 0;  // cannot happen: every stored key has its keyframe
    }
    return true;
}

/* the selection over a query's result. `connected` marks the entries of GetConnectedKeyFrames (loop mode, else
 * empty); GetBestCovisibilityKeyFrames(10) is asked only of the entries the reference can put in lScoreAndMatch */
template <class ScoreOf>
std::vector<KeyFrame*> select(int mode, const QueryResult& r, const std::vector<uint8_t>& connected, float minScore,
                              ScoreOf score_of) {
    const int n = (int)r.kf.size();
    std::vector<KeyFrame*> out;
    if (n == 0) return out;
    int maxCommonWords = 0;
    for (int i = 0; i < n; i++)
        if (!(mode == ORBDB_MODE_LOOP && connected[i]) && r.ncommon[i] > maxCommonWords) maxCommonWords = r.ncommon[i];
    if (maxCommonWords == 0) return out;
    const int minCommonWords = maxCommonWords * 0.8f;
    std::unordered_map<KeyFrame*, int> index;
    for (int i = 0; i < n; i++) index[r.kf[i]] = i;
    std::vector<int32_t> off(n + 1, 0), neigh;
    std::vector<float> last(n);
    for (int i = 0; i < n; i++) {
        last[i] = r.kf[i] ? score_of(r.kf[i]) : 0.f;
        if (r.kf[i] && r.ncommon[i] > minCommonWords && !(mode == ORBDB_MODE_LOOP && connected[i])) {
            const std::vector<KeyFrame*> vpNeighs = r.kf[i]->GetBestCovisibilityKeyFrames(10);
            for (size_t k = 0; k < vpNeighs.size(); k++) {
                std::unordered_map<KeyFrame*, int>::const_iterator it = index.find(vpNeighs[k]);
                neigh.push_back(it == index.end() ? -1 : it->second);
            }
        }
        off[i + 1] = (int32_t)neigh.size();
    }
    const std::vector<float> before = last;
    std::vector<int32_t> idx(n);
    int nout = 0;
    if (!amd::StatusOk(orbdb_select_candidates(mode, n, r.ncommon.data(), r.score.data(), r.first.data(),
                                               mode == ORBDB_MODE_LOOP ? connected.data() : nullptr, off.data(),
                                               neigh.data(), minScore, last.data(), idx.data(), &nout),
                       "orbdb_select_candidates"))
        return out;
    for (int i = 0; i < n; i++)
        if (r.kf[i] && memcmp(&last[i], &before[i], sizeof(float)) != 0) score_of(r.kf[i]) = last[i];
    out.reserve(nout);
    for (int i = 0; i < nout; i++) out.push_back(r.kf[idx[i]]);
    return out;
}

float& loop_score(KeyFrame* kf) { return kf->mLoopScore; }
float& reloc_score(KeyFrame* kf) { return kf->mRelocScore; }

}  // namespace

std::vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates(KeyFrame* pKF, float minScore) {
    std::set<KeyFrame*> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
    QueryResult r;
    std::vector<uint8_t> connected;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (!run_query(mpDb, mKeyToKF, pKF->mBowVec, r)) return std::vector<KeyFrame*>();
        const int n = (int)r.kf.size();
        connected.assign(n > 0 ? n : 1, 0);
        for (int i = 0; i < n; i++) {
            KeyFrame* pKFi = r.kf[i];
            if (r.ncommon[i] <= 0) continue;
            connected[i] = spConnectedKeyFrames.count(pKFi) ? 1 : 0;
            if (connected[i]) {
                pKFi->mnLoopWords = 1;  // reset at every shared word, then counted (:95, :102)
            } else {
                pKFi->mnLoopQuery = pKF->mnId;
                pKFi->mnLoopWords = r.ncommon[i];
            }
        }
    }
    return select(ORBDB_MODE_LOOP, r, connected, minScore, loop_score);
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F) {
    QueryResult r;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (!run_query(mpDb, mKeyToKF, F->mBowVec, r)) return std::vector<KeyFrame*>();
        for (size_t i = 0; i < r.kf.size(); i++) {
            if (r.ncommon[i] <= 0) continue;
            r.kf[i]->mnRelocQuery = F->mnId;
            r.kf[i]->mnRelocWords = r.ncommon[i];
        }
    }
    return select(ORBDB_MODE_RELOC, r, std::vector<uint8_t>(), 0.f, reloc_score);
}

}  // namespace ORB_SLAM2
