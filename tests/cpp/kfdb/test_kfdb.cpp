/* test_kfdb.cpp -- the KeyFrameDatabase drop-in (host/KeyFrameDatabase.h, KeyFrameDatabase_amd.cc) called like
 * LoopClosing::DetectLoop and Tracking::Relocalization call the reference's, against a restatement of
 * KeyFrameDatabase.cc:40-309 with an inverted file of lists and a sequential double L1 score. Two identical sets
 * of mock keyframes, one per side; after every call the candidate vectors (as keyframe indices, in order) and
 * every field the database writes must agree (scores as bits).
 *   test_kfdb            needs the device
 *   test_kfdb nodevice   run with ORBAMD_DEVICE=99: no candidates, a status line on stderr, no exception
 * Prints "ALL PASS" on success. Build: tests/cpp/kfdb/build_kfdb.sh */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <list>
#include <map>
#include <set>
#include <vector>

#include "KeyFrameDatabase.h"
#include "orbamd_status.h"

using namespace ORB_SLAM2;

static int failures = 0;
#define CHECK(cond, ...)                               \
    do {                                               \
        if (!(cond)) {                                 \
            printf("FAIL %s:%d ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                       \
            printf("\n");                              \
            failures++;                                \
        }                                              \
    } while (0)

/* ---- the restatement ---- */
static float ref_score(const DBoW2::BowVector& v1, const DBoW2::BowVector& v2) {
    DBoW2::BowVector::const_iterator a = v1.begin(), b = v2.begin();
    double s = 0;
    while (a != v1.end() && b != v2.end()) {
        if (a->first == b->first) {
            const double vi = a->second, wi = b->second;
            s += (fabs(vi - wi) - fabs(vi)) - fabs(wi);
            ++a;
            ++b;
        } else if (a->first < b->first) {
            ++a;
        } else {
            ++b;
        }
    }
    return (float)(-s / 2.0);
}

struct RefDatabase {
    std::map<unsigned int, std::list<KeyFrame*> > inv;
    void add(KeyFrame* kf) {
        for (auto& e : kf->mBowVec) inv[e.first].push_back(kf);
    }
    void erase(KeyFrame* kf) {
        for (auto& e : kf->mBowVec) {
            std::list<KeyFrame*>& l = inv[e.first];
            for (auto it = l.begin(); it != l.end(); ++it)
                if (*it == kf) {
                    l.erase(it);
                    break;
                }
        }
    }
    static std::vector<KeyFrame*> retain(const std::vector<std::pair<float, KeyFrame*> >& acc, float best) {
        const float keep = 0.75f * best;
        std::vector<KeyFrame*> out;
        std::set<KeyFrame*> seen;
        for (auto& e : acc)
            if (e.first > keep && !seen.count(e.second)) {
                out.push_back(e.second);
                seen.insert(e.second);
            }
        return out;
    }
    std::vector<KeyFrame*> loop(KeyFrame* q, float minScore) {
        std::set<KeyFrame*> conn = q->GetConnectedKeyFrames();
        std::vector<KeyFrame*> sharing;
        for (auto& w : q->mBowVec)
            for (KeyFrame* k : inv[w.first]) {
                if (k->mnLoopQuery != q->mnId) {
                    k->mnLoopWords = 0;
                    if (!conn.count(k)) {
                        k->mnLoopQuery = q->mnId;
                        sharing.push_back(k);
                    }
                }
                k->mnLoopWords++;
            }
        if (sharing.empty()) return {};
        int maxw = 0;
        for (KeyFrame* k : sharing) maxw = k->mnLoopWords > maxw ? k->mnLoopWords : maxw;
        const int minw = maxw * 0.8f;
        std::vector<std::pair<float, KeyFrame*> > scored, acc;
        for (KeyFrame* k : sharing)
            if (k->mnLoopWords > minw) {
                const float si = ref_score(q->mBowVec, k->mBowVec);
                k->mLoopScore = si;
                if (si >= minScore) scored.push_back(std::make_pair(si, k));
            }
        if (scored.empty()) return {};
        float bestAcc = minScore;
        for (auto& e : scored) {
            float best = e.first, sum = e.first;
            KeyFrame* bestKF = e.second;
            for (KeyFrame* k2 : e.second->GetBestCovisibilityKeyFrames(10))
                if (k2->mnLoopQuery == q->mnId && k2->mnLoopWords > minw) {
                    sum += k2->mLoopScore;
                    if (k2->mLoopScore > best) {
                        bestKF = k2;
                        best = k2->mLoopScore;
                    }
                }
            acc.push_back(std::make_pair(sum, bestKF));
            if (sum > bestAcc) bestAcc = sum;
        }
        return retain(acc, bestAcc);
    }
    std::vector<KeyFrame*> reloc(Frame* F) {
        std::vector<KeyFrame*> sharing;
        for (auto& w : F->mBowVec)
            for (KeyFrame* k : inv[w.first]) {
                if (k->mnRelocQuery != F->mnId) {
                    k->mnRelocWords = 0;
                    k->mnRelocQuery = F->mnId;
                    sharing.push_back(k);
                }
                k->mnRelocWords++;
            }
        if (sharing.empty()) return {};
        int maxw = 0;
        for (KeyFrame* k : sharing) maxw = k->mnRelocWords > maxw ? k->mnRelocWords : maxw;
        const int minw = maxw * 0.8f;
        std::vector<std::pair<float, KeyFrame*> > scored, acc;
        for (KeyFrame* k : sharing)
            if (k->mnRelocWords > minw) {
                const float si = ref_score(F->mBowVec, k->mBowVec);
                k->mRelocScore = si;
                scored.push_back(std::make_pair(si, k));
            }
        if (scored.empty()) return {};
        float bestAcc = 0;
        for (auto& e : scored) {
            float best = e.first, sum = e.first;
            KeyFrame* bestKF = e.second;
            for (KeyFrame* k2 : e.second->GetBestCovisibilityKeyFrames(10)) {
                if (k2->mnRelocQuery != F->mnId) continue;
                sum += k2->mRelocScore;
                if (k2->mRelocScore > best) {
                    bestKF = k2;
                    best = k2->mRelocScore;
                }
            }
            acc.push_back(std::make_pair(sum, bestKF));
            if (sum > bestAcc) bestAcc = sum;
        }
        return retain(acc, bestAcc);
    }
};

/* ---- the scene: two identical sets of keyframes ---- */
static uint32_t rng_state = 12345u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static DBoW2::BowVector random_bow(int nwords, int universe, const DBoW2::BowVector* like) {
    DBoW2::BowVector bv;
    if (like)  // most of another vector's words, so that the two score well
        for (auto& e : *like)
            if (rnd() % 10 < 8) bv[e.first] = 1.0 + (rnd() % 1000) / 100.0;
    while ((int)bv.size() < nwords) bv[rnd() % universe] = 0.1 + (rnd() % 1000) / 100.0;
    double norm = 0;
    for (auto& e : bv) norm += fabs(e.second);
    for (auto& e : bv) e.second /= norm;
    return bv;
}

struct Side {
    std::vector<KeyFrame> kf;
    int index(KeyFrame* p) const { return (int)(p - &kf[0]); }
};

static std::vector<int> indices(const Side& s, const std::vector<KeyFrame*>& v) {
    std::vector<int> out;
    for (KeyFrame* p : v) out.push_back(s.index(p));
    return out;
}

static void compare_fields(const Side& a, const Side& b, const char* what) {
    for (size_t i = 0; i < a.kf.size(); i++) {
        const KeyFrame &x = a.kf[i], &y = b.kf[i];
        CHECK(x.mnLoopQuery == y.mnLoopQuery && x.mnLoopWords == y.mnLoopWords &&
                  memcmp(&x.mLoopScore, &y.mLoopScore, 4) == 0,
              "%s: kf %zu loop fields (%lu %d %.9g) vs (%lu %d %.9g)", what, i, x.mnLoopQuery, x.mnLoopWords,
              x.mLoopScore, y.mnLoopQuery, y.mnLoopWords, y.mLoopScore);
        CHECK(x.mnRelocQuery == y.mnRelocQuery && x.mnRelocWords == y.mnRelocWords &&
                  memcmp(&x.mRelocScore, &y.mRelocScore, 4) == 0,
              "%s: kf %zu reloc fields (%lu %d %.9g) vs (%lu %d %.9g)", what, i, x.mnRelocQuery, x.mnRelocWords,
              x.mRelocScore, y.mnRelocQuery, y.mnRelocWords, y.mRelocScore);
    }
}

static int run_device() {
    const int N = 48, NQ = 8, U = 400;
    Side dev, ref;
    dev.kf.resize(N + NQ);
    ref.kf.resize(N + NQ);
    for (int i = 0; i < N + NQ; i++) {
        // keyframes in groups of four similar ones; the queries (the last NQ) resemble a group each
        const DBoW2::BowVector* like = i % 4 ? &dev.kf[i - i % 4].mBowVec : nullptr;
        if (i >= N) like = &dev.kf[(i - N) * 5 % N].mBowVec;
        dev.kf[i].mBowVec = ref.kf[i].mBowVec = random_bow(30 + rnd() % 90, U, like);
        dev.kf[i].mnId = ref.kf[i].mnId = 1 + i;
    }
    for (int i = 0; i < N + NQ; i++) {
        const int nn = rnd() % 13, nc = rnd() % 8;  // up to 12 neighbours: only the best 10 count
        for (int k = 0; k < nn; k++) {
            const int j = rnd() % N;
            dev.kf[i].mOrdered.push_back(&dev.kf[j]);
            ref.kf[i].mOrdered.push_back(&ref.kf[j]);
        }
        for (int k = 0; k < nc; k++) {
            const int j = rnd() % N;
            dev.kf[i].mConnected.insert(&dev.kf[j]);
            ref.kf[i].mConnected.insert(&ref.kf[j]);
        }
    }
    ORBVocabulary voc;
    KeyFrameDatabase db(voc);
    RefDatabase rdb;
    int found = 0, frame_id = 1;
    auto add = [&](int i) { db.add(&dev.kf[i]); rdb.add(&ref.kf[i]); };
    auto erase = [&](int i) { db.erase(&dev.kf[i]); rdb.erase(&ref.kf[i]); };
    auto loop = [&](int q, float minScore) {
        const std::vector<int> a = indices(dev, db.DetectLoopCandidates(&dev.kf[q], minScore));
        const std::vector<int> b = indices(ref, rdb.loop(&ref.kf[q], minScore));
        CHECK(a == b, "DetectLoopCandidates(kf %d): %zu vs %zu candidates", q, a.size(), b.size());
        compare_fields(dev, ref, "loop");
        found += (int)b.size();
    };
    auto reloc = [&](int q) {
        Frame F;
        F.mnId = frame_id++;
        F.mBowVec = dev.kf[q].mBowVec;
        const std::vector<int> a = indices(dev, db.DetectRelocalizationCandidates(&F));
        const std::vector<int> b = indices(ref, rdb.reloc(&F));
        CHECK(a == b, "DetectRelocalizationCandidates(bow of kf %d): %zu vs %zu candidates", q, a.size(), b.size());
        compare_fields(dev, ref, "reloc");
        found += (int)b.size();
    };
    // an empty database
    loop(N, 0.f);
    reloc(N);
    for (int i = 0; i < 40; i++) add(i);
    for (int q = N; q < N + 3; q++) {
        loop(q, 0.02f);
        reloc(q + 3);
    }
    loop(N + 6, 0.9f);  // nothing reaches minScore
    erase(4);
    erase(21);
    reloc(N + 1);
    add(4);  // behind every other keyframe now
    for (int i = 40; i < N; i++) add(i);
    loop(N + 7, 0.f);
    reloc(N + 2);  // reads the mRelocScore left by the earlier frames
    reloc(5);
    loop(9, 0.01f);  // a keyframe of the database as the query (as LoopClosing's mpCurrentKF is)
    db.clear();
    rdb.inv.clear();
    reloc(N);
    CHECK(found >= 10, "only %d candidates in the whole run", found);
    CHECK(amd::LastStatus() == ORBX_OK, "a call failed");
    return 0;
}

static int run_nodevice() {
    ORBVocabulary voc;
    KeyFrameDatabase db(voc);
    std::vector<KeyFrame> kf(4);
    for (int i = 0; i < 4; i++) {
        kf[i].mnId = 1 + i;
        kf[i].mBowVec = random_bow(20, 50, nullptr);
        if (i < 3) db.add(&kf[i]);
    }
    CHECK(amd::LastStatus() == ORBX_EDEVICE, "add records the device status");
    CHECK(db.DetectLoopCandidates(&kf[3], 0.f).empty(), "loop candidates without a device");
    Frame F;
    F.mnId = 1;
    F.mBowVec = kf[3].mBowVec;
    CHECK(db.DetectRelocalizationCandidates(&F).empty(), "reloc candidates without a device");
    CHECK(kf[0].mnLoopWords == 0 && kf[0].mnRelocWords == 0, "nothing written");
    db.erase(&kf[0]);
    db.clear();
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc > 1 && !strcmp(argv[1], "nodevice"))
            run_nodevice();
        else
            run_device();
    } catch (const std::exception& e) {
        printf("FAIL: the drop-in threw: %s\n", e.what());
        return 1;
    } catch (...) {
        printf("FAIL: the drop-in threw\n");
        return 1;
    }
    if (failures) {
        printf("%d FAILURES\n", failures);
        return 1;
    }
    printf("ALL PASS\n");
    return 0;
}
