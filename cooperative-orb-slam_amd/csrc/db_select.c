/*
 * db_select.c -- the candidate selection of KeyFrameDatabase::DetectLoopCandidates (KeyFrameDatabase.cc:107-196)
 * and DetectRelocalizationCandidates (:224-308) over one query's per-entry word counts, scores and first common
 * words (orbdb_query / orbdb_query_device). Plain C, no device: float arithmetic and comparisons as the reference
 * writes them.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/orbslam_amd.h"

typedef struct {
    uint32_t first_word;
    int32_t idx;
} share_t;

/* lKFsSharingWords is filled word by word in ascending word id, each word's list in insertion order
 * (KeyFrameDatabase.cc:86-104): a keyframe enters at its smallest common word, ties in insertion order */
static int share_cmp(const void* a, const void* b) {
    const share_t* x = (const share_t*)a;
    const share_t* y = (const share_t*)b;
    if (x->first_word != y->first_word) return x->first_word < y->first_word ? -1 : 1;
    return x->idx < y->idx ? -1 : (x->idx > y->idx);
}

int orbdb_select_candidates(int mode, int n, const int32_t* ncommon, const float* score, const uint32_t* first_word,
                            const uint8_t* connected, const int32_t* neigh_off, const int32_t* neigh, float min_score,
                            float* last_score, int32_t* out_idx, int* nout) {
    if ((mode != ORBDB_MODE_LOOP && mode != ORBDB_MODE_RELOC) || n < 0 || !nout ||
        (n && (!ncommon || !score || !first_word || !neigh_off || !last_score || !out_idx)))
        return ORBX_EARG;
    *nout = 0;
    if (n == 0) return 0;
    const int loop = mode == ORBDB_MODE_LOOP;
    for (int i = 0; i < n; i++) {
        if (neigh_off[i] < 0 || neigh_off[i + 1] < neigh_off[i]) return ORBX_EARG;
        for (int k = neigh_off[i]; k < neigh_off[i + 1]; k++)
            if (!neigh || neigh[k] < -1 || neigh[k] >= n) return ORBX_EARG;
    }
    share_t* share = (share_t*)malloc(sizeof(share_t) * (size_t)n);
    float* acc = (float*)malloc(sizeof(float) * (size_t)n);
    int32_t* sel = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);   // lScoreAndMatch
    int32_t* best = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);  // lAccScoreAndMatch's keyframes
    uint8_t* added = (uint8_t*)calloc((size_t)n, 1);
    int rc = 0;
    if (!share || !acc || !sel || !best || !added) {
        rc = ORBX_EDEVICE;
        goto done;
    }
    {
        /* keyframes sharing a word; loop mode discards the connected ones (:96-100), which thereby never carry
         * this query's mnLoopQuery */
        int ns = 0, nsel = 0;
        for (int i = 0; i < n; i++)
            if (ncommon[i] > 0 && !(loop && connected && connected[i])) {
                share[ns].first_word = first_word[i];
                share[ns].idx = i;
                ns++;
            }
        if (ns == 0) goto done;
        qsort(share, (size_t)ns, sizeof(share_t), share_cmp);
        int maxCommonWords = 0;
        for (int s = 0; s < ns; s++)
            if (ncommon[share[s].idx] > maxCommonWords) maxCommonWords = ncommon[share[s].idx];
        const int minCommonWords = (int)(maxCommonWords * 0.8f);
        for (int s = 0; s < ns; s++) {
            const int i = share[s].idx;
            if (ncommon[i] > minCommonWords) {
                const float si = score[i];
                last_score[i] = si;
                if (!loop || si >= min_score) sel[nsel++] = i;
            }
        }
        if (nsel == 0) goto done;
        float bestAccScore = loop ? min_score : 0;
        for (int s = 0; s < nsel; s++) {
            const int i = sel[s];
            float bestScore = score[i];
            float accScore = score[i];
            int pBest = i;
            for (int k = neigh_off[i]; k < neigh_off[i + 1]; k++) {
                const int j = neigh[k];
                if (j < 0) continue;
                if (loop) {  // pKF2->mnLoopQuery==pKF->mnId && pKF2->mnLoopWords>minCommonWords (:159)
                    if (!(ncommon[j] > 0 && !(connected && connected[j]) && ncommon[j] > minCommonWords)) continue;
                } else {  // pKF2->mnRelocQuery!=F->mnId (:273): the stored score counts, scored by this call or not
                    if (!(ncommon[j] > 0)) continue;
                }
                accScore += last_score[j];
                if (last_score[j] > bestScore) {
                    pBest = j;
                    bestScore = last_score[j];
                }
            }
            acc[s] = accScore;
            best[s] = pBest;
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        const float minScoreToRetain = 0.75f * bestAccScore;
        int no = 0;
        for (int s = 0; s < nsel; s++)
            if (acc[s] > minScoreToRetain && !added[best[s]]) {
                added[best[s]] = 1;
                out_idx[no++] = best[s];
            }
        *nout = no;
    }
done:
    free(share);
    free(acc);
    free(sel);
    free(best);
    free(added);
    return rc;
}
