/*
 * db_kernels.hip -- the keyframe database on gfx950: KeyFrameDatabase::DetectLoopCandidates /
 * DetectRelocalizationCandidates (KeyFrameDatabase.cc:76-309) score the query's BowVector against every
 * keyframe that shares enough words, one ORBVocabulary::score (DBoW2 L1Scoring::score) per keyframe. Here
 * every live entry is scored against every query in one launch; the inverted file's per-keyframe word count
 * (mnLoopWords / mnRelocWords) and the position of the keyframe in lKFsSharingWords (its smallest common
 * word) come out of the same sorted-list intersection.
 *
 * L1Scoring::score walks both vectors in ascending word id and adds, per common word,
 *     score += fabs(vi - wi) - fabs(vi) - fabs(wi)        (double; vi the query's value, wi the entry's)
 * and returns -score / 2.0, which the callers narrow to float. The sum is order dependent, so the kernel
 * adds the terms one after another in ascending word order (no tree, no shuffle reduction).
 */
#include <hip/hip_runtime.h>

#include "orb_db.h"

namespace orbamd {

namespace {

constexpr int kDbThreads = 256;        // k_db_add
constexpr int kDbQueryThreads = 1024;  // k_db_query: 16 waves share one staged query (48 KB of LDS, two blocks per CU)
constexpr int kDbWaves = kDbQueryThreads / 64;

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

/* One add: validates (count in [0, stride], word ids strictly ascending) before anything is copied. A bad
 * input leaves an empty live entry and raises the error word; nothing is read past min(count, stride). */
__global__ __launch_bounds__(kDbThreads) void k_db_add(DbDev db, int e, const uint32_t* __restrict__ word,
                                                       const double* __restrict__ value,
                                                       const int32_t* __restrict__ count) {
    const int tid = threadIdx.x;
    const int n = *count;
    int bad = n < 0 || n > db.stride;
    if (!bad)
        for (int i = tid + 1; i < n; i += kDbThreads) bad |= word[i - 1] >= word[i];
    bad = __syncthreads_or(bad);
    const size_t base = (size_t)e * db.stride;
    if (!bad)
        for (int i = tid; i < n; i += kDbThreads) {
            db.word[base + i] = word[i];
            db.value[base + i] = value[i];
        }
    if (tid == 0) {
        db.count[e] = bad ? 0 : n;
        db.live[e] = 1;
        if (bad) atomicOr(db.err, 1);
    }
}

__global__ void k_db_mark(DbDev db, int e0, int e1, int count, int live) {
    const int e = e0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (e < e1) {
        db.count[e] = count;
        db.live[e] = live;
    }
}

/* grid (entry groups, queries). The block stages its query in LDS; each wave takes entries e = group * 16 + wave,
 * stepping by the grid. Lanes take the entry's words 64 at a time and find each in the query by a branchless
 * lower bound (uniform trip count); the ballot of the hits gives ncommon, and its set bits are walked in lane
 * order (= ascending word id) to add the hit lanes' terms to the running double one after another. */
__global__ __launch_bounds__(kDbQueryThreads) void k_db_query(DbDev db, int nentries, DbQueries qs,
                                                         int32_t* __restrict__ ncommon, float* __restrict__ score,
                                                         uint32_t* __restrict__ first_word) {
    __shared__ uint32_t s_word[kDbMaxWords];
    __shared__ double s_value[kDbMaxWords];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y;
    int nq = *(const int32_t*)(qs.count + (long long)q * qs.count_bytes);
    if (nq < 0 || nq > kDbMaxWords) {  // a query that cannot be staged scores as an empty one
        if (tid == 0 && blockIdx.x == 0) atomicOr(db.err, 1);
        nq = 0;
    }
    const uint32_t* qw = (const uint32_t*)(qs.word + (long long)q * qs.word_bytes);
    const double* qv = (const double*)(qs.value + (long long)q * qs.value_bytes);
    for (int i = tid; i < nq; i += kDbQueryThreads) {
        s_word[i] = qw[i];
        s_value[i] = qv[i];
    }
    __syncthreads();
    int top = 0;  // the largest power of two <= nq
    if (nq > 0) top = 1 << (31 - __builtin_clz(nq));

    for (int e = blockIdx.x * kDbWaves + wave; e < nentries; e += gridDim.x * kDbWaves) {
        const size_t o = (size_t)q * db.capacity + e;
        if (!__builtin_amdgcn_readfirstlane(db.live[e])) {
            if (lane == 0) {
                ncommon[o] = -1;
                score[o] = -0.0f;
                first_word[o] = 0xFFFFFFFFu;
            }
            continue;
        }
        int cnt = __builtin_amdgcn_readfirstlane(db.count[e]);
        cnt = cnt < 0 ? 0 : (cnt > db.stride ? db.stride : cnt);
        const uint32_t* ew = db.word + (size_t)e * db.stride;
        const double* ev = db.value + (size_t)e * db.stride;
        double s = 0.0;
        int nc = 0;
        uint32_t first = 0xFFFFFFFFu;
        // the next chunk's words and values are loaded while this chunk is searched
        uint32_t w_next = lane < cnt ? ew[lane] : 0u;
        double wi_next = lane < cnt ? ev[lane] : 0.0;
        for (int base = 0; base < cnt; base += 64) {
            const bool act = base + lane < cnt;
            const uint32_t w = w_next;
            const double wi = wi_next;
            const int inext = base + 64 + lane;
            w_next = inext < cnt ? ew[inext] : 0u;
            wi_next = inext < cnt ? ev[inext] : 0.0;
            int lo = 0;  // the number of query words below w
            for (int step = top; step; step >>= 1)
                if (lo + step <= nq && s_word[lo + step - 1] < w) lo += step;
            const bool hit = act && lo < nq && s_word[lo] == w;
            const double vi = hit ? s_value[lo] : 0.0;
            const double term = (fabs(vi - wi) - fabs(vi)) - fabs(wi);
            unsigned long long mask = __ballot(hit);
            if (mask && first == 0xFFFFFFFFu)
                first = (uint32_t)__builtin_amdgcn_readlane((int)w, __builtin_ctzll(mask));
            nc += __builtin_popcountll(mask);
            while (mask) {
                const int l = __builtin_ctzll(mask);
                mask &= mask - 1;
                s += readlane_f64(term, l);
            }
        }
        if (lane == 0) {
            ncommon[o] = nc;
            score[o] = (float)(-s / 2.0);
            first_word[o] = first;
        }
    }
}

}  // namespace

hipError_t launch_db_add(const DbDev& db, int entry, const uint32_t* word, const double* value, const int32_t* count,
                         hipStream_t st) {
    hipLaunchKernelGGL(k_db_add, dim3(1), dim3(kDbThreads), 0, st, db, entry, word, value, count);
    return hipGetLastError();
}

hipError_t launch_db_mark(const DbDev& db, int e0, int e1, int count, int live, hipStream_t st) {
    if (e1 <= e0) return hipSuccess;
    hipLaunchKernelGGL(k_db_mark, dim3((e1 - e0 + 255) / 256), dim3(256), 0, st, db, e0, e1, count, live);
    return hipGetLastError();
}

hipError_t launch_db_query(const DbDev& db, int nentries, const DbQueries& q, int nq, int32_t* ncommon, float* score,
                           uint32_t* first_word, hipStream_t st) {
    if (nentries <= 0 || nq <= 0) return hipSuccess;
    // 48 KB of LDS and 16 waves per block: two blocks per CU, 512 on the chip; more entries than that loop in the block
    int groups = (nentries + kDbWaves - 1) / kDbWaves;
    const int cap = (512 + nq - 1) / nq;
    if (groups > cap) groups = cap;
    hipLaunchKernelGGL(k_db_query, dim3(groups, nq), dim3(kDbQueryThreads), 0, st, db, nentries, q, ncommon, score,
                       first_word);
    return hipGetLastError();
}

}  // namespace orbamd
