/* matcher_host.h -- the matchers' host state: the per-thread context (orbm_ctx) and the keyframe cache
 * (orbm_kf_cache), shared by matcher.cpp, slots.cpp and projection.cpp. */
#pragma once
#include <memory>
#include <vector>

#include "host_util.h"
#include "kf_cache.h"
#include "launch.h"

struct orbm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // the host calls' stream, created at the first one: the *_device paths run on the caller's stream, and an idle
    // HIP stream costs the bench's graph streams their step rate (profiles/r04_idle_stream_cost.log). Every host
    // entry point calls ready() first: it makes the context's device current (whatever the calling thread had) and
    // creates the stream there, or fails the call with ORBX_EDEVICE
    int ready() {
        HIPR(hipSetDevice(device));
        if (!stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) {
            stream = nullptr;
            return ORBX_EDEVICE;
        }
        return 0;
    }
    hipStream_t s() const { return stream; }
    orbamd::DevBuf scratch;
    orbamd::DevBuf err;  // device error flag of the *_device calls that validate their input (orbm_check_error)
    std::vector<uint8_t> host;
    void* pinned = nullptr;  // host staging of one call's inputs (one H2D copy) and its results
    void* pinned_dev = nullptr;
    size_t pinned_bytes = 0;
    uint8_t* ensure_pinned(size_t need) {
        if (need <= pinned_bytes) return (uint8_t*)pinned;
        if (stream) (void)hipStreamSynchronize(stream);  // the previous call may still be retiring (wait_call)
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr;
        pinned_dev = nullptr;
        pinned_bytes = 0;
        // fine-grained: the per-call kernels' host writes are visible to the polling host at once
        if (hipHostMalloc(&pinned, need, hipHostMallocCoherent) != hipSuccess) return nullptr;
        if (hipHostGetDevicePointer(&pinned_dev, pinned, 0) != hipSuccess) {
            (void)hipHostFree(pinned);
            pinned = nullptr;
            return nullptr;
        }
        pinned_bytes = need;
        return (uint8_t*)pinned;
    }
    /* device address of byte `off` of the pinned buffer (kernels write results there directly) */
    int32_t* pinned_on_device(size_t off) const { return (int32_t*)((uint8_t*)pinned_dev + off); }
    uint32_t seq = 0;  // call sequence number of k_bow_small's done words (never 0)
    uint32_t next_seq() {
        seq = seq >= orbamd::kSmallSeqMask ? 1u : seq + 1u;
        return seq;
    }
    /* the per-call state words (match_kernels.hip call_tail): ints 16..47 of the zeroed err buffer */
    int32_t* call_state() { return err.as<int32_t>() + 16; }
    /* The epipolar tile cull of the BF triangulation batch calls (orb_tri_cull.h): k_tri_order's layout for
     * k_tri_mfma, one row of S entries per pair. Grown here, before the call enqueues anything (an allocation
     * never lands in a stream capture of the caller's; growing frees the old buffer, which waits for the device).
     * One buffer per context: the calls that share a context are ordered on one stream (include/orbslam_amd.h).
     * tri_cull (orbm_debug_tri_cull): 0 = the full scan, 1 = the cull (default), 2 = the cull + tile counters. */
    orbamd::DevBuf tri_scratch, tri_stats;
    int tri_cull = 1;
    bool tri_culled(int kp_stride) const { return tri_cull && kp_stride <= orbamd::kTriOrdCap; }  // else the full scan
    int tri_plan(int npairs, int kp_stride, orbamd::TriPlan& pl) {
        orbamd::Carve cv;
        const size_t S = (size_t)orbamd::align_up(kp_stride, 64), rows = (size_t)npairs * S;
        const size_t o_perm = cv.take(rows * sizeof(uint16_t)), o_desc = cv.take(rows * 32);
        const size_t o_rec = cv.take(rows * 16), o_tile = cv.take(rows / orbamd::kTriTile * sizeof(orbamd::TriTile));
        if (tri_scratch.ensure(cv.off)) return ORBX_EDEVICE;
        uint8_t* b = tri_scratch.as<uint8_t>();
        pl.permQ = (uint16_t*)(b + o_perm);
        pl.sdesc = b + o_desc;
        pl.srec = (float*)(b + o_rec);
        pl.tiles = (orbamd::TriTile*)(b + o_tile);
        pl.stats = tri_cull == 2 ? tri_stats.as<unsigned long long>() : nullptr;
        pl.S = (int)S;
        return 0;
    }
};

namespace orbamd {

/* One keyframe's immutable per-feature arrays in HBM (orbm_kf_cache): mDescriptors, mvKeysUn (x, y, angle,
 * octave), mvuRight, the FeatureVector's feature list and, for the projection matchers, its 64x48 feature
 * grid (k_grid output). A call holds a shared_ptr to the entries it reads until it has its results. Every
 * per-call kernel writes a result word only after the reads it depends on, and the call returns only once it
 * has seen every result word, so no read of the entry is outstanding when the call drops its reference; an
 * eviction on another thread then frees the buffer with hipFree, which in addition waits for the device. */
struct KfEntry {
    DevBuf buf;
    int n = 0, nfeat = 0, n_nodes = 0;
    bool has_ur = false, has_grid = false;
    size_t o_desc = 0, o_x = 0, o_y = 0, o_ang = 0, o_oct = 0, o_ur = 0, o_feat = 0, o_gs = 0, o_gi = 0;
    size_t o_dnode = 0, o_rnode = 0;  // descriptors / NodeRecs in FeatureVector order (k_bow_small, k_tri_small)
    float min_x = 0, min_y = 0, gw_inv = 0, gh_inv = 0;  // grid bounds / scale the grid was built with
    const uint8_t* at(size_t o) const { return buf.as<uint8_t>() + o; }
    size_t bytes() const { return buf.bytes; }  // what it holds against the cache's capacity (KfLru)
};

}  // namespace orbamd

struct orbm_kf_cache {
    int device = 0;
    hipStream_t stream = nullptr;
    // kind 0: matcher views (orbm_kf_view: + FeatureVector), kind 1: projection views (orbm_frame_view: + grid); the
    // LRU books and their mutex are csrc/kf_cache.h's (also run under ThreadSanitizer by tests/test_sanitizers.py)
    orbamd::KfLru<orbamd::KfEntry> lru;
    explicit orbm_kf_cache(size_t capacity) : lru(capacity) {}
};

namespace orbamd {
/* matcher.cpp: the cached entry of (kind, key) for this call's view, uploaded on `st` when absent or stale */
std::shared_ptr<KfEntry> cache_get(orbm_kf_cache* c, int kind, uint64_t key, const orbm_kf_view* kv,
                                   const orbm_frame_view* fv, hipStream_t st);
}
