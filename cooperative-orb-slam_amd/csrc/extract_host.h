/* extract_host.h -- the extractor's host state (constructor tables, per-frame-size geometry, orbx_handle), shared by
 * extract.cpp, which builds and runs it, and stereo.cpp, which reads the last extraction's pyramid. */
#pragma once
#include <vector>

#include "host_util.h"
#include "launch.h"

namespace orbamd {

inline int cv_round_f(float v) { return (int)lrintf(v); }
inline int cv_floor_f(float v) { int i = (int)v; return i - (i > v); }
inline int cv_ceil_f(float v) { int i = (int)v; return i + (i < v); }

/* ORBextractor constructor tables (ORBextractor.cc:410-470) */
struct Tables {
    int nfeatures, nlevels, ini_th, min_th;
    double scaleFactor;  // double member (ORBextractor.h:100)
    float scale[kMaxLevels], inv_scale[kMaxLevels], sigma2[kMaxLevels], inv_sigma2[kMaxLevels];
    int nfeat[kMaxLevels];
    int umax[16];
    void build(const orbx_params& p) {
        nfeatures = p.nfeatures;
        nlevels = p.nlevels;
        ini_th = p.ini_th_fast;
        min_th = p.min_th_fast;
        scaleFactor = p.scale_factor;
        scale[0] = 1.0f;
        sigma2[0] = 1.0f;
        for (int i = 1; i < nlevels; i++) {
            scale[i] = (float)(scale[i - 1] * scaleFactor);
            sigma2[i] = scale[i] * scale[i];
        }
        for (int i = 0; i < nlevels; i++) {
            inv_scale[i] = 1.0f / scale[i];
            inv_sigma2[i] = 1.0f / sigma2[i];
        }
        float factor = (float)(1.0f / scaleFactor);
        float nDesired = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels));
        int sum = 0;
        for (int l = 0; l < nlevels - 1; l++) {
            nfeat[l] = cv_round_f(nDesired);
            sum += nfeat[l];
            nDesired *= factor;
        }
        nfeat[nlevels - 1] = std::max(nfeatures - sum, 0);
        int v, v0, vmax = cv_floor_f(kHalfPatch * sqrtf(2.f) / 2 + 1);
        int vmin = cv_ceil_f(kHalfPatch * sqrtf(2.f) / 2);
        const double hp2 = kHalfPatch * kHalfPatch;
        for (v = 0; v <= vmax; ++v) umax[v] = (int)lrint(sqrt(hp2 - v * v));
        for (v = kHalfPatch, v0 = 0; v >= vmin; --v) {
            while (umax[v0] == umax[v0 + 1]) ++v0;
            umax[v] = v0;
            ++v0;
        }
    }
};

/* Everything that depends on (W, H): host copies + device copies */
struct Geometry {
    int W = 0, H = 0;
    ExtractParams ep{};
    std::vector<LevelDesc> lv;
    std::vector<CellDesc> cells;
    std::vector<int> coef;
    std::vector<int> bjob_begin;  // blur strip jobs (256 cols x kBlurRows rows) per level
    int nbjobs = 0;
    int bjob_small[kMaxLevels + 1] = {0};  // the same in kBlurRowsSmall-row chunks (run_extract_levels)
    int nbjobs_small = 0;
    int NC = 0, KL = 0, lds_bytes = 0;
    int oct_split = 0;                      // batches: levels [0, oct_split) use NC/KL, [oct_split, L) NC_lo/KL_lo
    int NC_lo = 0, KL_lo = 0, lds_lo = 0;
    int roi_pitch = 0, roi_rows = 0;  // FAST cell LDS staging (max cell ROI)
    int max_pass = 1;                 // ROI staging passes (rows per 64-lane dword pass)
    int tiled_ok[kMaxLevels] = {0};   // level's resize fits the LDS-tiled kernel
    std::vector<int> ptab;            // k_pyramid_frames column-group / row tables
    bool frames_ok = true;            // every level fits k_pyramid_frames
    int band_off = 0;                 // ptab offset of the small-batch row bands ([kPyrBands][kMaxLevels] int2)
    int pyr_rows = 1;                 // tallest level >= 1 (k_pyramid_frames' LDS row table rows)
    DevBuf d_lv, d_cells, d_coef, d_ptab;

    int build(const Tables& T, int W_, int H_);
    void release() { d_lv.release(); d_cells.release(); d_coef.release(); d_ptab.release(); }
};

}  // namespace orbamd

struct orbx_handle {
    orbx_params params;
    orbamd::Tables T;
    int device = 0;
    int max_w = 0, max_h = 0, max_batch = 1;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;  // branches of the extraction graph (run_extract)
    hipEvent_t ev_pyr = nullptr, ev_blur = nullptr;
    hipEvent_t user_ev_pyr = nullptr;   // orbx_set_stage_event(0) / orbx_set_pyramid_event (caller-owned)
    hipEvent_t user_ev_fast = nullptr;  // orbx_set_stage_event(1) (caller-owned)
    orbamd::Geometry geo;
    orbamd::DevBuf pyr, blur, cellkey, cellcnt, lvkey, lvcnt, gscratch, err;
    // host-path staging
    orbamd::DevBuf in_frame, out_kps, out_desc, out_cnt;
    // orbx_compute_stereo_matches staging (host path) and k_stereo's LDS attribute
    orbamd::DevBuf st_buf;
    orbamd::DevBuf stereo_sad;  // orbx_stereo_matches_batch_device: each left keypoint's SAD for the median pass
    int stereo_lds_set = 0;
    // last extraction, for orbx_pyramid_level
    const uint8_t* last_frames = nullptr;
    long long last_fstride = 0;
    int last_pitch = 0, last_nframes = 0;
    hipStream_t last_stream = nullptr;  // stream of the last run_extract
    bool lds_attr_set = false;
    // host path as one captured hipGraph (orbx_extract): pinned staging in / out, replayed per frame
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    int graph_w = 0, graph_h = 0;
    unsigned graph_epoch = 0;   // geometry / buffer epoch the graph was captured at
    unsigned epoch = 1;         // bumped whenever ensure_geometry rebuilds or reallocates
    int graph_warm = 0;         // eager runs at the current epoch (the first one runs uncaptured)
    uint8_t* pin_in = nullptr;  // W*H frame
    uint8_t* pin_out = nullptr; // {cnt, err} + K orbx_kp + K x 32 descriptors
    uint8_t* pin_out_dev = nullptr;  // its device-mapped address: the graph's kernels write the results there
    size_t pin_in_bytes = 0, pin_out_bytes = 0;
    // orbx_set_host_pyramid: the host path also delivers levels 1..L-1 (device layout of one frame) into pin_pyr
    bool host_pyr = false;
    bool host_pyr_valid = false;  // pin_in / pin_pyr hold the last orbx_extract's levels
    uint8_t* pin_pyr = nullptr;
    uint8_t* pin_pyr_dev = nullptr;
    size_t pin_pyr_bytes = 0;
    // orbx_set_host_pyramid_target: caller-owned registered memory receiving the next calls' levels (level 0 at 0,
    // levels 1..L-1 from host_l0_bytes in the device layout) instead of pin_in / pin_pyr; last_target = the one the
    // last call filled (what orbx_host_pyramid_level points into)
    uint8_t* target = nullptr;
    uint8_t* target_dev = nullptr;
    size_t target_bytes = 0;
    uint8_t* last_target = nullptr;
    // orbx_set_camera: the host call's graph also undistorts (k_undistort<true>) and delivers mvKeysUn behind the
    // descriptors of pin_out; un_valid / un_count / un_off describe what the last orbx_extract delivered
    bool cam_on = false;
    orbx_camera cam{};
    bool un_valid = false;
    int un_count = 0;
    size_t un_off = 0;
    // stage profiling (orbx_profile_*)
    bool prof_on = false;
    int prof_mask = 0;  // stages with event pairs (bit k = stage k)
    std::vector<hipEvent_t> prof_ev;  // per profiled call: 5 stages x {start, end}
    int prof_calls = 0;
    double prof_ms[5] = {0, 0, 0, 0, 0};
    int skip_mask = 0;  // orbx_debug_skip_stages (test hook)
    bool serial = false;  // orbx_debug_serial (measurement hook): every stage in order on the caller's stream
    bool alias = false;   // orbx_debug_alias_frames (measurement hook): every frame of a batch is frame 0
};

/* Error words of h->err: kErrSticky (word 0) collects the device batch paths' flags until orbx_check_error
 * takes them (kErrTake, word 32, receives the atomic read-and-clear); kErrExtract (word 2) is the host-buffer
 * extraction's per-call flag, read and cleared by the call's last launch (k_flag_take), so it is clean for the
 * next call; kErrCall (word 1) is the stereo host call's (zeroed and read by that call). A host call never
 * erases an unread batch error. */
constexpr int kErrWordSticky = 0, kErrWordCall = 1, kErrWordExtract = 2, kErrWordTake = 32, kErrWordExtractTake = 33;
constexpr int kErrWordExtractSeq = 40;  // the host extraction's call counter (k_call_done's done word)

namespace orbamd { int ensure_stream(orbx_handle* h, hipStream_t* s); }  // extract.cpp
