/* slots.cpp -- the cross-agent keyframe slot (include/orbslam_amd.h; replaces lcmKeyFrameInfo,
 * lcmKeyFrameInfo.hpp:24-150): its wire format, packing and parsing, and the cross-agent SearchByBoW /
 * SearchForTriangulation over received slots. */
#include "matcher_host.h"

using namespace orbamd;

static SlotLayout slot_layout_of(int cap) {
    SlotLayout L;
    L.cap = cap;
    if (!slot_offsets(cap, L.off, &L.bytes)) L.bytes = 0;
    return L;
}

extern "C" {

size_t orbx_slot_bytes(int cap) {
    uint32_t off[ORBX_SLOT_NSECTIONS], total = 0;
    if (!slot_offsets(cap, off, &total)) return 0;
    return total;
}

int orbx_slot_layout(int cap, orbx_slot_header* hdr) {
    const SlotLayout L = slot_layout_of(cap);
    if (!L.bytes) return ORBX_EARG;
    if (hdr) {
        memset(hdr, 0, sizeof(*hdr));
        hdr->magic = ORBX_SLOT_MAGIC;
        hdr->version = ORBX_SLOT_VERSION;
        hdr->cap = cap;
        hdr->bytes = L.bytes;
        for (int k = 0; k < ORBX_SLOT_NSECTIONS; k++) hdr->off[k] = L.off[k];
    }
    return 0;
}

int orbx_pack_keyframe_device(const orbx_kf_source* src, const orbx_kf_meta* meta, int cap, uint8_t* d_slot,
                              int32_t* d_err, void* stream) {
    if (!src || !meta || !src->kps || !src->desc || !src->count || !d_slot || cap < 1) return ORBX_EARG;
    const SlotLayout L = slot_layout_of(cap);
    if (!L.bytes) return ORBX_EARG;
    HIPR(launch_pack_slot(*src, L, *meta, d_slot, d_err, (hipStream_t)stream));
    return 0;
}

/* host restatement of k_pack_slot, byte for byte */
int orbx_pack_keyframe_host(const orbx_kf_source* s, const orbx_kf_meta* meta, int cap, uint8_t* slot,
                            size_t slot_bytes) {
    if (!s || !meta || !s->count || !slot || cap < 1) return ORBX_EARG;
    const SlotLayout L = slot_layout_of(cap);
    if (!L.bytes || slot_bytes < L.bytes) return ORBX_EARG;
    const int n = *s->count;
    if (n < 0) return ORBX_EARG;
    if (n > 0 && (!s->kps || !s->desc)) return ORBX_EARG;
    const bool has_bow = s->bow_word && s->bow_value;
    const int nbow = has_bow && s->nbow ? *s->nbow : 0;
    const bool has_fv = s->fv_node && s->fv_off && s->fv_feat;
    const int nfv = has_fv && s->nfv ? *s->nfv : 0;
    const int nfeat = has_fv && nfv > 0 ? s->fv_off[nfv] : 0;
    if (n > cap || nbow < 0 || nbow > cap || nfv < 0 || nfv > cap || nfeat < 0 || nfeat > cap) return ORBX_ECAPACITY;
    memset(slot, 0, L.bytes);
    orbx_slot_header* h = (orbx_slot_header*)slot;
    h->magic = ORBX_SLOT_MAGIC;
    h->version = ORBX_SLOT_VERSION;
    h->n = n;
    h->cap = cap;
    h->nbow = has_bow ? nbow : 0;
    h->nfv = nfv;
    h->flags = (s->kun ? ORBX_SLOT_F_KUN : 0u) | ((s->uright && s->depth) ? ORBX_SLOT_F_STEREO : 0u) |
               (s->mp_flags ? ORBX_SLOT_F_MP : 0u) | (has_bow ? ORBX_SLOT_F_BOW : 0u) | (has_fv ? ORBX_SLOT_F_FV : 0u);
    h->bytes = L.bytes;
    for (int k = 0; k < ORBX_SLOT_NSECTIONS; k++) h->off[k] = L.off[k];
    memcpy(slot + kSlotMetaOff, meta, sizeof(*meta));
    orbx_kp* kps = (orbx_kp*)(slot + L.off[ORBX_SLOT_KPS]);
    float* kun = (float*)(slot + L.off[ORBX_SLOT_KUN]);
    float* ur = (float*)(slot + L.off[ORBX_SLOT_URIGHT]);
    float* dp = (float*)(slot + L.off[ORBX_SLOT_DEPTH]);
    for (int i = 0; i < n; i++) {
        kps[i] = s->kps[i];
        kun[2 * i] = s->kun ? s->kun[2 * i] : s->kps[i].x;
        kun[2 * i + 1] = s->kun ? s->kun[2 * i + 1] : s->kps[i].y;
        const bool st = s->uright && s->depth;
        ur[i] = st ? s->uright[i] : -1.f;
        dp[i] = st ? s->depth[i] : -1.f;
    }
    if (n) memcpy(slot + L.off[ORBX_SLOT_DESC], s->desc, 32 * (size_t)n);
    if (s->mp_flags && n) {
        memcpy(slot + L.off[ORBX_SLOT_MPFLAGS], s->mp_flags, (size_t)n);
        if (s->mp_pos) memcpy(slot + L.off[ORBX_SLOT_MPPOS], s->mp_pos, 12 * (size_t)n);
    }
    if (has_bow && nbow) {
        memcpy(slot + L.off[ORBX_SLOT_BOWWORD], s->bow_word, 4 * (size_t)nbow);
        memcpy(slot + L.off[ORBX_SLOT_BOWVALUE], s->bow_value, 8 * (size_t)nbow);
    }
    if (has_fv && nfv) {
        memcpy(slot + L.off[ORBX_SLOT_FVNODE], s->fv_node, 4 * (size_t)nfv);
        int32_t* fo = (int32_t*)(slot + L.off[ORBX_SLOT_FVOFF]);
        for (int k = 0; k <= nfv; k++) fo[k] = std::min(std::max(s->fv_off[k], 0), cap);
        if (nfeat) memcpy(slot + L.off[ORBX_SLOT_FVFEAT], s->fv_feat, 4 * (size_t)nfeat);
    }
    return 0;
}

int orbx_slot_parse(const uint8_t* slot, size_t slot_bytes, orbx_slot_view* v) {
    if (!slot || !v || slot_bytes < kSlotBodyOff) return ORBX_EARG;
    const orbx_slot_header* h = (const orbx_slot_header*)slot;
    if (h->magic != ORBX_SLOT_MAGIC || h->version != ORBX_SLOT_VERSION) return ORBX_EARG;
    const SlotLayout L = slot_layout_of(h->cap);
    if (!L.bytes || h->bytes != L.bytes || (size_t)L.bytes > slot_bytes) return ORBX_EARG;
    for (int k = 0; k < ORBX_SLOT_NSECTIONS; k++)
        if (h->off[k] != L.off[k]) return ORBX_EARG;
    const int n = h->n, cap = h->cap;
    if (n < 0 || n > cap || h->nbow < 0 || h->nbow > cap || h->nfv < 0 || h->nfv > cap) return ORBX_EARG;
    const orbx_kf_meta* m = (const orbx_kf_meta*)(slot + kSlotMetaOff);
    if (m->mnScaleLevels < 1 || m->mnScaleLevels > 16) return ORBX_EARG;
    const orbx_kp* kps = (const orbx_kp*)(slot + L.off[ORBX_SLOT_KPS]);
    for (int i = 0; i < n; i++)
        if (kps[i].octave < 0 || kps[i].octave >= m->mnScaleLevels) return ORBX_EARG;
    const uint32_t* bw = (const uint32_t*)(slot + L.off[ORBX_SLOT_BOWWORD]);
    for (int k = 1; k < h->nbow; k++)
        if (bw[k] <= bw[k - 1]) return ORBX_EARG;
    const uint32_t* fn = (const uint32_t*)(slot + L.off[ORBX_SLOT_FVNODE]);
    const int32_t* fo = (const int32_t*)(slot + L.off[ORBX_SLOT_FVOFF]);
    const int32_t* ff = (const int32_t*)(slot + L.off[ORBX_SLOT_FVFEAT]);
    if (h->nfv > 0) {
        if (fo[0] != 0 || fo[h->nfv] > n) return ORBX_EARG;
        for (int k = 0; k < h->nfv; k++) {
            if (k && fn[k] <= fn[k - 1]) return ORBX_EARG;
            if (fo[k + 1] < fo[k]) return ORBX_EARG;
            for (int j = fo[k]; j < fo[k + 1]; j++)
                if (ff[j] < 0 || ff[j] >= n || (j > fo[k] && ff[j] <= ff[j - 1])) return ORBX_EARG;
        }
    }
    v->hdr = h;
    v->meta = m;
    v->kps = kps;
    v->kun = (const float*)(slot + L.off[ORBX_SLOT_KUN]);
    v->uright = (const float*)(slot + L.off[ORBX_SLOT_URIGHT]);
    v->depth = (const float*)(slot + L.off[ORBX_SLOT_DEPTH]);
    v->desc = slot + L.off[ORBX_SLOT_DESC];
    v->mp_flags = slot + L.off[ORBX_SLOT_MPFLAGS];
    v->mp_pos = (const float*)(slot + L.off[ORBX_SLOT_MPPOS]);
    v->bow_word = bw;
    v->bow_value = (const double*)(slot + L.off[ORBX_SLOT_BOWVALUE]);
    v->fv_node = fn;
    v->fv_off = fo;
    v->fv_feat = ff;
    return 0;
}

int orbm_check_error(orbm_ctx* ctx, void* stream) {
    if (!ctx) return ORBX_EARG;
    HIPR(hipSetDevice(ctx->device));
    // atomic read-and-clear on the device (word 0 -> word 56; the per-call state is words 16..47)
    int flag = 0;
    int32_t* w = ctx->err.as<int32_t>();
    HIPR(launch_flag_take(w, w + 56, (hipStream_t)stream));
    HIPR(hipMemcpyAsync(&flag, w + 56, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPR(hipStreamSynchronize((hipStream_t)stream));
    return flag ? ORBX_EDEVICE : 0;
}

int orbm_search_by_bow_slots_device(orbm_ctx* ctx, const orbx_kf_source* query, int cap1, int nref,
                                    const uint8_t* d_slots, size_t slot_bytes, float nnratio, int check_ori,
                                    int max_nodes, int32_t* d_match, int32_t* d_nmatches, void* stream) {
    if (!ctx || !query || !query->kps || !query->desc || !query->count || !query->fv_node || !query->fv_off ||
        !query->fv_feat || !query->nfv || cap1 < 1 || cap1 > 65535 || nref < 0 || max_nodes < 0 || max_nodes > cap1 ||
        (nref > 0 && (!d_slots || !d_match || !d_nmatches)) || slot_bytes < kSlotBodyOff)
        return ORBX_EARG;
    if (nref == 0) return 0;
    HIPR(hipSetDevice(ctx->device));
    QueryKF q;
    memset(&q, 0, sizeof(q));
    q.kps = query->kps;
    q.mpf = query->mp_flags;
    q.desc = query->desc;
    q.count = query->count;
    q.fv_node = query->fv_node;
    q.fv_off = query->fv_off;
    q.fv_feat = query->fv_feat;
    q.nfv = query->nfv;
    q.cap = cap1;
    hipStream_t st = (hipStream_t)stream;
    HIPR(hipMemsetAsync(d_nmatches, 0, sizeof(int32_t) * (size_t)nref, st));
    HIPR(hipMemsetAsync(d_match, 0xFF, sizeof(int32_t) * (size_t)nref * cap1, st));
    HIPR(launch_bow_slots(q, d_slots, (long long)slot_bytes, nref, nnratio, check_ori ? 1 : 0, max_nodes, d_match,
                          d_nmatches, ctx->err.as<int32_t>(), st));
    return 0;
}

int orbm_search_for_triangulation_slots_device(orbm_ctx* ctx, const orbx_kf_source* query, int cap1, int nref,
                                               const uint8_t* d_slots, size_t slot_bytes, const orbm_slot_geom* geom,
                                               int use_bow, int max_nodes, int32_t* d_match, int32_t* d_nmatches,
                                               void* stream) {
    if (!ctx || !query || !query->kps || !query->desc || !query->count || cap1 < 1 || nref < 0 ||
        (nref > 0 && (!d_slots || !geom || !d_match || !d_nmatches)) || slot_bytes < kSlotBodyOff)
        return ORBX_EARG;
    if (use_bow && (!query->fv_node || !query->fv_off || !query->fv_feat || !query->nfv || max_nodes < 0 ||
                    max_nodes > cap1))
        return ORBX_EARG;
    if (nref == 0) return 0;
    HIPR(hipSetDevice(ctx->device));
    QueryKF q;
    q.kps = query->kps;
    q.kun = (const float2*)query->kun;
    q.uright = query->uright;
    q.mpf = query->mp_flags;
    q.desc = query->desc;
    q.count = query->count;
    q.fv_node = query->fv_node;
    q.fv_off = query->fv_off;
    q.fv_feat = query->fv_feat;
    q.nfv = query->nfv;
    q.cap = cap1;
    hipStream_t st = (hipStream_t)stream;
    HIPR(hipMemsetAsync(d_nmatches, 0, sizeof(int32_t) * (size_t)nref, st));
    if (use_bow) HIPR(hipMemsetAsync(d_match, 0xFF, sizeof(int32_t) * (size_t)nref * cap1, st));
    HIPR(launch_tri_slots(q, d_slots, (long long)slot_bytes, nref, geom, use_bow, max_nodes, d_match, d_nmatches,
                          ctx->err.as<int32_t>(), st));
    return 0;
}

}  // extern "C"
