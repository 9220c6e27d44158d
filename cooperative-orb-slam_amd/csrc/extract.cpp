/* extract.cpp -- ORBextractor behind orbx_*: the geometry tables of a frame size, the two extraction schedules over
 * extract_kernels.hip, the captured host path (orbx_extract), the host-pyramid ABI and the debug / profile hooks. */
#include "extract_host.h"
#include "orbslam_amd_testing.h"

using namespace orbamd;

static short sat_short(float v) {
    int i = cv_round_f(v);
    return (short)std::min(32767, std::max(-32768, i));
}

/* k_pyramid_frames tables for one level (see PyrColGroup in extract_kernels.hip), appended to ptab: per 4-column
 * group the 8-byte source window W and per output a v_perm selector + tap weights; per row
 * (r0, r1, beta). Returns false if some group's taps do not fit an 8-byte window. */
static bool build_pyr_tables(std::vector<int>& ptab, LevelDesc& d, const int* xofs, const short* alpha, const int* yofs,
                             const short* beta, int xmax, int sw, int sh, int dw, int dh) {
    bool ok = dh <= kPyrMaxRows && (dw + 3) / 4 <= kPyrThreadsMax && sw >= 12;
    const int AU = (int)align_up(sw, 4);
    const int gw = (dw + 3) / 4;
    d.cg_off = (int)ptab.size();
    for (int gi = 0; gi < gw; gi++) {
        int e[12] = {0};
        const int W = std::min(xofs[4 * gi], AU - 8);
        for (int i = 0; i < 4; i++) {
            const int x = std::min(4 * gi + i, dw - 1);
            const int o = xofs[x] - W;
            const bool two = x < xmax;  // second tap has a non-zero weight
            if (o < 0 || o > 7 || (two && o + 1 > 7)) ok = false;
            const int o1 = std::min(o + 1, 7);
            e[i] = (o & 7) | (0x0c << 8) | (o1 << 16) | (0x0c << 24);
            const short a0 = two ? alpha[2 * x] : (short)2048, a1 = two ? alpha[2 * x + 1] : (short)0;
            e[4 + i] = (int)(((uint32_t)(uint16_t)a1 << 16) | (uint16_t)a0);
        }
        e[8] = W;
        e[9] = AU - 4;  // last dword of the row (clamp of the window's third dword)
        ptab.insert(ptab.end(), e, e + 12);
    }
    d.rt_off = (int)ptab.size();
    for (int y = 0; y < dh; y++) {
        const int r0 = std::min(std::max(yofs[y], 0), sh - 1), r1 = std::min(std::max(yofs[y] + 1, 0), sh - 1);
        const int b = (int)(((uint32_t)(uint16_t)beta[2 * y + 1] << 16) | (uint16_t)beta[2 * y]);
        const int e[4] = {r0, r1, b, 0};
        ptab.insert(ptab.end(), e, e + 4);
    }
    return ok;
}

int Geometry::build(const Tables& T, int W_, int H_) {
    W = W_;
    H = H_;
    const int L = T.nlevels;
    lv.assign(L, LevelDesc{});
    cells.clear();
    coef.clear();
    ptab.clear();
    frames_ok = true;
    long long pyr_off = 0, blur_off = 0;
    int key_begin = 0, kp_off = 0;
    int maxnode = 0;
    for (int l = 0; l < L; l++) {
        LevelDesc& d = lv[l];
        // ComputePyramid (ORBextractor.cc:1111-1112)
        d.w = cv_round_f((float)W * T.inv_scale[l]);
        d.h = cv_round_f((float)H * T.inv_scale[l]);
        if (d.w < 62 || d.h < 62 || d.w > 4096 || d.h > 4096) return ORBX_EARG;
        d.pitch = (int)align_up(d.w, 64);
        d.pyr_off = l == 0 ? 0 : pyr_off;
        if (l > 0) pyr_off += align_up((long long)d.pitch * d.h, 256);
        d.blur_off = blur_off;
        blur_off += align_up((long long)d.pitch * d.h, 256);
        d.scale = T.scale[l];
        d.patch_size = (float)(int)(kPatchSize * T.scale[l]);
        d.blur_vec_end = d.w & ~3;
        // resize tables from level l-1 (OpenCV resize(), INTER_LINEAR, 8U)
        if (l > 0) {
            const int sw = lv[l - 1].w, sh = lv[l - 1].h, dw = d.w, dh = d.h;
            d.coef_off = (int)coef.size();
            coef.resize(coef.size() + 2 * dw + 2 * dh);
            int* xofs = coef.data() + d.coef_off;
            short* alpha = (short*)(xofs + dw);
            int* yofs = xofs + 2 * dw;
            short* beta = (short*)(yofs + dh);
            const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
            int xmax = dw;
            for (int dx = 0; dx < dw; dx++) {
                float fx = (float)((dx + 0.5) * scale_x - 0.5);
                int sx = cv_floor_f(fx);
                fx -= sx;
                if (sx < 0) { fx = 0; sx = 0; }
                if (sx + 1 >= sw) {
                    xmax = std::min(xmax, dx);
                    if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
                }
                xofs[dx] = sx;
                alpha[2 * dx] = sat_short((1.f - fx) * 2048);
                alpha[2 * dx + 1] = sat_short(fx * 2048);
            }
            for (int dy = 0; dy < dh; dy++) {
                float fy = (float)((dy + 0.5) * scale_y - 0.5);
                int sy = cv_floor_f(fy);
                fy -= sy;
                yofs[dy] = sy;
                beta[2 * dy] = sat_short((1.f - fy) * 2048);
                beta[2 * dy + 1] = sat_short(fy * 2048);
            }
            int se = 0;
            while (se <= dw - 16) se += 16;
            while (se < dw - 4) se += 4;
            d.xmax = xmax;
            d.simd_end = se;
            tiled_ok[l] = resize_tile_fits(xofs, yofs, sw, sh, dw, dh);
            frames_ok = frames_ok && build_pyr_tables(ptab, d, xofs, alpha, yofs, beta, xmax, sw, sh, dw, dh);
            // OpenCV switches INTER_LINEAR to INTER_AREA for exact 2x downscales; unsupported
            if (std::abs(scale_x - 2.0) < 1e-15 && std::abs(scale_y - 2.0) < 1e-15) return ORBX_EARG;
        }
        // FAST cell grid (ORBextractor.cc:769-806)
        const float Wc = 30;
        const int minBorderX = kEdgeThreshold - 3, minBorderY = minBorderX;
        const int maxBorderX = d.w - kEdgeThreshold + 3, maxBorderY = d.h - kEdgeThreshold + 3;
        const float width = (float)(maxBorderX - minBorderX), height = (float)(maxBorderY - minBorderY);
        const int nCols = (int)(width / Wc), nRows = (int)(height / Wc);
        if (nCols <= 0 || nRows <= 0) return ORBX_EARG;
        const int wCell = (int)ceilf(width / nCols), hCell = (int)ceilf(height / nRows);
        d.cell_begin = (int)cells.size();
        d.key_begin = key_begin;
        int kc = 0;
        for (int i = 0; i < nRows; i++) {
            const float iniY = (float)(minBorderY + i * hCell);
            float maxY = iniY + hCell + 6;
            if (iniY >= maxBorderY - 3) continue;
            if (maxY > maxBorderY) maxY = (float)maxBorderY;
            for (int j = 0; j < nCols; j++) {
                const float iniX = (float)(minBorderX + j * wCell);
                float maxX = iniX + wCell + 6;
                if (iniX >= maxBorderX - 6) continue;
                if (maxX > maxBorderX) maxX = (float)maxBorderX;
                CellDesc c;
                c.level = l;
                c.x0 = (int)iniX;
                c.y0 = (int)iniY;
                c.w = (int)maxX - c.x0;
                c.h = (int)maxY - c.y0;
                if (c.w > kRoiMax || c.h > kRoiMax) return ORBX_EARG;
                c.xoff = j * wCell;
                c.yoff = i * hCell;
                const int bw = std::max(c.w - 6, 0), bh = std::max(c.h - 6, 0);
                c.cap = ((bw + 1) / 2) * ((bh + 1) / 2);
                c.slot = key_begin + kc;
                kc += c.cap;
                c.D = (c.w + 3) / 4;
                c.rpp = 64 / c.D;
                c.magD = (65536 + c.D - 1) / c.D;
                c.G = (bw + 6) / 4;
                c.rpc = c.G > 0 ? 64 / c.G : 1;
                c.magG = c.G > 0 ? (65536 + c.G - 1) / c.G : 0;
                for (int ln = 0; ln < 64; ln++)  // the magic divisions are exact (checked)
                    if ((ln * c.magD) >> 16 != ln / c.D || (c.G > 0 && (ln * c.magG) >> 16 != ln / c.G))
                        return ORBX_EARG;
                cells.push_back(c);
            }
        }
        d.ncells = (int)cells.size() - d.cell_begin;
        d.key_cap = kc;
        key_begin += (int)align_up(kc, 64);
        // DistributeOctTree roots (ORBextractor.cc:542-545)
        d.minX = minBorderX;
        d.maxX = maxBorderX;
        d.minY = minBorderY;
        d.maxY = maxBorderY;
        d.nIni = (int)roundf((float)(maxBorderX - minBorderX) / (maxBorderY - minBorderY));
        if (d.nIni <= 0) return ORBX_EARG;
        d.hX = (float)(maxBorderX - minBorderX) / d.nIni;
        d.N = T.nfeat[l];
        d.node_cap = std::max(d.N + 3, 4 * d.nIni);
        d.kp_off = kp_off;
        d.kp_cap = d.node_cap;
        kp_off += d.kp_cap;
        maxnode = std::max(maxnode, d.node_cap);
    }
    roi_pitch = 4;
    roi_rows = 1;
    max_pass = 1;
    for (const CellDesc& c : cells) {
        roi_pitch = std::max(roi_pitch, (int)align_up(c.w, 4));
        roi_rows = std::max(roi_rows, c.h);
        const int D = (c.w + 3) / 4, rpp = 64 / D;
        max_pass = std::max(max_pass, (c.h + rpp - 1) / rpp);
    }
    if (max_pass > 24) return ORBX_EARG;
    ep.L = L;
    ep.ncells = (int)cells.size();
    ep.keys_per_frame = key_begin;
    ep.kp_per_frame = kp_off;
    ep.ini_th = T.ini_th;
    ep.min_th = T.min_th;
    ep.pyr_frame_bytes = align_up(pyr_off, 256);
    ep.blur_frame_bytes = align_up(blur_off, 256);
    ep.umax_packed = 0;
    for (int v = 0; v < 16; v++) {
        ep.umax[v] = T.umax[v];
        ep.umax_packed |= (unsigned long long)(T.umax[v] & 15) << (4 * v);
    }
    // IC_Angle lane masks (k_describe): row ri = v + 15 (0..31), column group g (u = -15+4g+i):
    // {packed (u+15) inside the circular patch, packed 1 inside} (ORBextractor.cc:77-104)
    ep.ic_off = (int)ptab.size();
    for (int ri = 0; ri < 32; ri++) {
        const int v = ri - 15, av = v < 0 ? -v : v;
        for (int gq = 0; gq < 8; gq++) {
            uint32_t uw = 0, m1 = 0;
            for (int i = 0; i < 4; i++) {
                const int u = -15 + 4 * gq + i, au = u < 0 ? -u : u;
                if (av <= 15 && au <= 15 && au <= T.umax[av]) {
                    uw |= (uint32_t)(u + 15) << (8 * i);
                    m1 |= 1u << (8 * i);
                }
            }
            ptab.push_back((int)uw);
            ptab.push_back((int)m1);
        }
    }
    bjob_begin.assign(L + 1, 0);
    for (int l = 0; l < L; l++)
        bjob_begin[l + 1] = bjob_begin[l] + ((lv[l].w + 255) / 256) * ((lv[l].h + kBlurRows - 1) / kBlurRows);
    nbjobs = bjob_begin[L];
    int bs = 0;  // the same jobs in kBlurRowsSmall-row chunks (small batches)
    for (int l = 0; l <= kMaxLevels; l++) {
        ep.kp_off[l] = l < L ? lv[l].kp_off : kp_off;
        ep.bjob_begin[l] = l <= L ? bjob_begin[l] : nbjobs;
        bjob_small[l] = bs;
        if (l < L) bs += ((lv[l].w + 255) / 256) * ((lv[l].h + kBlurRowsSmall - 1) / kBlurRowsSmall);
    }
    nbjobs_small = bjob_small[L];
    pyr_rows = 1;
    for (int l = 1; l < L; l++) pyr_rows = std::max(pyr_rows, lv[l].h);
    // row bands of the banded pyramid: band b of B owns rows [b h / B, (b + 1) h / B) of every level and also
    // makes the rows its own higher levels read (the (r0, r1) of k_pyramid_frames' row table), so each
    // workgroup only reads back rows it wrote itself
    auto band_table = [&](int B) {
        const int off = (int)ptab.size();
        std::vector<int> bt(2 * B * kMaxLevels, 0);
        for (int b = 0; b < B; b++) {
            int nlo = 0, nhi = 0;  // rows of level l that level l + 1's range reads ([nlo, nhi), empty at the top)
            for (int l = L - 1; l >= 1; l--) {
                const int h = lv[l].h;
                int lo = (int)((long long)b * h / B), hi = (int)((long long)(b + 1) * h / B);
                if (nhi > nlo) {
                    lo = hi > lo ? std::min(lo, nlo) : nlo;
                    hi = std::max(hi, nhi);
                }
                bt[2 * (b * kMaxLevels + l)] = lo;
                bt[2 * (b * kMaxLevels + l) + 1] = hi;
                nlo = nhi = 0;
                if (hi > lo && l > 1) {  // this range's source rows in level l - 1
                    const int* rt = &ptab[lv[l].rt_off];
                    nlo = rt[4 * lo];
                    nhi = rt[4 * (hi - 1) + 1] + 1;
                }
            }
        }
        ptab.insert(ptab.end(), bt.begin(), bt.end());
        return off;
    };
    band_off = frames_ok ? band_table(kPyrBands) : 0;
    // octree LDS: node arrays (92 B/node, NC pow2) + keys (7 B/key)
    NC = 1;
    while (NC < maxnode) NC <<= 1;
    const int node_bytes = 76 * NC;
    // keys of a level stay in LDS up to KL, larger levels use global scratch. KL is sized so a workgroup
    // fits 32 KB when that still leaves >= 1024 keys (five octree workgroups per CU beside the other
    // graphs' kernels; 1888 keys at NC = 256 cover a 640x480 / 1000-feature level 0), else up to 2048.
    if (node_bytes + 7 * 256 > 160 * 1024) return ORBX_EARG;
    auto key_lds = [](int nc, int* kl, int* lds) {
        const int nb = 76 * nc;
        const int kl32 = ((32 * 1024 - nb - 64) / 7) & ~15;
        *kl = kl32 >= 1024 ? std::min(2048, kl32) : std::min(2048, ((160 * 1024 - nb) / 7) & ~15);
        *lds = nb + 7 * *kl;
    };
    key_lds(NC, &KL, &lds_bytes);
    // batches: the levels whose node tables fit 256 entries (all but level 0 of a 1200- or 2000-feature
    // extractor) take their own launch with 256-node tables and 256-thread workgroups, instead of every level
    // carrying the largest level's 512-node tables and 53 KB of LDS (C3 / C4: 2.4 ms per 1024-frame launch)
    oct_split = L;
    while (oct_split > 0 && lv[oct_split - 1].node_cap <= 256) oct_split--;
    NC_lo = NC;
    KL_lo = KL;
    lds_lo = lds_bytes;
    if (oct_split > 0 && oct_split < L) {
        int mx = 0;
        for (int l = oct_split; l < L; l++) mx = std::max(mx, lv[l].node_cap);
        NC_lo = 1;
        while (NC_lo < mx) NC_lo <<= 1;
        key_lds(NC_lo, &KL_lo, &lds_lo);
    } else {
        oct_split = 0;  // one launch: every level fits the same tables
    }
    // upload
    if (d_lv.ensure(sizeof(LevelDesc) * L) || d_cells.ensure(sizeof(CellDesc) * cells.size()) ||
        d_coef.ensure(sizeof(int) * std::max<size_t>(coef.size(), 1)) ||
        d_ptab.ensure(sizeof(int) * std::max<size_t>(ptab.size(), 4)))
        return ORBX_EDEVICE;
    HIPR(hipMemcpy(d_lv.p, lv.data(), sizeof(LevelDesc) * L, hipMemcpyHostToDevice));
    HIPR(hipMemcpy(d_cells.p, cells.data(), sizeof(CellDesc) * cells.size(), hipMemcpyHostToDevice));
    if (!coef.empty()) HIPR(hipMemcpy(d_coef.p, coef.data(), sizeof(int) * coef.size(), hipMemcpyHostToDevice));
    if (!ptab.empty()) HIPR(hipMemcpy(d_ptab.p, ptab.data(), sizeof(int) * ptab.size(), hipMemcpyHostToDevice));
    return 0;
}

static const int kProfMaxCalls = 4096;
static const int kHostCopyBlocks = 16;  // octree-launch workgroups (1024 threads) copying the host path's pyramid
// pin_out byte offset of the host copy's destination pointer: the captured graph's copy workgroups read it at run time,
// so a call can deliver its levels into another buffer (orbx_set_host_pyramid_target) without a new capture
static const int kPinOutCopyDst = 48;

/* bytes of a host pyramid target: level 0 (w x h, contiguous) rounded up to 256, then levels 1..L-1 as on the device */
static size_t host_l0_bytes(const orbx_handle* h) { return align_up((size_t)h->geo.W * h->geo.H, 256); }

/* stage k = {pyramid, fast_cells, octree, blur, describe}; e = 0 start / 1 end, recorded on the
 * stream the stage's kernel is launched on (the overlapped schedule is kept) */
static int prof_mark(orbx_handle* h, int k, int e, hipStream_t st) {
    if (!h->prof_on || !((h->prof_mask >> k) & 1)) return 0;
    if (h->prof_calls >= kProfMaxCalls) return 0;
    const size_t need = (size_t)(h->prof_calls + 1) * 10;
    while (h->prof_ev.size() < need) {
        hipEvent_t ev;
        HIPR(hipEventCreate(&ev));
        h->prof_ev.push_back(ev);
    }
    HIPR(hipEventRecord(h->prof_ev[(size_t)h->prof_calls * 10 + 2 * k + e], st));
    return 0;
}

static int ensure_geometry(orbx_handle* h, int W, int H, int nframes) {
    if (nframes < 1 || nframes > h->max_batch) return ORBX_EARG;
    if (h->geo.W != W || h->geo.H != H) {
        h->epoch++;
        int rc = h->geo.build(h->T, W, H);
        if (rc) { h->geo.W = h->geo.H = 0; return rc; }
    }
    const ExtractParams& ep = h->geo.ep;
    const size_t B = (size_t)h->max_batch;
    const void* before[7] = {h->pyr.p, h->blur.p, h->cellkey.p, h->cellcnt.p, h->lvkey.p, h->lvcnt.p, h->gscratch.p};
    const void* err_before = h->err.p;
    // the blurred pyramid is only for frames the fused describe cannot take (unaligned level-0 rows): allocated at the
    // first such call (ensure_blur), and kept sized here once it exists
    if (h->pyr.ensure(B * ep.pyr_frame_bytes) || (h->blur.p && h->blur.ensure(B * ep.blur_frame_bytes)) ||
        h->cellkey.ensure(B * ep.keys_per_frame * 4) || h->cellcnt.ensure(B * ep.ncells * 4) ||
        h->lvkey.ensure(B * ep.kp_per_frame * 4) || h->lvcnt.ensure((B * ep.L + kMaxLevels) * 4) ||
        h->gscratch.ensure(B * (size_t)ep.keys_per_frame * 8) || h->err.ensure(256))
        return ORBX_EDEVICE;
    if (h->err.p != err_before && hipMemset(h->err.p, 0, 256) != hipSuccess) return ORBX_EDEVICE;  // sticky flag starts clear
    const void* after[7] = {h->pyr.p, h->blur.p, h->cellkey.p, h->cellcnt.p, h->lvkey.p, h->lvcnt.p, h->gscratch.p};
    if (memcmp(before, after, sizeof(before))) h->epoch++;
    if (h->geo.lds_bytes > 64 * 1024 && !h->lds_attr_set) {
        HIPR(octree_setup(h->geo.lds_bytes));
        h->lds_attr_set = true;
    }
    return 0;
}

/* the separate blur's buffer (k_blur_strips / k_fast_blur + k_describe), allocated at the first extraction of frames whose
 * level-0 rows are not 4-byte aligned: every aligned frame blurs inside describe's LDS, so most handles never hold the
 * ~1 MB per 640x480 frame of max_batch (3 GB at the bench's 3 x 1024 frames). A host-call graph captured before holds no
 * blur launch, so a reallocation only bumps the epoch like any other buffer change. */
static int ensure_blur(orbx_handle* h) {
    const void* before = h->blur.p;
    if (h->blur.ensure((size_t)h->max_batch * h->geo.ep.blur_frame_bytes)) return ORBX_EDEVICE;
    if (h->blur.p != before) h->epoch++;
    return 0;
}

static int launch_pyramid(orbx_handle* h, const ExtractParams& ep, const uint8_t* d_frames, long long fstride,
                          int pitch, int nframes, hipStream_t st) {
    Geometry& g = h->geo;
    // pyramid levels 1..L-1 (ORBextractor.cc:1107-1132) of 4-byte-aligned frames: whole-frame workgroups for
    // large batches, row-band workgroups (kPyrBands per frame) for small ones; per-level kernels otherwise
    const bool aligned = ((uintptr_t)d_frames & 3) == 0 && (fstride & 3) == 0 && (pitch & 3) == 0;
    if (g.frames_ok && aligned && ep.L > 1) {
        int max_groups = 1;
        for (int l = 1; l < ep.L; l++) max_groups = std::max(max_groups, (g.lv[l].w + 3) / 4);
        const bool banded = nframes < kPyrFramesMinBatch;
        HIPR(launch_pyramid_frames(d_frames, fstride, pitch, h->pyr.as<uint8_t>(), ep, g.d_lv.as<LevelDesc>(),
                                   g.d_ptab.as<int>(), g.pyr_rows, max_groups, nframes, st,
                                   banded ? (const int2*)(g.d_ptab.as<int>() + g.band_off) : nullptr,
                                   banded ? kPyrBands : 0));
        return 0;
    }
    for (int l = 1; l < ep.L; l++) {
        const LevelDesc& s = g.lv[l - 1];
        const LevelDesc& d = g.lv[l];
        const uint8_t* src = l == 1 ? d_frames : h->pyr.as<uint8_t>() + s.pyr_off;
        const long long sfs = l == 1 ? fstride : ep.pyr_frame_bytes;
        const int sp = l == 1 ? pitch : s.pitch;
        if (g.tiled_ok[l])
            HIPR(launch_resize_tiled(src, sfs, sp, s.w, s.h, h->pyr.as<uint8_t>() + d.pyr_off, ep.pyr_frame_bytes,
                                     d.pitch, d.w, d.h, g.d_coef.as<int>() + d.coef_off, d.xmax, d.simd_end, nframes,
                                     st));
        else
            HIPR(launch_resize(src, sfs, sp, s.w, s.h, h->pyr.as<uint8_t>() + d.pyr_off, ep.pyr_frame_bytes, d.pitch,
                               d.w, d.h, g.d_coef.as<int>() + d.coef_off, d.xmax, d.simd_end, nframes, st));
    }
    return 0;
}

static int launch_fast(orbx_handle* h, const ExtractParams& ep, const uint8_t* d_frames, long long fstride, int pitch,
                       int cell_lo, int cell_hi, int nframes, hipStream_t st) {
    Geometry& g = h->geo;
    HIPR(launch_fast_cells2(d_frames, fstride, pitch, h->pyr.as<uint8_t>(), ep, g.d_lv.as<LevelDesc>(),
                            g.d_cells.as<CellDesc>(), h->cellkey.as<uint32_t>(), h->cellcnt.as<int>(), g.roi_pitch,
                            g.roi_rows, g.max_pass, cell_lo, cell_hi, nframes, st));
    return 0;
}

/* the octree over levels [level0, level0 + nlevels) (nlevels -1: up to the top) with NC-entry node tables and KL keys
 * in LDS; copy: the host path's pyramid copy, riding on the launch (extract_graph) */
static int launch_octree_levels(orbx_handle* h, const ExtractParams& ep, int level0, int nlevels, int NC, int KL,
                                int lds_bytes, int* errp, int nframes, hipStream_t st, const HostCopy* copy = nullptr) {
    Geometry& g = h->geo;
    HIPR(launch_octree(ep, g.d_lv.as<LevelDesc>(), g.d_cells.as<CellDesc>(), h->cellkey.as<uint32_t>(),
                       h->cellcnt.as<int>(), h->lvkey.as<uint32_t>(), h->lvcnt.as<int>(), h->gscratch.as<uint8_t>(),
                       (long long)ep.keys_per_frame * 8, NC, KL, lds_bytes, errp, nframes, st, level0, nlevels, copy));
    return 0;
}

/* the blur inside describe (k_describe_blur, no blurred pyramid in HBM) takes every frame whose level-0 rows are
 * 4-byte aligned; other frames blur each level in k_blur_strips and describe from it */
static int launch_describe_any(orbx_handle* h, const ExtractParams& ep, bool fused, const uint8_t* d_frames,
                               long long fstride, int pitch, orbx_kp* d_kps, uint8_t* d_desc, int32_t* d_counts,
                               int kp_stride, int nframes, hipStream_t st) {
    Geometry& g = h->geo;
    const LevelDesc* dl = g.d_lv.as<LevelDesc>();
    if (fused)
        HIPR(launch_describe_blur(d_frames, fstride, pitch, h->pyr.as<uint8_t>(), ep, dl, h->lvkey.as<uint32_t>(),
                                  h->lvcnt.as<int>(), d_kps, d_desc, d_counts, kp_stride, g.d_ptab.as<int>(),
                                  nframes, st));
    else
        HIPR(launch_describe(d_frames, fstride, pitch, h->pyr.as<uint8_t>(), h->blur.as<uint8_t>(), ep, dl,
                             h->lvkey.as<uint32_t>(), h->lvcnt.as<int>(), d_kps, d_desc, d_counts, kp_stride,
                             g.d_ptab.as<int>(), nframes, st));
    return 0;
}

/* what orbx_pyramid_level and the stereo matcher read of the last extraction */
static void note_last(orbx_handle* h, const uint8_t* d_frames, long long fstride, int pitch, int nframes,
                      hipStream_t st) {
    h->last_frames = d_frames, h->last_fstride = fstride, h->last_pitch = pitch;
    h->last_nframes = nframes, h->last_stream = st;
}

/* Small batches (the Tracking thread's one frame per call, ORBextractor.cc:1043-1105): every stage in order on the
 * caller's queue -- the pyramid in kPyrBands row bands per frame (one launch); FAST over every cell; the octree over
 * every level; the blur inside describe (k_describe_blur). Unaligned frames run FAST and the blur in 14-row chunks
 * (4.5x the waves of the batch form's 63-row chunks: one frame's blur is one chunk's row chain) in one launch
 * (k_fast_blur), then describe. A single queue because the graph executor turns every edge between queues into a
 * marker behind all the work already submitted to the source queue (~10 us per hop in the kernel trace, and a
 * side branch started only once its marker came up), and streams share the process's 4 hardware queues; every
 * branch layout measured slower than the one queue (profiles/r04_latency_branches.log, r04_latency_lists.log,
 * r04m_latency_ab.log), and so did a single launch for levels 2.. whose tiles wait on each other's counters
 * (r04_latency_chain_reverted.log). */
static int run_extract_levels(orbx_handle* h, const ExtractParams& ep, int nframes, const uint8_t* d_frames,
                              long long fstride, int pitch, orbx_kp* d_kps, uint8_t* d_desc, int32_t* d_counts,
                              int kp_stride, hipStream_t st, int* errp, hipEvent_t ev_pyr, hipEvent_t ev_fast,
                              const HostCopy* copy) {
    Geometry& g = h->geo;
    const LevelDesc* dl = g.d_lv.as<LevelDesc>();
    if (!(h->skip_mask & 1) && launch_pyramid(h, ep, d_frames, fstride, pitch, nframes, st)) return ORBX_EDEVICE;
    if (ev_pyr) HIPR(hipEventRecord(ev_pyr, st));  // orbx_set_pyramid_event: right after the pyramid launch
    const bool fused = describe_blur_ok(d_frames, fstride, pitch);
    if (fused) {  // FAST -> octree -> blur + describe
        if (!(h->skip_mask & 2) && launch_fast(h, ep, d_frames, fstride, pitch, 0, ep.ncells, nframes, st))
            return ORBX_EDEVICE;
        if (ev_fast) HIPR(hipEventRecord(ev_fast, st));
    } else {
        if (ensure_blur(h)) return ORBX_EDEVICE;
        ExtractParams eb = ep;  // the blur's short-chunk job table
        for (int i = 0; i <= kMaxLevels; i++) eb.bjob_begin[i] = g.bjob_small[i];
        if (!(h->skip_mask & 2) && !(h->skip_mask & 8)) {  // FAST and the blur in one launch
            HIPR(launch_fast_blur(d_frames, fstride, pitch, h->pyr.as<uint8_t>(), ep, dl, g.d_cells.as<CellDesc>(),
                                  h->cellkey.as<uint32_t>(), h->cellcnt.as<int>(), g.roi_pitch, g.roi_rows, g.max_pass,
                                  h->blur.as<uint8_t>(), eb, g.nbjobs_small, nframes, st));
            if (ev_fast) HIPR(hipEventRecord(ev_fast, st));
        } else {
            if (!(h->skip_mask & 2) && launch_fast(h, ep, d_frames, fstride, pitch, 0, ep.ncells, nframes, st))
                return ORBX_EDEVICE;
            if (!(h->skip_mask & 8))
                HIPR(launch_blur_strips(d_frames, fstride, pitch, h->pyr.as<uint8_t>(), h->blur.as<uint8_t>(), eb, dl,
                                        0, g.nbjobs_small, nullptr, nframes, st, kBlurRowsSmall));
        }
    }
    if (!(h->skip_mask & 4) && launch_octree_levels(h, ep, 0, -1, g.NC, g.KL, g.lds_bytes, errp, nframes, st, copy))
        return ORBX_EDEVICE;
    if (!(h->skip_mask & 16) &&
        launch_describe_any(h, ep, fused, d_frames, fstride, pitch, d_kps, d_desc, d_counts, kp_stride, nframes, st))
        return ORBX_EDEVICE;
    return 0;
}

/* a handle's own HIP stream (h->stream: host calls; h->side: the separate blur of frames the fused describe cannot
 * take), created on the handle's device at its first use */
int orbamd::ensure_stream(orbx_handle* h, hipStream_t* s) {
    if (*s) return 0;
    HIPR(hipSetDevice(h->device));
    if (hipStreamCreateWithFlags(s, hipStreamNonBlocking) != hipSuccess) {
        *s = nullptr;
        return ORBX_EDEVICE;
    }
    return 0;
}

/* ORBextractor::operator() for a batch. Dependencies between the stages:
 *
 *   st   (caller): pyramid(1..L-1) -> [ev_pyr] FAST(all cells) -> octree -> [ev_blur] describe
 *   side         :                   [ev_pyr] blur(all levels) ---------> [ev_blur]
 *
 * The blur needs only the pyramid, so it runs beside FAST and the octree (whose workgroups are
 * barrier/latency-bound); describe joins both. (The reference blurs only levels that kept
 * keypoints (ORBextractor.cc:1081); blurring every level changes no output, since describe
 * reads only levels with keypoints.) h->serial (orbx_debug_serial, a measurement hook) runs every
 * stage in order on `st`, so each kernel runs alone. */
static int run_extract(orbx_handle* h, int nframes, const uint8_t* d_frames, long long fstride, int pitch,
                       orbx_kp* d_kps, uint8_t* d_desc, int32_t* d_counts, int kp_stride, hipStream_t st,
                       bool host_call = true, bool mapped_out = false, const HostCopy* copy = nullptr) {
    Geometry& g = h->geo;
    // the L2-residency bound (orbx_debug_alias_frames): every frame of the batch reads frame 0's image and
    // shares one pyramid / blur buffer, so the stages read lines other workgroups of the launch keep in L2
    ExtractParams ep_alias = g.ep;
    if (h->alias) {
        ep_alias.pyr_frame_bytes = 0;
        ep_alias.blur_frame_bytes = 0;
        fstride = 0;
    }
    ep_alias.host_out = mapped_out ? 1 : 0;
    const ExtractParams& ep = ep_alias;
    const LevelDesc* dl = g.d_lv.as<LevelDesc>();
    // the host-buffer paths report their own per-call word; the device batch path leaves word 0 sticky
    // until orbx_check_error takes (and clears) it, so no fill kernel sits on the batch stream every call
    int* errp = h->err.as<int>() + (host_call ? kErrWordExtract : kErrWordSticky);
    if (nframes < kPyrFramesMinBatch && !h->serial && !h->prof_on && !h->alias) {
        if (run_extract_levels(h, ep, nframes, d_frames, fstride, pitch, d_kps, d_desc, d_counts, kp_stride, st, errp,
                               host_call ? nullptr : h->user_ev_pyr, host_call ? nullptr : h->user_ev_fast, copy))
            return ORBX_EDEVICE;
        note_last(h, d_frames, fstride, pitch, nframes, st);
        return 0;
    }
    const bool fused = describe_blur_ok(d_frames, fstride, pitch);
    if (!fused && ensure_blur(h)) return ORBX_EDEVICE;
    if (!fused && !h->serial && ensure_stream(h, &h->side)) return ORBX_EDEVICE;
    const hipStream_t sd = h->serial ? st : h->side;
    if (prof_mark(h, 0, 0, st)) return ORBX_EDEVICE;
    if (!(h->skip_mask & 1) && launch_pyramid(h, ep, d_frames, fstride, pitch, nframes, st)) return ORBX_EDEVICE;
    if (prof_mark(h, 0, 1, st)) return ORBX_EDEVICE;
    if (!host_call && h->user_ev_pyr) HIPR(hipEventRecord(h->user_ev_pyr, st));
    if (!fused) {
        if (!h->serial) {
            HIPR(hipEventRecord(h->ev_pyr, st));
            HIPR(hipStreamWaitEvent(sd, h->ev_pyr, 0));
        }
        if (prof_mark(h, 3, 0, sd)) return ORBX_EDEVICE;
        if (!(h->skip_mask & 8))
            HIPR(launch_blur_strips(d_frames, fstride, pitch, h->pyr.as<uint8_t>(), h->blur.as<uint8_t>(), ep, dl, 0,
                                    g.nbjobs, nullptr, nframes, sd));
        if (prof_mark(h, 3, 1, sd)) return ORBX_EDEVICE;
        if (!h->serial) HIPR(hipEventRecord(h->ev_blur, sd));
    } else if (prof_mark(h, 3, 0, st) || prof_mark(h, 3, 1, st)) {  // no blur stage: a zero-length pair
        return ORBX_EDEVICE;
    }
    if (prof_mark(h, 1, 0, st)) return ORBX_EDEVICE;
    if (!(h->skip_mask & 2) && launch_fast(h, ep, d_frames, fstride, pitch, 0, ep.ncells, nframes, st)) return ORBX_EDEVICE;
    if (!host_call && h->user_ev_fast) HIPR(hipEventRecord(h->user_ev_fast, st));
    if (prof_mark(h, 1, 1, st) || prof_mark(h, 2, 0, st)) return ORBX_EDEVICE;
    if (!(h->skip_mask & 4)) {
        const int split = g.oct_split;  // 0: one launch over every level
        if (launch_octree_levels(h, ep, 0, split ? split : -1, g.NC, g.KL, g.lds_bytes, errp, nframes, st) ||
            (split && launch_octree_levels(h, ep, split, ep.L - split, g.NC_lo, g.KL_lo, g.lds_lo, errp, nframes, st)))
            return ORBX_EDEVICE;
    }
    if (prof_mark(h, 2, 1, st)) return ORBX_EDEVICE;
    if (!h->serial && !fused) HIPR(hipStreamWaitEvent(st, h->ev_blur, 0));
    if (prof_mark(h, 4, 0, st)) return ORBX_EDEVICE;
    if (!(h->skip_mask & 16) &&
        launch_describe_any(h, ep, fused, d_frames, fstride, pitch, d_kps, d_desc, d_counts, kp_stride, nframes, st))
        return ORBX_EDEVICE;
    if (prof_mark(h, 4, 1, st)) return ORBX_EDEVICE;
    if (h->prof_on && h->prof_calls < kProfMaxCalls) h->prof_calls++;
    note_last(h, d_frames, fstride, pitch, nframes, st);
    return 0;
}

extern "C" {

const char* orbx_version(void) { return "orbslam-mi355x 0.1 (gfx950)"; }

int orbx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int orbx_create(const orbx_params* p, int device, int max_width, int max_height, int max_batch,
                orbx_handle** out) {
    if (!p || !out || p->nlevels < 1 || p->nlevels > kMaxLevels || p->nfeatures < 1 || p->scale_factor <= 1.0f ||
        max_width <= 0 || max_height <= 0 || max_batch < 1)
        return ORBX_EARG;
    *out = nullptr;
    int ndev = orbx_device_count();
    if (device < 0 || device >= ndev) return ORBX_EDEVICE;
    HIPR(hipSetDevice(device));
    orbx_handle* h = new orbx_handle();
    h->params = *p;
    h->T.build(*p);
    h->device = device;
    h->max_w = max_width;
    h->max_h = max_height;
    h->max_batch = max_batch;
    // no HIP stream here: the host-call stream and the blur's side stream are created at their first use
    // (ensure_stream), since every idle stream in the process costs the batch schedule's graph streams their step
    // rate (profiles/r04_idle_stream_cost.log) and a device batch on the caller's stream needs neither
    if (hipEventCreateWithFlags(&h->ev_pyr, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_blur, hipEventDisableTiming) != hipSuccess) {
        orbx_destroy(h);
        return ORBX_EDEVICE;
    }
    int rc = ensure_geometry(h, max_width, max_height, 1);
    if (rc) {
        orbx_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

void orbx_destroy(orbx_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->side) (void)hipStreamSynchronize(h->side);
    for (DevBuf* b : {&h->pyr, &h->blur, &h->cellkey, &h->cellcnt, &h->lvkey, &h->lvcnt, &h->gscratch, &h->err,
                      &h->in_frame, &h->out_kps, &h->out_desc, &h->out_cnt, &h->st_buf, &h->stereo_sad})
        b->release();
    h->geo.release();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->side) (void)hipStreamDestroy(h->side);
    for (hipEvent_t e : {h->ev_pyr, h->ev_blur})
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
    if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
    if (h->graph) (void)hipGraphDestroy(h->graph);
    if (h->pin_in) (void)hipHostFree(h->pin_in);
    if (h->pin_out) (void)hipHostFree(h->pin_out);
    if (h->pin_pyr) (void)hipHostFree(h->pin_pyr);
    delete h;
}

int orbx_check_error(orbx_handle* h, void* stream) {
    if (!h) return ORBX_EARG;
    HIPR(hipSetDevice(h->device));
    // read and clear in one device atomic (a batch on another stream that raises the flag afterwards
    // leaves it set for the next check)
    int flag = 0;
    int* w = h->err.as<int>();
    HIPR(launch_flag_take(w + kErrWordSticky, w + kErrWordTake, (hipStream_t)stream));
    HIPR(hipMemcpyAsync(&flag, w + kErrWordTake, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPR(hipStreamSynchronize((hipStream_t)stream));
    return flag ? ORBX_EDEVICE : 0;
}

int orbx_selftest_sincosf(const float* d_in, float* d_sin, float* d_cos, int n, void* stream) {
    if (!d_in || !d_sin || !d_cos || n < 0) return ORBX_EARG;
    if (n == 0) return 0;
    HIPR(launch_sincos_selftest(d_in, d_sin, d_cos, n, (hipStream_t)stream));
    return 0;
}

int orbx_set_pyramid_event(orbx_handle* h, void* event) { return orbx_set_stage_event(h, 0, event); }

int orbx_set_stage_event(orbx_handle* h, int stage, void* event) {
    if (!h || stage < 0 || stage > 1) return ORBX_EARG;
    (stage == 0 ? h->user_ev_pyr : h->user_ev_fast) = (hipEvent_t)event;
    return 0;
}

int orbx_describe_blur_fused(const void* frames, size_t frame_stride, size_t pitch) {
    return describe_blur_ok((const uint8_t*)frames, (long long)frame_stride, (int)pitch) ? 1 : 0;
}

int orbx_debug_hip_failure(void) {
    // two events that were never recorded: hipEventElapsedTime fails (invalid resource handle), as an unrecorded
    // stage pair did in round 5's orbx_profile_read
    hipEvent_t a = nullptr, b = nullptr;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
        if (a) (void)hipEventDestroy(a);
        (void)hipGetLastError();
        return ORBX_EDEVICE;
    }
    float t = 0;
    const hipError_t e = hipEventElapsedTime(&t, a, b);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    HIPR(e);
    return 0;
}

int orbx_debug_skip_stages(orbx_handle* h, int mask) {
    if (!h || mask < 0 || mask > 0x1F) return ORBX_EARG;
    h->skip_mask = mask;
    h->epoch++;  // a captured host-call graph holds the schedule it was captured with
    return 0;
}

int orbx_debug_serial(orbx_handle* h, int on) {
    if (!h) return ORBX_EARG;
    h->serial = on != 0;
    h->epoch++;
    return 0;
}

int orbx_debug_alias_frames(orbx_handle* h, int on) {
    if (!h) return ORBX_EARG;
    h->alias = on != 0;
    h->epoch++;
    return 0;
}

int orbx_debug_raise_error(orbx_handle* h, int flag, void* stream) {
    if (!h || flag <= 0) return ORBX_EARG;
    HIPR(hipSetDevice(h->device));
    int cur = 0;
    hipStream_t st = (hipStream_t)stream;
    HIPR(hipMemcpyAsync(&cur, h->err.as<int>() + kErrWordSticky, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPR(hipStreamSynchronize(st));
    cur |= flag;
    HIPR(hipMemcpyAsync(h->err.as<int>() + kErrWordSticky, &cur, sizeof(int), hipMemcpyHostToDevice, st));
    HIPR(hipStreamSynchronize(st));
    return 0;
}

int orbx_profile_enable(orbx_handle* h, int on) {
    if (!h) return ORBX_EARG;
    h->prof_on = on != 0;
    h->prof_mask = on & 0x1F;
    h->prof_calls = 0;
    for (double& v : h->prof_ms) v = 0;
    return 0;
}

int orbx_profile_read(orbx_handle* h, double* ms, int* ncalls) {
    if (!h) return ORBX_EARG;
    HIPR(hipSetDevice(h->device));
    double acc[5] = {0, 0, 0, 0, 0};
    for (int c = 0; c < h->prof_calls; c++) {
        for (int k = 0; k < 5; k++) {
            const size_t e0 = (size_t)c * 10 + 2 * k;
            if (!((h->prof_mask >> k) & 1)) continue;
            HIPR(hipEventSynchronize(h->prof_ev[e0 + 1]));
            float t = 0;
            HIPR(hipEventElapsedTime(&t, h->prof_ev[e0], h->prof_ev[e0 + 1]));
            acc[k] += t;
        }
    }
    if (ms) for (int k = 0; k < 5; k++) ms[k] = acc[k];
    if (ncalls) *ncalls = h->prof_calls;
    return 0;
}

int orbx_max_keypoints(const orbx_handle* h, int width, int height) {
    if (!h) return ORBX_EARG;
    if (h->geo.W == width && h->geo.H == height) return h->geo.ep.kp_per_frame;
    // host-only computation of the cap (no upload): replicate build's kp accounting
    int total = 0;
    for (int l = 0; l < h->T.nlevels; l++) {
        const int w = cv_round_f((float)width * h->T.inv_scale[l]);
        const int hh = cv_round_f((float)height * h->T.inv_scale[l]);
        if (w - 32 <= 0 || hh - 32 <= 0) return ORBX_EARG;  // as Geometry::build rejects the level
        const int nIni = (int)roundf((float)(w - 32) / (hh - 32));
        total += std::max(h->T.nfeat[l] + 3, 4 * std::max(nIni, 1));
    }
    return total;
}

int orbx_extract_batch_device(orbx_handle* h, int nframes, const uint8_t* d_frames, size_t frame_stride, int width,
                              int height, size_t pitch, orbx_kp* d_kps, uint8_t* d_desc, int32_t* d_counts,
                              int kp_stride, void* stream) {
    if (!h || !d_frames || !d_kps || !d_desc || !d_counts || width <= 0 || height <= 0 || pitch < (size_t)width)
        return ORBX_EARG;
    HIPR(hipSetDevice(h->device));
    int rc = ensure_geometry(h, width, height, nframes);
    if (rc) return rc;
    if (kp_stride < h->geo.ep.kp_per_frame) return ORBX_ECAPACITY;
    return run_extract(h, nframes, d_frames, (long long)frame_stride, (int)pitch, d_kps, d_desc, d_counts, kp_stride,
                       (hipStream_t)stream, false);
}

/* The captured host path: pinned H2D -> run_extract -> one pinned D2H of {count, error flag, K
 * keypoints, K descriptors}, as one hipGraph per geometry (replayed: no per-kernel launch cost on
 * the calling thread, one synchronisation per frame). The first call at a new geometry/buffer epoch
 * runs eagerly (it also performs one-time setup such as LDS attributes), the next one captures. */
static int extract_graph(orbx_handle* h, const uint8_t* img, int width, int height, size_t pitch, orbx_kp* kps,
                         uint8_t* desc, int cap, int* n) {
    const int K = h->geo.ep.kp_per_frame;
    const size_t in_bytes = (size_t)width * height;
    const bool un = h->cam_on;  // orbx_set_camera: one more node, mvKeysUn behind the descriptors
    const size_t un_off = 64 + (sizeof(orbx_kp) + 32) * (size_t)K;
    const size_t out_bytes = un_off + (un ? sizeof(orbx_kp) * (size_t)K : 0);
    if (h->pin_in_bytes < in_bytes) {
        if (h->pin_in) (void)hipHostFree(h->pin_in);
        h->pin_in = nullptr;
        h->pin_in_bytes = 0;
        HIPR(hipHostMalloc((void**)&h->pin_in, in_bytes, hipHostMallocDefault));
        h->pin_in_bytes = in_bytes;
        h->epoch++;
    }
    if (h->pin_out_bytes < out_bytes) {
        if (h->pin_out) (void)hipHostFree(h->pin_out);
        h->pin_out = nullptr;
        h->pin_out_bytes = 0;
        // fine-grained (coherent) like the matchers' polled buffers: the kernels' writes of the results and of the
        // done word are visible to the polling host without relying on an L2 writeback
        HIPR(hipHostMalloc((void**)&h->pin_out, out_bytes, hipHostMallocMapped | hipHostMallocCoherent));
        memset(h->pin_out, 0, out_bytes);  // done word 0: the device counter's first value is 1
        h->pin_out_bytes = out_bytes;
        HIPR(hipHostGetDevicePointer((void**)&h->pin_out_dev, h->pin_out, 0));
        h->epoch++;
    }
    // mvImagePyramid for the host (orbx_set_host_pyramid): extra workgroups of the octree launch copy levels 1..L-1
    // of this frame into mapped pinned memory while the octree runs; level 0 is pin_in itself
    const bool copies = h->host_pyr && !h->serial && !h->alias && h->geo.ep.L > 1;
    HostCopy hc{nullptr, nullptr, 0, 0};
    if (copies) {
        const size_t pb = (size_t)h->geo.ep.pyr_frame_bytes;
        if (h->pin_pyr_bytes < pb) {
            if (h->pin_pyr) (void)hipHostFree(h->pin_pyr);
            h->pin_pyr = h->pin_pyr_dev = nullptr;
            h->pin_pyr_bytes = 0;
            HIPR(hipHostMalloc((void**)&h->pin_pyr, pb, hipHostMallocMapped | hipHostMallocCoherent));
            h->pin_pyr_bytes = pb;
            HIPR(hipHostGetDevicePointer((void**)&h->pin_pyr_dev, h->pin_pyr, 0));
            h->epoch++;
        }
        hc = HostCopy{(const uint4*)h->pyr.p, nullptr, (long long)(pb / 16), kHostCopyBlocks,
                      (uint4* const*)(h->pin_out_dev + kPinOutCopyDst)};
        if (h->target && h->target_bytes < host_l0_bytes(h) + pb) return ORBX_EARG;
        // this call's destination of levels 1..L-1, read by the copy workgroups when they run
        uint8_t* dst = h->target ? h->target_dev + host_l0_bytes(h) : h->pin_pyr_dev;
        memcpy(h->pin_out + kPinOutCopyDst, &dst, sizeof(dst));
    }
    for (int y = 0; y < height; y++) memcpy(h->pin_in + (size_t)y * width, img + (size_t)y * pitch, width);
    uint8_t* o_kps = h->pin_out + 64;
    uint8_t* o_desc = o_kps + sizeof(orbx_kp) * (size_t)K;
    // describe writes the count, keypoints and descriptors straight into the pinned buffer (its device-mapped
    // address: 56 B per keypoint over PCIe inside the kernel, no D2H copies), and the last launch moves the
    // call's error word there and clears it for the next call
    uint8_t* d_out = h->pin_out_dev;
    auto enqueue = [&]() -> int {
        HIPR(hipMemcpyAsync(h->in_frame.p, h->pin_in, in_bytes, hipMemcpyHostToDevice, h->stream));
        // with a camera describe leaves keypoints and count in HBM and the undistort node delivers them, raw and
        // undistorted, so no kernel reads across PCIe
        int rc = run_extract(h, 1, h->in_frame.as<uint8_t>(), (long long)in_bytes, width,
                             un ? h->out_kps.as<orbx_kp>() : (orbx_kp*)(d_out + 64),
                             d_out + 64 + sizeof(orbx_kp) * (size_t)K, un ? h->out_cnt.as<int32_t>() : (int32_t*)d_out,
                             K, h->stream, true, true, copies ? &hc : nullptr);
        if (rc) return rc;
        if (un)
            HIPR(launch_undistort_deliver(h->cam, h->out_kps.as<orbx_kp>(), h->out_cnt.as<int32_t>(), K,
                                          (orbx_kp*)(d_out + 64), (orbx_kp*)(d_out + un_off), (int32_t*)d_out,
                                          h->stream));
        HIPR(launch_call_done(h->err.as<int32_t>() + kErrWordExtract, (int32_t*)(d_out + 4),
                              h->err.as<int32_t>() + kErrWordExtractSeq, (int32_t*)(d_out + 8), h->stream));
        return 0;
    };
    // the done word before this call's launch (the previous call's value): the call is over when it changes
    const int32_t* done = (const int32_t*)(h->pin_out + 8);
    const int32_t done0 = __atomic_load_n(done, __ATOMIC_ACQUIRE);
    const bool valid = h->gexec && h->graph_w == width && h->graph_h == height && h->graph_epoch == h->epoch;
    if (!valid) {
        if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
        if (h->graph) (void)hipGraphDestroy(h->graph);
        h->gexec = nullptr;
        h->graph = nullptr;
        if (h->graph_epoch != h->epoch || h->graph_w != width || h->graph_h != height) h->graph_warm = 0;
        h->graph_w = width;
        h->graph_h = height;
        h->graph_epoch = h->epoch;
    }
    if (!h->gexec && h->graph_warm == 0) {
        // first frame at this epoch: eager
        int rc = enqueue();
        if (rc) return rc;
        h->graph_warm = 1;
    } else {
        if (!h->gexec) {
            HIPR(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
            int rc = enqueue();
            hipGraph_t g = nullptr;
            const hipError_t ce = hipStreamEndCapture(h->stream, &g);
            if (rc) {
                if (g) (void)hipGraphDestroy(g);
                return rc;
            }
            HIPR(ce);
            h->graph = g;
            HIPR(hipGraphInstantiate(&h->gexec, h->graph, nullptr, nullptr, 0));
        }
        HIPR(hipGraphLaunch(h->gexec, h->stream));
    }
    // level 0 of a caller-owned target: the staged input, copied on the host while the device works
    if (copies && h->target) memcpy(h->target, h->pin_in, in_bytes);
    if (const int rc = wait_until(h->stream, [&] { return __atomic_load_n(done, __ATOMIC_ACQUIRE) != done0; })) return rc;
    // the copy workgroups ride on the octree launch: a skipped octree (orbx_debug_skip_stages bit 2) delivers nothing
    h->host_pyr_valid = copies && !(h->skip_mask & 4);
    h->last_target = copies ? h->target : nullptr;
    note_last(h, h->in_frame.as<uint8_t>(), (long long)in_bytes, width, 1, h->stream);
    int cnt = 0, errflag = 0;
    memcpy(&cnt, h->pin_out, sizeof(int));
    memcpy(&errflag, h->pin_out + 4, sizeof(int));
    if (errflag) return ORBX_EDEVICE;
    if (cnt > cap) return ORBX_ECAPACITY;
    if (cnt > 0) {
        if (kps) memcpy(kps, o_kps, sizeof(orbx_kp) * (size_t)cnt);
        if (desc) memcpy(desc, o_desc, 32 * (size_t)cnt);
    }
    *n = cnt;
    h->un_valid = un && !(h->skip_mask & 16) && cnt <= K;
    h->un_count = cnt;
    h->un_off = un_off;
    return 0;
}

int orbx_extract(orbx_handle* h, const uint8_t* img, int width, int height, size_t pitch, orbx_kp* kps,
                 uint8_t* desc, int cap, int* n) {
    if (!h || !n) return ORBX_EARG;
    *n = 0;
    if (width <= 0 || height <= 0 || !img) return 0;  // empty image: outputs untouched (:1046-1047)
    if (pitch < (size_t)width) return ORBX_EARG;
    HIPR(hipSetDevice(h->device));
    h->host_pyr_valid = false;
    h->un_valid = false;
    if (ensure_stream(h, &h->stream)) return ORBX_EDEVICE;
    int rc = ensure_geometry(h, width, height, 1);
    if (rc) return rc;
    const int K = h->geo.ep.kp_per_frame;
    const void* before[4] = {h->in_frame.p, h->out_kps.p, h->out_desc.p, h->out_cnt.p};
    if (h->in_frame.ensure((size_t)width * height) || h->out_kps.ensure(sizeof(orbx_kp) * K) ||
        h->out_desc.ensure(32 * (size_t)K) || h->out_cnt.ensure(64))
        return ORBX_EDEVICE;
    const void* after[4] = {h->in_frame.p, h->out_kps.p, h->out_desc.p, h->out_cnt.p};
    if (memcmp(before, after, sizeof(before))) h->epoch++;
    // an unaligned frame (width not a multiple of 4) blurs into HBM: allocate that buffer here, never inside a capture
    if (!describe_blur_ok(h->in_frame.as<uint8_t>(), (long long)width * height, width) && ensure_blur(h))
        return ORBX_EDEVICE;
    // captured graph, except while stage profiling (its events are recorded per call)
    if (!h->prof_on) return extract_graph(h, img, width, height, pitch, kps, desc, cap, n);
    HIPR(hipMemcpy2DAsync(h->in_frame.p, width, img, pitch, width, height, hipMemcpyHostToDevice, h->stream));
    rc = run_extract(h, 1, h->in_frame.as<uint8_t>(), (long long)width * height, width, h->out_kps.as<orbx_kp>(),
                     h->out_desc.as<uint8_t>(), h->out_cnt.as<int32_t>(), K, h->stream);
    if (rc) return rc;
    int cnt = 0, errflag = 0;
    HIPR(hipMemcpyAsync(&cnt, h->out_cnt.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPR(launch_flag_take(h->err.as<int32_t>() + kErrWordExtract, h->err.as<int32_t>() + kErrWordExtractTake, h->stream));
    HIPR(hipMemcpyAsync(&errflag, h->err.as<int>() + kErrWordExtractTake, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPR(hipStreamSynchronize(h->stream));
    if (errflag) return ORBX_EDEVICE;
    if (cnt > cap) return ORBX_ECAPACITY;
    if (cnt > 0) {
        if (kps) HIPR(hipMemcpyAsync(kps, h->out_kps.p, sizeof(orbx_kp) * cnt, hipMemcpyDeviceToHost, h->stream));
        if (desc) HIPR(hipMemcpyAsync(desc, h->out_desc.p, 32 * (size_t)cnt, hipMemcpyDeviceToHost, h->stream));
        HIPR(hipStreamSynchronize(h->stream));
    }
    *n = cnt;
    return 0;
}

int orbx_set_camera(orbx_handle* h, const orbx_camera* cam) {
    if (!h || (cam && (cam->fx == 0 || cam->fy == 0))) return ORBX_EARG;
    h->cam_on = cam != nullptr;
    if (cam) h->cam = *cam;
    h->un_valid = false;
    h->epoch++;  // the captured host-call graph holds the camera and whether it undistorts
    return 0;
}

int orbx_last_keypoints_un(orbx_handle* h, orbx_kp* kps_un, int cap, int* n) {
    if (!h || !n || cap < 0 || !h->un_valid) return ORBX_EARG;
    *n = 0;
    if (h->un_count > cap) return ORBX_ECAPACITY;
    if (h->un_count > 0) {
        if (!kps_un) return ORBX_EARG;
        memcpy(kps_un, h->pin_out + h->un_off, sizeof(orbx_kp) * (size_t)h->un_count);
    }
    *n = h->un_count;
    return 0;
}

int orbx_pyramid_level(orbx_handle* h, int frame, int level, uint8_t* dst, size_t pitch, int* width, int* height) {
    if (!h || level < 0 || level >= h->T.nlevels || !h->geo.W) return ORBX_EARG;
    const LevelDesc& d = h->geo.lv[level];
    if (width) *width = d.w;
    if (height) *height = d.h;
    if (!dst) return 0;
    if (!h->last_frames || frame < 0 || frame >= h->last_nframes || pitch < (size_t)d.w) return ORBX_EARG;
    HIPR(hipSetDevice(h->device));
    // wait for this handle's own last extraction only (the stream it was enqueued on and the handle's side
    // stream), not for every stream on the device (other extractor / matcher threads)
    HIPR(hipStreamSynchronize(h->last_stream));
    if (h->side) HIPR(hipStreamSynchronize(h->side));
    const uint8_t* src = level == 0 ? h->last_frames + frame * h->last_fstride
                                    : h->pyr.as<uint8_t>() + frame * h->geo.ep.pyr_frame_bytes + d.pyr_off;
    const size_t sp = level == 0 ? (size_t)h->last_pitch : (size_t)d.pitch;
    HIPR(hipMemcpy2D(dst, pitch, src, sp, d.w, d.h, hipMemcpyDeviceToHost));
    return 0;
}

int orbx_set_host_pyramid(orbx_handle* h, int on) {
    if (!h) return ORBX_EARG;
    h->host_pyr = on != 0;
    h->host_pyr_valid = false;
    h->epoch++;  // the captured host-call graph holds whether the octree launch carries the copy
    return 0;
}

int orbx_host_pyramid_level(orbx_handle* h, int level, const uint8_t** data, size_t* pitch, int* width, int* height) {
    if (!h || !data || !pitch || level < 0 || level >= h->T.nlevels || !h->geo.W || !h->host_pyr_valid)
        return ORBX_EARG;
    const LevelDesc& d = h->geo.lv[level];
    if (h->last_target)
        *data = level == 0 ? h->last_target : h->last_target + host_l0_bytes(h) + d.pyr_off;
    else
        *data = level == 0 ? h->pin_in : h->pin_pyr + d.pyr_off;
    *pitch = level == 0 ? (size_t)d.w : (size_t)d.pitch;
    if (width) *width = d.w;
    if (height) *height = d.h;
    return 0;
}

int orbx_host_pyramid_bytes(orbx_handle* h, int width, int height, size_t* bytes) {
    if (!h || !bytes || width <= 0 || height <= 0) return ORBX_EARG;
    *bytes = 0;
    HIPR(hipSetDevice(h->device));
    if (const int rc = ensure_geometry(h, width, height, 1)) return rc;
    *bytes = host_l0_bytes(h) + (size_t)h->geo.ep.pyr_frame_bytes;
    return 0;
}

int orbx_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return ORBX_EARG;
    HIPR(hipHostRegister(p, bytes, hipHostRegisterMapped));
    return 0;
}

int orbx_host_unregister(void* p) {
    if (!p) return ORBX_EARG;
    HIPR(hipHostUnregister(p));
    return 0;
}

int orbx_set_host_pyramid_target(orbx_handle* h, uint8_t* host, size_t bytes) {
    if (!h || (host && !bytes)) return ORBX_EARG;
    if (!host) {
        h->target = h->target_dev = nullptr;
        h->target_bytes = 0;
        return 0;
    }
    if (host == h->target && bytes == h->target_bytes) return 0;  // the drop-in sets the same buffer every call
    HIPR(hipSetDevice(h->device));
    uint8_t* dev = nullptr;
    HIPR(hipHostGetDevicePointer((void**)&dev, host, 0));  // fails unless the memory is registered (or pinned) mapped
    h->target = host;
    h->target_dev = dev;
    h->target_bytes = bytes;
    return 0;
}

int orbx_get_levels(const orbx_handle* h) { return h ? h->T.nlevels : ORBX_EARG; }
float orbx_get_scale_factor(const orbx_handle* h) { return h ? (float)h->T.scaleFactor : 0.f; }

int orbx_get_scale_tables(const orbx_handle* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2) {
    if (!h) return ORBX_EARG;
    for (int l = 0; l < h->T.nlevels; l++) {
        if (scale) scale[l] = h->T.scale[l];
        if (inv_scale) inv_scale[l] = h->T.inv_scale[l];
        if (sigma2) sigma2[l] = h->T.sigma2[l];
        if (inv_sigma2) inv_sigma2[l] = h->T.inv_sigma2[l];
    }
    return 0;
}

int orbx_compute_scale_tables(const orbx_params* p, float* scale, float* inv_scale, float* sigma2,
                              float* inv_sigma2) {
    if (!p || p->nlevels < 1 || p->nlevels > kMaxLevels || p->nfeatures < 1 || p->scale_factor <= 1.0f)
        return ORBX_EARG;
    Tables T;
    T.build(*p);
    for (int l = 0; l < T.nlevels; l++) {
        if (scale) scale[l] = T.scale[l];
        if (inv_scale) inv_scale[l] = T.inv_scale[l];
        if (sigma2) sigma2[l] = T.sigma2[l];
        if (inv_sigma2) inv_sigma2[l] = T.inv_sigma2[l];
    }
    return 0;
}

int orbx_get_feature_split(const orbx_handle* h, int32_t* per_level, int32_t* umax16) {
    if (!h) return ORBX_EARG;
    for (int l = 0; l < h->T.nlevels; l++)
        if (per_level) per_level[l] = h->T.nfeat[l];
    for (int v = 0; v < 16; v++)
        if (umax16) umax16[v] = h->T.umax[v];
    return 0;
}

}  // extern "C"
