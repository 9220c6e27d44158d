/* matcher.cpp -- ORBmatcher's SearchByBoW and SearchForTriangulation behind orbm_*: the per-call forms (view staging,
 * the small-call kernels), the *_batch_device entries, and the keyframe cache with the *_cached matchers. */
#include "matcher_host.h"

using namespace orbamd;

namespace {

int wait_call(hipStream_t st, const int32_t* word) {
    return wait_until(st, [word] { return __atomic_load_n(word, __ATOMIC_ACQUIRE) >= 0; });
}

void make_geom(MatchGeom& g, const float F12[9], float ex, float ey, int nlevels, const float* scale,
               const float* sigma2) {
    for (int i = 0; i < 9; i++) g.F[i] = F12[i];
    g.ex = ex;
    g.ey = ey;
    for (int o = 0; o < 16; o++) {
        g.th100[o] = o < nlevels ? 100 * scale[o] : 0.f;
        g.th384[o] = o < nlevels ? 3.84 * (double)sigma2[o] : 0.0;
        // the smallest float >= th384: (double)d < th384 <=> d < th384f for every float d
        float t = (float)g.th384[o];
        if ((double)t < g.th384[o]) t = std::nextafter(t, INFINITY);
        g.th384f[o] = t;
    }
}

/* merge-walk of two FeatureVectors (DBoW2 std::map iteration with lower_bound jumps,
 * ORBmatcher.cc:691-789): returns the common (node index 1, node index 2) pairs */
void common_nodes(const orbm_kf_view* a, const orbm_kf_view* b, std::vector<std::pair<int, int>>& out) {
    out.clear();
    int i = 0, j = 0;
    while (i < a->n_nodes && j < b->n_nodes) {
        if (a->node_id[i] == b->node_id[j]) {
            out.emplace_back(i, j);
            i++;
            j++;
        } else if (a->node_id[i] < b->node_id[j]) {
            i = (int)(std::lower_bound(a->node_id + i, a->node_id + a->n_nodes, b->node_id[j]) - a->node_id);
        } else {
            j = (int)(std::lower_bound(b->node_id + j, b->node_id + b->n_nodes, a->node_id[i]) - b->node_id);
        }
    }
}

bool view_ok(const orbm_kf_view* v) {
    return v && v->n >= 0 && (v->n == 0 || (v->desc && v->x && v->y && v->angle && v->octave)) && v->n_nodes >= 0 &&
           (v->n_nodes == 0 || (v->node_id && v->node_off && v->node_feat)) && v->nlevels > 0 && v->nlevels <= 16 &&
           v->scale_factors && v->level_sigma2;
}

struct ViewPlan {
    size_t desc, x, y, angle, octave, uright, has_mp, mp_bad, feat;
    int nfeat;
};
/* geom = false (SearchByBoW): positions, octaves and mvuRight are not uploaded (the BoW matchers read
 * descriptors, MapPoint flags, angles and the node lists only) */
void plan_view(Carve& c, const orbm_kf_view* v, ViewPlan& p, bool geom = true, const KfEntry* ce = nullptr) {
    const size_t n = (size_t)std::max(v->n, 1);
    const size_t none = (size_t)-1;
    p.nfeat = v->n_nodes ? v->node_off[v->n_nodes] : 0;
    if (ce) {  // cached keyframe: only the MapPoint flags (they change between calls) are staged
        p.desc = p.x = p.y = p.angle = p.octave = p.uright = p.feat = none;
        p.has_mp = v->has_mp ? c.take(n) : none;
        p.mp_bad = v->mp_bad ? c.take(n) : none;
        return;
    }
    p.desc = c.take(32 * n);
    p.x = geom ? c.take(4 * n) : none;
    p.y = geom ? c.take(4 * n) : none;
    p.angle = c.take(4 * n);
    p.octave = geom ? c.take(4 * n) : none;
    p.uright = geom && v->uright ? c.take(4 * n) : none;
    p.has_mp = v->has_mp ? c.take(n) : (size_t)-1;
    p.mp_bad = v->mp_bad ? c.take(n) : (size_t)-1;
    p.feat = c.take(4 * (size_t)std::max(p.nfeat, 1));
}

/* stage one view into the pinned host image of the scratch (offsets from plan_view) and return
 * the device view of the same offsets: a call then uploads all its inputs with ONE H2D copy */
DevView stage_view(uint8_t* hbase, uint8_t* dbase, const orbm_kf_view* v, const ViewPlan& p,
                   const KfEntry* ce = nullptr) {
    DevView d;
    const size_t n = (size_t)v->n;
    d.n = v->n;
    if (ce) {
        d.desc = ce->at(ce->o_desc);
        d.x = (const float*)ce->at(ce->o_x);
        d.y = (const float*)ce->at(ce->o_y);
        d.angle = (const float*)ce->at(ce->o_ang);
        d.octave = (const int32_t*)ce->at(ce->o_oct);
        d.uright = v->uright && ce->has_ur ? (const float*)ce->at(ce->o_ur) : nullptr;
        d.node_feat = (const int32_t*)ce->at(ce->o_feat);
        d.has_mp = v->has_mp ? dbase + p.has_mp : nullptr;
        d.mp_bad = v->mp_bad ? dbase + p.mp_bad : nullptr;
        if (n && v->has_mp) memcpy(hbase + p.has_mp, v->has_mp, n);
        if (n && v->mp_bad) memcpy(hbase + p.mp_bad, v->mp_bad, n);
        return d;
    }
    d.desc = dbase + p.desc;
    const size_t none = (size_t)-1;
    d.x = p.x != none ? (const float*)(dbase + p.x) : nullptr;
    d.y = p.y != none ? (const float*)(dbase + p.y) : nullptr;
    d.angle = (const float*)(dbase + p.angle);
    d.octave = p.octave != none ? (const int32_t*)(dbase + p.octave) : nullptr;
    d.uright = p.uright != none ? (const float*)(dbase + p.uright) : nullptr;
    d.has_mp = v->has_mp ? dbase + p.has_mp : nullptr;
    d.mp_bad = v->mp_bad ? dbase + p.mp_bad : nullptr;
    d.node_feat = (const int32_t*)(dbase + p.feat);
    if (n) {
        memcpy(hbase + p.desc, v->desc, 32 * n);
        if (p.x != none) memcpy(hbase + p.x, v->x, 4 * n);
        if (p.y != none) memcpy(hbase + p.y, v->y, 4 * n);
        memcpy(hbase + p.angle, v->angle, 4 * n);
        if (p.octave != none) memcpy(hbase + p.octave, v->octave, 4 * n);
        if (p.uright != none) memcpy(hbase + p.uright, v->uright, 4 * n);
        if (v->has_mp) memcpy(hbase + p.has_mp, v->has_mp, n);
        if (v->mp_bad) memcpy(hbase + p.mp_bad, v->mp_bad, n);
    }
    if (p.nfeat) memcpy(hbase + p.feat, v->node_feat, 4 * (size_t)p.nfeat);
    return d;
}

}  // namespace

extern "C" {

int orbm_create(int device, orbm_ctx** out) {
    if (!out) return ORBX_EARG;
    *out = nullptr;
    if (device < 0 || device >= orbx_device_count()) return ORBX_EDEVICE;
    HIPR(hipSetDevice(device));
    orbm_ctx* c = new orbm_ctx();
    c->device = device;
    if (c->err.ensure(256) || hipMemset(c->err.p, 0, 256) != hipSuccess) {
        orbm_destroy(c);
        return ORBX_EDEVICE;
    }
    *out = c;
    return 0;
}

void orbm_destroy(orbm_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->scratch.release();
    c->tri_scratch.release();
    c->tri_stats.release();
    c->err.release();
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

/* measurement hooks of the BF triangulation batch calls (orbslam_amd_testing.h) */
int orbm_debug_tri_cull(orbm_ctx* ctx, int mode) {
    if (!ctx || mode < 0 || mode > 2) return ORBX_EARG;
    HIPR(hipSetDevice(ctx->device));
    if (mode == 2) {
        if (ctx->tri_stats.ensure(2 * sizeof(unsigned long long))) return ORBX_EDEVICE;
        HIPR(hipDeviceSynchronize());
        HIPR(hipMemset(ctx->tri_stats.p, 0, 2 * sizeof(unsigned long long)));
    }
    ctx->tri_cull = mode;
    return 0;
}

int orbm_debug_tri_cull_counts(orbm_ctx* ctx, unsigned long long out[2]) {
    if (!ctx || !out) return ORBX_EARG;
    out[0] = out[1] = 0;
    if (!ctx->tri_stats.p) return 0;
    HIPR(hipSetDevice(ctx->device));
    HIPR(hipDeviceSynchronize());
    HIPR(hipMemcpy(out, ctx->tri_stats.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPR(hipMemset(ctx->tri_stats.p, 0, 2 * sizeof(unsigned long long)));
    return 0;
}

/* ORBmatcher::DescriptorDistance (ORBmatcher.cc:1647-1663) -- host scalar */
int orbm_descriptor_distance(const uint8_t* a, const uint8_t* b) {
    if (!a || !b) return ORBX_EARG;
    int d = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t x, y;
        memcpy(&x, a + 4 * i, 4);
        memcpy(&y, b + 4 * i, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

void orbm_epipole(const float R2w[9], const float t2w[3], const float Cw[3], float fx, float fy, float cx, float cy,
                  float* ex, float* ey) {
    // C2 = R2w*Cw + t2w: OpenCV's 3x3-by-3x1 gemm path (float products and sums, then
    // (float)(t*alpha + c*beta) in double), as pinned in DESIGN.md
    float C2[3];
    for (int i = 0; i < 3; i++) {
        const float* a = R2w + 3 * i;
        const float t0 = a[0] * Cw[0] + a[1] * Cw[1] + a[2] * Cw[2];
        C2[i] = (float)((double)t0 * 1.0 + (double)t2w[i] * 1.0);
    }
    const float invz = 1.0f / C2[2];
    *ex = fx * C2[0] * invz + cx;
    *ey = fy * C2[1] * invz + cy;
}

}  // extern "C"

static int node_feats(const orbm_kf_view* v) { return v->n_nodes ? v->node_off[v->n_nodes] : 0; }

/* ---- small per-call matchers (k_bow_small / k_tri_small): common nodes and per-call MapPoint bits in the
 * kernel arguments, node-ordered keyframe data from the keyframe cache or read by the kernel straight from
 * the pinned staging (zero copy: each element is read once, by one lane, so no H2D copy and no copy kernel
 * precede the launch), accepts + per-task done words written
 * to host memory, the rotation histogram on the host ---- */
struct SmallSide {
    const uint4* d = nullptr;
    const NodeRec* r = nullptr;  // k_tri_small
    const float* a = nullptr;    // k_bow_small: angles, a[p * a_stride]
    int a_stride = 1;
    const int32_t* f = nullptr;
};

/* carve + stage one side in node order (an uncached view), or take the cached entry's arrays */
struct SmallPlan {
    size_t od = 0, orec = 0, of = 0;
    int nf = 0;
    bool cached = false, bow = false;
};
/* bow: an uncached side stages its angles only (4 bytes a position instead of a NodeRec: the kernel reads
 * them across PCIe) */
static void small_plan(Carve& cv, const orbm_kf_view* v, const KfEntry* ce, SmallPlan& p, bool bow) {
    p.nf = node_feats(v);
    p.cached = ce != nullptr;
    p.bow = bow;
    if (ce) return;
    const size_t n = (size_t)std::max(p.nf, 1);
    p.od = cv.take(32 * n);
    p.orec = cv.take((bow ? 4 : sizeof(NodeRec)) * n);
    p.of = cv.take(4 * n);
}
static NodeRec node_rec(const float* x, const float* y, const float* ang, const int32_t* oct, const float* ur, int f) {
    NodeRec r;
    r.x = x ? x[f] : 0.f;
    r.y = y ? y[f] : 0.f;
    r.oct = (oct ? oct[f] : 0) | (ur && ur[f] >= 0.f ? 0x100 : 0);
    r.angle = ang ? ang[f] : 0.f;
    return r;
}
static SmallSide small_stage(const orbm_kf_view* v, const KfEntry* ce, const SmallPlan& p, uint8_t* hp,
                             uint8_t* dbase) {
    SmallSide s;
    if (ce) {
        s.d = (const uint4*)ce->at(ce->o_dnode);
        s.r = (const NodeRec*)ce->at(ce->o_rnode);
        s.a = &s.r->angle;
        s.a_stride = sizeof(NodeRec) / sizeof(float);
        s.f = (const int32_t*)ce->at(ce->o_feat);
        return s;
    }
    NodeRec* rec = (NodeRec*)(hp + p.orec);
    float* ang = (float*)(hp + p.orec);
    for (int q = 0; q < p.nf; q++) {
        const int f = v->node_feat[q];
        memcpy(hp + p.od + 32 * (size_t)q, v->desc + 32 * (size_t)f, 32);
        if (p.bow) ang[q] = v->angle ? v->angle[f] : 0.f;
        else rec[q] = node_rec(v->x, v->y, v->angle, v->octave, v->uright, f);
    }
    if (p.nf) memcpy(hp + p.of, v->node_feat, 4 * (size_t)p.nf);
    s.d = (const uint4*)(dbase + p.od);
    s.r = (const NodeRec*)(dbase + p.orec);
    s.a = (const float*)(dbase + p.orec);
    s.f = (const int32_t*)(dbase + p.of);
    return s;
}
/* per node position: bit set when pred(feature index) */
template <class Pred>
static void small_bits(const orbm_kf_view* v, uint32_t* bits, Pred pred) {
    const int nf = node_feats(v);
    for (int q = 0; q < nf; q++)
        if (pred(v->node_feat[q])) bits[q >> 5] |= 1u << (q & 31);
}

/* wait for every task's done word of this call, then the rotation histogram + ComputeThreeMaxima over the
 * accepts (ORBmatcher.cc:236-285 / 784-819) and the caller's output (out[x] = partner, -1 elsewhere) */
static int small_finish(orbm_ctx* ctx, const uint8_t* hp, size_t o_out, size_t o_done, const SmallTask* tasks, int nt,
                        uint32_t seq, int check_ori, int32_t* out, int nout, int* nmatches) {
    const unsigned long long* done = (const unsigned long long*)(hp + o_done);
    const unsigned long long* acc = (const unsigned long long*)(hp + o_out);
    // polled in task order: a done word, then its accepts, each final once it carries this call's seq (the
    // kernel's stores are unordered: no fence)
    int next = 0, k = 0;
    if (const int rc = wait_until(ctx->s(), [&] {
            for (; next < nt; next++, k = 0) {
                const unsigned long long d = __atomic_load_n(done + next, __ATOMIC_ACQUIRE);
                if ((uint32_t)d != seq) return false;
                for (const int na = (int)(d >> 32); k < na; k++)
                    if ((uint32_t)(__atomic_load_n(acc + tasks[next].q_begin + k, __ATOMIC_ACQUIRE) >> 37) != seq)
                        return false;
            }
            return true;
        }))
        return rc;
    int hist[30] = {0}, keep[3] = {-2, -2, -2};
    if (check_ori) {
        for (int i = 0; i < nt; i++) {
            const int na = (int)(done[i] >> 32);
            for (int j = 0; j < na; j++) hist[(acc[tasks[i].q_begin + j] >> 32) & 31]++;
        }
        three_maxima(hist, keep);
    }
    std::fill(out, out + nout, -1);
    int cnt = 0;
    for (int i = 0; i < nt; i++) {
        const int na = (int)(done[i] >> 32);
        for (int j = 0; j < na; j++) {
            const unsigned long long e = acc[tasks[i].q_begin + j];
            const int bin = (int)((e >> 32) & 31);
            if (check_ori && bin != keep[0] && bin != keep[1] && bin != keep[2]) continue;
            out[e & 0xFFFF] = (int32_t)((e >> 16) & 0xFFFF);
            cnt++;
        }
    }
    if (nmatches) *nmatches = cnt;
    return 0;
}

/* SearchByBoW through k_bow_small (every common node <= 64 candidates, <= kSmallTasks common nodes, <= 2048
 * FeatureVector entries a side) */
static int bow_small(orbm_ctx* ctx, const orbm_kf_view* vq, const orbm_kf_view* vc, const std::vector<NodeTask>& tasks,
                     float nnratio, int check_ori, int mode, int32_t* out, int nout, int* nmatches,
                     const KfEntry* cq, const KfEntry* cc) {
    const int nt = (int)tasks.size();
    Carve cv;
    SmallPlan pq, pc;
    small_plan(cv, vq, cq, pq, true);
    small_plan(cv, vc, cc, pc, true);
    const size_t o_out = cv.take(8 * (size_t)std::max(pq.nf, 1));
    const size_t o_done = cv.take(8 * (size_t)nt);
    uint8_t* hp = ctx->ensure_pinned(cv.off);
    if (!hp) return ORBX_EDEVICE;
    uint8_t* dbase = (uint8_t*)ctx->pinned_on_device(0);
    BowSmall a;
    memset(&a, 0, sizeof(a));
    const SmallSide sq = small_stage(vq, cq, pq, hp, dbase), sc = small_stage(vc, cc, pc, hp, dbase);
    a.qd = sq.d; a.qa = sq.a; a.qa_stride = sq.a_stride; a.qf = sq.f;
    a.cd = sc.d; a.ca = sc.a; a.ca_stride = sc.a_stride; a.cf = sc.f;
    auto good = [](const orbm_kf_view* v) {  // a good MapPoint: one, and not bad
        return [v](int f) { return v->has_mp && v->has_mp[f] && !(v->mp_bad && v->mp_bad[f]); };
    };
    small_bits(vq, a.qgood, good(vq));
    if (mode == 1) small_bits(vc, a.cgood, good(vc));
    for (int i = 0; i < nt; i++)
        a.tasks[i] = SmallTask{(uint16_t)tasks[i].q_begin, (uint16_t)tasks[i].q_end, (uint16_t)tasks[i].c_begin,
                               (uint16_t)tasks[i].c_end};
    a.out = (unsigned long long*)ctx->pinned_on_device(o_out);
    a.done = (unsigned long long*)ctx->pinned_on_device(o_done);
    a.seq = (int)ctx->next_seq();
    a.ntasks = nt;
    a.mode = mode;
    a.check_ori = check_ori ? 1 : 0;
    a.nnratio = nnratio;
    // the polled words start at 0, which no call carries (seq >= 1): a word left by an earlier call on this
    // context (another layout, or the same bits by chance) can never read as this call's
    memset(hp + o_out, 0, cv.off - o_out);
    HIPR(launch_bow_small(a, ctx->s()));
    return small_finish(ctx, hp, o_out, o_done, a.tasks, nt, (uint32_t)a.seq, check_ori, out, nout, nmatches);
}

/* SearchForTriangulation over common nodes through k_tri_small (<= kSmallTasks 64-query chunks, every common
 * node <= 256 candidates, <= 2048 FeatureVector entries a side) */
static int tri_small(orbm_ctx* ctx, const orbm_kf_view* kf1, const orbm_kf_view* kf2, const std::vector<NodeTask>& tasks,
                     const float F12[9], float ex, float ey, int only_stereo, int check_ori, int32_t* match12,
                     int* nmatches, const KfEntry* c1, const KfEntry* c2) {
    const int nt = (int)tasks.size();
    Carve cv;
    SmallPlan p1, p2;
    small_plan(cv, kf1, c1, p1, false);
    small_plan(cv, kf2, c2, p2, false);
    const size_t o_out = cv.take(8 * (size_t)std::max(p1.nf, 1));
    const size_t o_done = cv.take(8 * (size_t)nt);
    uint8_t* hp = ctx->ensure_pinned(cv.off);
    if (!hp) return ORBX_EDEVICE;
    uint8_t* dbase = (uint8_t*)ctx->pinned_on_device(0);
    TriSmall a;
    memset(&a, 0, sizeof(a));
    const SmallSide s1 = small_stage(kf1, c1, p1, hp, dbase), s2 = small_stage(kf2, c2, p2, hp, dbase);
    a.qd = s1.d; a.qr = s1.r; a.qf = s1.f;
    a.cd = s2.d; a.cr = s2.r; a.cf = s2.f;
    auto has_mp = [](const orbm_kf_view* v) { return [v](int f) { return v->has_mp && v->has_mp[f] != 0; }; };
    small_bits(kf1, a.qmp, has_mp(kf1));
    small_bits(kf2, a.cmp, has_mp(kf2));
    for (int i = 0; i < nt; i++)
        a.tasks[i] = SmallTask{(uint16_t)tasks[i].q_begin, (uint16_t)tasks[i].q_end, (uint16_t)tasks[i].c_begin,
                               (uint16_t)tasks[i].c_end};
    a.out = (unsigned long long*)ctx->pinned_on_device(o_out);
    a.done = (unsigned long long*)ctx->pinned_on_device(o_done);
    a.seq = (int)ctx->next_seq();
    a.ntasks = nt;
    a.check_ori = check_ori ? 1 : 0;
    a.only_stereo = only_stereo ? 1 : 0;
    a.q_ur = kf1->uright != nullptr;
    a.c_ur = kf2->uright != nullptr;
    make_geom(a.g, F12, ex, ey, kf2->nlevels, kf2->scale_factors, kf2->level_sigma2);
    memset(hp + o_out, 0, cv.off - o_out);  // polled words: 0 is no call's seq (bow_small)
    HIPR(launch_tri_small(a, ctx->s()));
    return small_finish(ctx, hp, o_out, o_done, a.tasks, nt, (uint32_t)a.seq, check_ori, match12, kf1->n, nmatches);
}

/* c1 / c2: the keyframes' cached device arrays (orbm_kf_cache), or nullptr to upload them with the call */
static int tri_common(orbm_ctx* ctx, const orbm_kf_view* kf1, const orbm_kf_view* kf2, const float F12[9], float ex,
                      float ey, int only_stereo, int check_ori, int32_t* match12, int* nmatches,
                      const KfEntry* c1 = nullptr, const KfEntry* c2 = nullptr) {
    if (const int rc_ = ctx->ready()) return rc_;
    std::vector<std::pair<int, int>> common;
    common_nodes(kf1, kf2, common);
    std::vector<NodeTask> tasks;
    for (auto& c : common) {
        const int qb = kf1->node_off[c.first], qe = kf1->node_off[c.first + 1];
        for (int q = qb; q < qe; q += 64)
            tasks.push_back({q, std::min(q + 64, qe), kf2->node_off[c.second], kf2->node_off[c.second + 1]});
    }
    const int n1 = kf1->n;
    if (tasks.empty()) {  // no common node: nothing to match
        std::fill(match12, match12 + n1, -1);
        if (nmatches) *nmatches = 0;
        return 0;
    }
    int max_nc = 0;
    for (const NodeTask& t : tasks) max_nc = std::max(max_nc, t.c_end - t.c_begin);
    if (max_nc <= 256 && tasks.size() <= (size_t)kSmallTasks && kf1->n <= 65535 && kf2->n <= 65535 &&
        node_feats(kf1) <= 32 * kSmallBitWords && node_feats(kf2) <= 32 * kSmallBitWords)
        return tri_small(ctx, kf1, kf2, tasks, F12, ex, ey, only_stereo, check_ori, match12, nmatches, c1, c2);
    // one H2D copy (views, tasks), one launch whose last workgroup writes the (rotation-filtered)
    // matches into pinned host memory pre-filled with -1, one synchronize
    Carve cv;
    ViewPlan p1, p2;
    plan_view(cv, kf1, p1, true, c1);
    plan_view(cv, kf2, p2, true, c2);
    const size_t o_tasks = cv.take(sizeof(NodeTask) * tasks.size());
    const size_t in_bytes = cv.off;
    const size_t o_list = cv.take(16 * (size_t)std::max(n1, 1));
    const size_t o_res = cv.take(4 * ((size_t)n1 + 1));
    if (ctx->scratch.ensure(cv.off)) return ORBX_EDEVICE;
    uint8_t* hp = ctx->ensure_pinned(cv.off);
    if (!hp) return ORBX_EDEVICE;
    uint8_t* base = ctx->scratch.as<uint8_t>();
    DevView d1 = stage_view(hp, base, kf1, p1, c1), d2 = stage_view(hp, base, kf2, p2, c2);
    memcpy(hp + o_tasks, tasks.data(), sizeof(NodeTask) * tasks.size());
    int32_t* res = (int32_t*)(hp + o_res);
    std::fill(res, res + n1 + 1, -1);
    HIPR(hipMemcpyAsync(base, hp, in_bytes, hipMemcpyHostToDevice, ctx->s()));
    MatchGeom g;
    make_geom(g, F12, ex, ey, kf2->nlevels, kf2->scale_factors, kf2->level_sigma2);
    const CallTail tail{ctx->call_state(), (int32_t*)(base + o_list), ctx->pinned_on_device(o_res), d1.angle, d2.angle,
                        n1, check_ori ? 1 : 0, 0};
    HIPR(launch_tri_nodes(d1, d2, (const NodeTask*)(base + o_tasks), (int)tasks.size(), g, only_stereo, tail,
                          ctx->s()));
    if (const int rc = wait_call(ctx->s(), res)) return rc;
    memcpy(match12, res + 1, 4 * (size_t)n1);
    if (nmatches) *nmatches = res[0];
    return 0;
}

extern "C" int orbm_search_for_triangulation(orbm_ctx* ctx, const orbm_kf_view* kf1, const orbm_kf_view* kf2,
                                             const float F12[9], float ex, float ey, int only_stereo, int check_ori,
                                             int32_t* match12, int* nmatches) {
    if (!ctx || !view_ok(kf1) || !view_ok(kf2) || !F12 || !match12) return ORBX_EARG;
    return tri_common(ctx, kf1, kf2, F12, ex, ey, only_stereo, check_ori, match12, nmatches);
}

extern "C" {

static int bow_common(orbm_ctx* ctx, const orbm_kf_view* vq, const orbm_kf_view* vc, float nnratio, int check_ori,
                      int mode, int32_t* out, int nout, int* nmatches, const KfEntry* cq = nullptr,
                      const KfEntry* cc = nullptr) {
    if (const int rc_ = ctx->ready()) return rc_;
    std::vector<std::pair<int, int>> common;
    common_nodes(vq, vc, common);
    std::vector<NodeTask> tasks;
    int max_nc = 1;
    for (auto& c : common) {
        NodeTask t{vq->node_off[c.first], vq->node_off[c.first + 1], vc->node_off[c.second],
                   vc->node_off[c.second + 1]};
        max_nc = std::max(max_nc, t.c_end - t.c_begin);
        tasks.push_back(t);
    }
    if (max_nc > 64 * 1024) return ORBX_EARG;
    if (tasks.empty()) {  // no common node: nothing to match
        std::fill(out, out + nout, -1);
        if (nmatches) *nmatches = 0;
        return 0;
    }
    if (max_nc <= 64 && vq->n <= 65535 && vc->n <= 65535 && tasks.size() <= (size_t)kSmallTasks && node_feats(vq) <= 32 * kSmallBitWords &&
        node_feats(vc) <= 32 * kSmallBitWords)
        return bow_small(ctx, vq, vc, tasks, nnratio, check_ori, mode, out, nout, nmatches, cq, cc);
    // one H2D copy, one launch (greedy per node; the last workgroup's rotation filter writes the
    // matches into pinned host memory pre-filled with -1), one synchronize
    Carve cv;
    ViewPlan pq, pc;
    plan_view(cv, vq, pq, false, cq);
    plan_view(cv, vc, pc, false, cc);
    const size_t o_tasks = cv.take(sizeof(NodeTask) * tasks.size());
    const size_t in_bytes = cv.off;
    const size_t o_list = cv.take(16 * (size_t)std::max(nout, 1));
    const size_t o_res = cv.take(4 * ((size_t)nout + 1));
    if (ctx->scratch.ensure(cv.off)) return ORBX_EDEVICE;
    uint8_t* hp = ctx->ensure_pinned(cv.off);
    if (!hp) return ORBX_EDEVICE;
    uint8_t* base = ctx->scratch.as<uint8_t>();
    DevView dq = stage_view(hp, base, vq, pq, cq), dc = stage_view(hp, base, vc, pc, cc);
    memcpy(hp + o_tasks, tasks.data(), sizeof(NodeTask) * tasks.size());
    int32_t* res = (int32_t*)(hp + o_res);
    std::fill(res, res + nout + 1, -1);
    HIPR(hipMemcpyAsync(base, hp, in_bytes, hipMemcpyHostToDevice, ctx->s()));
    // mode 0: out indexed by the F idx, partner = KF idx -> rot = angKF[m] - angF[i] (swap)
    const CallTail tail{ctx->call_state(), (int32_t*)(base + o_list), ctx->pinned_on_device(o_res), dq.angle,
                        dc.angle, nout, check_ori ? 1 : 0, mode == 0 ? 1 : 0};
    HIPR(launch_bow(dq, dc, (const NodeTask*)(base + o_tasks), (int)tasks.size(), max_nc, nnratio, mode, tail,
                    ctx->s()));
    if (const int rc = wait_call(ctx->s(), res)) return rc;
    memcpy(out, res + 1, 4 * (size_t)nout);
    if (nmatches) *nmatches = res[0];
    return 0;
}

int orbm_search_by_bow_kf_f(orbm_ctx* ctx, const orbm_kf_view* kf, const orbm_kf_view* f, float nnratio,
                            int check_ori, int32_t* match_f, int* nmatches) {
    if (!ctx || !view_ok(kf) || !view_ok(f) || !match_f) return ORBX_EARG;
    return bow_common(ctx, kf, f, nnratio, check_ori, 0, match_f, f->n, nmatches);
}

int orbm_search_by_bow_kf_kf(orbm_ctx* ctx, const orbm_kf_view* kf1, const orbm_kf_view* kf2, float nnratio,
                             int check_ori, int32_t* match12, int* nmatches) {
    if (!ctx || !view_ok(kf1) || !view_ok(kf2) || !match12) return ORBX_EARG;
    return bow_common(ctx, kf1, kf2, nnratio, check_ori, 1, match12, kf1->n, nmatches);
}

int orbm_triangulation_bf_batch_device(orbm_ctx* ctx, int npairs, const int32_t* d_q1, const int32_t* d_q2,
                                       const orbx_kp* d_kps, const uint8_t* d_desc, const int32_t* d_counts,
                                       int kp_stride, const float F12[9], float ex, float ey, int nlevels,
                                       const float* scale_factors, const float* level_sigma2, int check_ori,
                                       int32_t* d_match12, int32_t* d_nmatches, void* stream) {
    if (!ctx || npairs < 0 || !F12 || nlevels < 1 || nlevels > 16 || !scale_factors || !level_sigma2 ||
        kp_stride < 1 || kp_stride > 64 * 1024)  // k_tri_mfma's selection key holds 65535 - idx2 in 16 bits
        return ORBX_EARG;
    if (npairs == 0) return 0;
    HIPR(hipSetDevice(ctx->device));
    MatchGeom g;
    make_geom(g, F12, ex, ey, nlevels, scale_factors, level_sigma2);
    hipStream_t st = (hipStream_t)stream;
    TriPlan pl;
    const bool cull = ctx->tri_culled(kp_stride);
    if (cull)
        if (const int rc = ctx->tri_plan(npairs, kp_stride, pl)) return rc;
    HIPR(hipMemsetAsync(d_nmatches, 0, sizeof(int32_t) * npairs, st));
    HIPR(launch_tri_bf(npairs, d_q1, d_q2, d_kps, d_desc, d_counts, kp_stride, g, d_match12, d_nmatches, st, nullptr, 0,
                       cull ? &pl : nullptr));
    if (check_ori)
        HIPR(launch_rot_filter_pairs(npairs, d_q1, d_q2, d_kps, d_counts, kp_stride, d_match12, d_nmatches, st));
    return 0;
}

int orbm_triangulation_bf_stereo_batch_device(orbm_ctx* ctx, int npairs, const int32_t* d_q1, const int32_t* d_q2,
                                              const orbx_kp* d_kps, const uint8_t* d_desc, const int32_t* d_counts,
                                              const float* d_uright, int kp_stride, const float F12[9], float ex,
                                              float ey, int nlevels, const float* scale_factors,
                                              const float* level_sigma2, int only_stereo, int check_ori,
                                              int32_t* d_match12, int32_t* d_nmatches, void* stream) {
    if (!ctx || npairs < 0 || !F12 || nlevels < 1 || nlevels > 16 || !scale_factors || !level_sigma2 ||
        kp_stride < 1 || kp_stride > 64 * 1024 || (npairs > 0 && !d_uright))  // 16-bit index in the selection key
        return ORBX_EARG;
    if (npairs == 0) return 0;
    HIPR(hipSetDevice(ctx->device));
    MatchGeom g;
    make_geom(g, F12, ex, ey, nlevels, scale_factors, level_sigma2);
    hipStream_t st = (hipStream_t)stream;
    TriPlan pl;
    const bool cull = ctx->tri_culled(kp_stride);
    if (cull)
        if (const int rc = ctx->tri_plan(npairs, kp_stride, pl)) return rc;
    HIPR(hipMemsetAsync(d_nmatches, 0, sizeof(int32_t) * npairs, st));
    HIPR(launch_tri_bf(npairs, d_q1, d_q2, d_kps, d_desc, d_counts, kp_stride, g, d_match12, d_nmatches, st, d_uright,
                       only_stereo ? 1 : 0, cull ? &pl : nullptr));
    if (check_ori)
        HIPR(launch_rot_filter_pairs(npairs, d_q1, d_q2, d_kps, d_counts, kp_stride, d_match12, d_nmatches, st));
    return 0;
}

int orbm_triangulation_nodes_batch_device(orbm_ctx* ctx, int npairs, const int32_t* d_q1, const int32_t* d_q2,
                                          const orbx_kp* d_kps, const uint8_t* d_desc, const int32_t* d_counts,
                                          int kp_stride, const uint32_t* d_fv_node, const int32_t* d_fv_off,
                                          const int32_t* d_fv_feat, const int32_t* d_nfv, int max_nodes,
                                          const float F12[9], float ex, float ey, int nlevels,
                                          const float* scale_factors, const float* level_sigma2, int check_ori,
                                          int32_t* d_match12, int32_t* d_nmatches, void* stream) {
    if (!ctx || npairs < 0 || !F12 || nlevels < 1 || nlevels > 16 || !scale_factors || !level_sigma2 ||
        kp_stride < 1 || max_nodes < 0 || max_nodes > kp_stride)
        return ORBX_EARG;
    if (npairs == 0) return 0;
    HIPR(hipSetDevice(ctx->device));
    MatchGeom g;
    make_geom(g, F12, ex, ey, nlevels, scale_factors, level_sigma2);
    hipStream_t st = (hipStream_t)stream;
    HIPR(hipMemsetAsync(d_match12, 0xFF, sizeof(int32_t) * (size_t)npairs * kp_stride, st));
    HIPR(hipMemsetAsync(d_nmatches, 0, sizeof(int32_t) * npairs, st));
    HIPR(launch_tri_nodes_pairs(npairs, max_nodes, d_q1, d_q2, d_kps, d_desc, kp_stride, d_fv_node, d_fv_off,
                                d_fv_feat, d_nfv, g, d_match12, d_nmatches, st));
    if (check_ori)
        HIPR(launch_rot_filter_pairs(npairs, d_q1, d_q2, d_kps, d_counts, kp_stride, d_match12, d_nmatches, st));
    return 0;
}

int orbm_search_by_bow_batch_device(orbm_ctx* ctx, int npairs, int mode, const int32_t* d_qf, const int32_t* d_cf,
                                    const orbx_kp* d_kps, const uint8_t* d_desc, const int32_t* d_counts,
                                    int kp_stride, const uint8_t* d_mp_flags, const uint32_t* d_fv_node,
                                    const int32_t* d_fv_off, const int32_t* d_fv_feat, const int32_t* d_nfv,
                                    int max_nodes, float nnratio, int check_ori, int32_t* d_out,
                                    int32_t* d_nmatches, void* stream) {
    if (!ctx || npairs < 0 || (mode != 0 && mode != 1) || kp_stride < 1 || max_nodes < 0 || max_nodes > kp_stride ||
        kp_stride > 64 * 1024)
        return ORBX_EARG;
    if (npairs == 0) return 0;
    HIPR(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    HIPR(hipMemsetAsync(d_out, 0xFF, sizeof(int32_t) * (size_t)npairs * kp_stride, st));
    HIPR(hipMemsetAsync(d_nmatches, 0, sizeof(int32_t) * npairs, st));
    HIPR(launch_bow_pairs(npairs, max_nodes, d_qf, d_cf, d_desc, kp_stride, d_mp_flags, d_fv_node, d_fv_off, d_fv_feat,
                          d_nfv, nnratio, mode, d_out, st));
    if (check_ori) {
        // rows of out: (KF,KF) the query frame's features, rot = angle1 - angle2; (KF,F) the Frame's,
        // rot = angleKF - angleF (ORBmatcher.cc:236-246, 616-627)
        if (mode == 1)
            HIPR(launch_rot_filter_pairs(npairs, d_qf, d_cf, d_kps, d_counts, kp_stride, d_out, d_nmatches, st, 0));
        else
            HIPR(launch_rot_filter_pairs(npairs, d_cf, d_qf, d_kps, d_counts, kp_stride, d_out, d_nmatches, st, 1));
    } else {
        HIPR(launch_count_pairs(npairs, d_out, kp_stride, d_nmatches, st));
    }
    return 0;
}

}  // extern "C"

/* ===================================================================================== */
/* Keyframe cache (orbm_kf_cache): KeyFrames' immutable per-feature arrays kept in HBM     */
/* across the per-call matchers (LocalMapping::CreateNewMapPoints matches one KF1 against  */
/* up to 20 neighbours, LocalMapping.cc:207-268; SearchInNeighbors fuses into them)        */
/* ===================================================================================== */

/* the cached entry for (kind, key) matching this call's view, uploading (or replacing) it when absent or
 * stale (a different N, FeatureVector size, stereo presence or grid geometry); LRU eviction over the
 * capacity (KfLru). The lookup and the insertion hold the cache's mutex; a miss builds and uploads its entry on the
 * calling context's stream with the mutex released, so calls of other threads are not held behind the upload
 * (two threads missing on the same key both upload; the second insertion keeps the first one's entry).
 * Returns nullptr on a device error. */
std::shared_ptr<KfEntry> orbamd::cache_get(orbm_kf_cache* c, int kind, uint64_t key, const orbm_kf_view* kv,
                                           const orbm_frame_view* fv, hipStream_t st) {
    const int n = kv ? kv->n : fv->n;
    const int n_nodes = kv ? kv->n_nodes : 0;
    const int nfeat = kv && kv->n_nodes ? kv->node_off[kv->n_nodes] : 0;
    const bool has_ur = kv ? kv->uright != nullptr : fv->uright != nullptr;
    auto matches = [&](const KfEntry& e) {
        return e.n == n && e.n_nodes == n_nodes && e.nfeat == nfeat && (e.has_ur || !has_ur) &&
               (kind == 0 || (e.min_x == fv->min_x && e.min_y == fv->min_y && e.gw_inv == fv->grid_w_inv &&
                              e.gh_inv == fv->grid_h_inv));
    };
    if (std::shared_ptr<KfEntry> hit = c->lru.find(kind, key, matches)) return hit;
    auto e = std::make_shared<KfEntry>();
    e->n = n;
    e->n_nodes = n_nodes;
    e->nfeat = nfeat;
    e->has_ur = has_ur;
    const size_t N = (size_t)std::max(n, 1);
    Carve cv;
    e->o_desc = cv.take(32 * N);
    e->o_x = cv.take(4 * N);
    e->o_y = cv.take(4 * N);
    e->o_ang = cv.take(4 * N);
    e->o_oct = cv.take(4 * N);
    e->o_ur = cv.take(has_ur ? 4 * N : 0);
    e->o_feat = cv.take(4 * (size_t)std::max(nfeat, 1));
    if (kind == 0) {
        e->o_dnode = cv.take(32 * (size_t)std::max(nfeat, 1));
        e->o_rnode = cv.take(sizeof(NodeRec) * (size_t)std::max(nfeat, 1));
    }
    size_t o_call = 0;
    if (kind == 1) {
        e->has_grid = true;
        e->min_x = fv->min_x;
        e->min_y = fv->min_y;
        e->gw_inv = fv->grid_w_inv;
        e->gh_inv = fv->grid_h_inv;
        e->o_gs = cv.take(4 * (kGridCols * kGridRows + 1));
        e->o_gi = cv.take(2 * N);
        o_call = cv.take(sizeof(ProjCall));
    }
    if (hipSetDevice(c->device) != hipSuccess || e->buf.ensure(cv.off)) return nullptr;
    std::vector<uint8_t> h(cv.off, 0);
    const uint8_t* desc = kv ? kv->desc : fv->desc;
    const float* x = kv ? kv->x : fv->x;
    const float* y = kv ? kv->y : fv->y;
    const float* ang = kv ? kv->angle : fv->angle;
    const int32_t* oct = kv ? kv->octave : fv->octave;
    const float* ur = kv ? kv->uright : fv->uright;
    if (n) {
        memcpy(h.data() + e->o_desc, desc, 32 * (size_t)n);
        memcpy(h.data() + e->o_x, x, 4 * (size_t)n);
        memcpy(h.data() + e->o_y, y, 4 * (size_t)n);
        if (ang) memcpy(h.data() + e->o_ang, ang, 4 * (size_t)n);
        memcpy(h.data() + e->o_oct, oct, 4 * (size_t)n);
        if (has_ur) memcpy(h.data() + e->o_ur, ur, 4 * (size_t)n);
    }
    if (nfeat) memcpy(h.data() + e->o_feat, kv->node_feat, 4 * (size_t)nfeat);
    if (kind == 0)
        for (int p = 0; p < nfeat; p++) {
            const int f = kv->node_feat[p];
            memcpy(h.data() + e->o_dnode + 32 * (size_t)p, desc + 32 * (size_t)f, 32);
            const NodeRec r = node_rec(x, y, ang, oct, has_ur ? ur : nullptr, f);
            memcpy(h.data() + e->o_rnode + sizeof(NodeRec) * (size_t)p, &r, sizeof(r));
        }
    if (kind == 1) {  // the KeyFrame's grid (AssignFeaturesToGrid), built once by k_grid
        ProjCall pc;
        memset(&pc, 0, sizeof(pc));
        pc.x = (const float*)e->at(e->o_x);
        pc.y = (const float*)e->at(e->o_y);
        pc.n = n;
        pc.min_x = fv->min_x;
        pc.min_y = fv->min_y;
        pc.gw_inv = fv->grid_w_inv;
        pc.gh_inv = fv->grid_h_inv;
        pc.grid_start = (int*)e->at(e->o_gs);
        pc.grid_idx = (uint16_t*)e->at(e->o_gi);
        memcpy(h.data() + o_call, &pc, sizeof(pc));
    }
    if (hipMemcpyAsync(e->buf.p, h.data(), cv.off, hipMemcpyHostToDevice, st) != hipSuccess) return nullptr;
    if (kind == 1 && launch_projection((const ProjCall*)e->at(o_call), 1, 0, st, false) != hipSuccess) return nullptr;
    if (hipStreamSynchronize(st) != hipSuccess) return nullptr;
    return c->lru.insert(kind, key, e, matches);  // another thread's matching entry, if it inserted one meanwhile
}

extern "C" {

int orbm_kf_cache_create(int device, size_t capacity_bytes, orbm_kf_cache** out) {
    if (!out) return ORBX_EARG;
    *out = nullptr;
    if (device < 0 || device >= orbx_device_count()) return ORBX_EDEVICE;
    HIPR(hipSetDevice(device));
    orbm_kf_cache* c = new orbm_kf_cache(capacity_bytes ? capacity_bytes : (size_t)1 << 30);
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return ORBX_EDEVICE;
    }
    *out = c;
    return 0;
}

void orbm_kf_cache_destroy(orbm_kf_cache* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->lru.clear();
    (void)hipStreamDestroy(c->stream);
    delete c;
}

int orbm_kf_cache_erase(orbm_kf_cache* c, uint64_t key) {
    if (!c) return ORBX_EARG;
    c->lru.erase(key);
    return 0;
}

int orbm_kf_cache_stats(orbm_kf_cache* c, int* entries, size_t* bytes, long long* hits, long long* misses) {
    if (!c) return ORBX_EARG;
    c->lru.stats(entries, bytes, hits, misses);
    return 0;
}

int orbm_search_for_triangulation_cached(orbm_ctx* ctx, orbm_kf_cache* cache, uint64_t key1, const orbm_kf_view* kf1,
                                         uint64_t key2, const orbm_kf_view* kf2, const float F12[9], float ex, float ey,
                                         int only_stereo, int check_ori, int32_t* match12, int* nmatches) {
    if (!ctx || !cache || cache->device != ctx->device || !view_ok(kf1) || !view_ok(kf2) || !F12 || !match12)
        return ORBX_EARG;
    if (const int rc_ = ctx->ready()) return rc_;
    const std::shared_ptr<KfEntry> c1 = cache_get(cache, 0, key1, kf1, nullptr, ctx->s());
    const std::shared_ptr<KfEntry> c2 = c1 ? cache_get(cache, 0, key2, kf2, nullptr, ctx->s()) : nullptr;
    if (!c1 || !c2) return ORBX_EDEVICE;
    return tri_common(ctx, kf1, kf2, F12, ex, ey, only_stereo, check_ori, match12, nmatches, c1.get(), c2.get());
}

int orbm_search_by_bow_kf_kf_cached(orbm_ctx* ctx, orbm_kf_cache* cache, uint64_t key1, const orbm_kf_view* kf1,
                                    uint64_t key2, const orbm_kf_view* kf2, float nnratio, int check_ori,
                                    int32_t* match12, int* nmatches) {
    if (!ctx || !cache || cache->device != ctx->device || !view_ok(kf1) || !view_ok(kf2) || !match12)
        return ORBX_EARG;
    if (const int rc_ = ctx->ready()) return rc_;
    const std::shared_ptr<KfEntry> c1 = cache_get(cache, 0, key1, kf1, nullptr, ctx->s());
    const std::shared_ptr<KfEntry> c2 = c1 ? cache_get(cache, 0, key2, kf2, nullptr, ctx->s()) : nullptr;
    if (!c1 || !c2) return ORBX_EDEVICE;
    return bow_common(ctx, kf1, kf2, nnratio, check_ori, 1, match12, kf1->n, nmatches, c1.get(), c2.get());
}

int orbm_search_by_bow_kf_f_cached(orbm_ctx* ctx, orbm_kf_cache* cache, uint64_t key, const orbm_kf_view* kf,
                                   const orbm_kf_view* f, float nnratio, int check_ori, int32_t* match_f,
                                   int* nmatches) {
    if (!ctx || !cache || cache->device != ctx->device || !view_ok(kf) || !view_ok(f) || !match_f) return ORBX_EARG;
    if (const int rc_ = ctx->ready()) return rc_;
    const std::shared_ptr<KfEntry> ck = cache_get(cache, 0, key, kf, nullptr, ctx->s());
    if (!ck) return ORBX_EDEVICE;
    return bow_common(ctx, kf, f, nnratio, check_ori, 0, match_f, f->n, nmatches, ck.get(), nullptr);
}

}  // extern "C"
