// Host build of csrc/orb_tri_cull.h for tests/test_tri_cull_bound.py: the ordering, the tile records and the cull
// test of the BF SearchForTriangulation scan exactly as k_tri_order / k_tri_mfma state them (same header, same
// sort keys), over arrays the test passes in. No HIP, no GPU.
#include <algorithm>
#include <vector>

#include "../../cooperative-orb-slam_amd/csrc/orb_tri_cull.h"

using namespace orbamd;

static void line_of(const float* F, float x1, float y1, float* a, float* b, float* c) {  // epi_line (orb_match_dev.h)
    *a = x1 * F[0] + y1 * F[3] + F[6];
    *b = x1 * F[1] + y1 * F[4] + F[7];
    *c = x1 * F[2] + y1 * F[5] + F[8];
}

static void order(std::vector<uint32_t>& k, uint16_t* perm) {
    std::sort(k.begin(), k.end());
    for (size_t i = 0; i < k.size(); i++) perm[i] = (uint16_t)(k[i] & (kTriOrdCap - 1));
}

extern "C" {

int tricull_cap(void) { return kTriOrdCap; }

/* xy1 / xy2: n x 2 floats; thf2: each candidate's threshold (th384f[octave], or -1 when it takes no part).
 * permQ[n1], permC[n2]: sorted position -> original index; tiles: ntiles x 8 floats (TriTile);
 * dead[qpos * ntiles + t]: tri_tile_dead of the query at sorted position qpos against tile t. */
int tricull_plan(const float* F, int n1, const float* xy1, int n2, const float* xy2, const float* thf2,
                 uint16_t* permQ, uint16_t* permC, float* tiles, uint8_t* dead) {
    if (n1 < 0 || n2 < 0 || n1 > kTriOrdCap || n2 > kTriOrdCap) return -1;
    const TriOrd o = tri_ord_make(F);
    std::vector<uint32_t> kq(n1), kc(n2);
    for (int i = 0; i < n1; i++) {
        float a, b, c;
        line_of(F, xy1[2 * i], xy1[2 * i + 1], &a, &b, &c);
        kq[i] = tri_query_key(o, a, b, c) << kTriOrdIdxBits | (uint32_t)i;
    }
    for (int j = 0; j < n2; j++) kc[j] = tri_cand_key(o, xy2[2 * j], xy2[2 * j + 1]) << kTriOrdIdxBits | (uint32_t)j;
    order(kq, permQ);
    order(kc, permC);
    const int ntiles = (n2 + kTriTile - 1) / kTriTile;
    TriTile* T = (TriTile*)tiles;
    for (int t = 0; t < ntiles; t++) {
        const int b0 = t * kTriTile, b1 = std::min(n2, b0 + kTriTile);
        std::sort(permC + b0, permC + b1);  // rows of a tile ascend in the original index
        TriTile r = {INFINITY, -INFINITY, INFINITY, -INFINITY, -1.f, 0.f, 0.f, 0.f};
        for (int k = b0; k < b1; k++) {
            const int j = permC[k];
            if (!(thf2[j] >= 0.f)) continue;
            r.xmin = fminf(r.xmin, xy2[2 * j]);
            r.xmax = fmaxf(r.xmax, xy2[2 * j]);
            r.ymin = fminf(r.ymin, xy2[2 * j + 1]);
            r.ymax = fmaxf(r.ymax, xy2[2 * j + 1]);
            r.thf = fmaxf(r.thf, thf2[j]);
        }
        T[t] = r;
    }
    for (int q = 0; q < n1; q++) {
        float a, b, c;
        line_of(F, xy1[2 * permQ[q]], xy1[2 * permQ[q] + 1], &a, &b, &c);
        for (int t = 0; t < ntiles; t++) dead[(size_t)q * ntiles + t] = tri_tile_dead(a, b, c, T[t]) ? 1 : 0;
    }
    return ntiles;
}

}  // extern "C"
