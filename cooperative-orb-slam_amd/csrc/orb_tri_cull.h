/*
 * orb_tri_cull.h -- the epipolar tile cull of the BF SearchForTriangulation scan (k_tri_order / k_tri_mfma,
 * match_kernels.hip): the ordering scalars that make a wave's queries and a tile's candidates spatially coherent,
 * the tile record, and the conservative test that a whole 32-candidate tile holds no candidate a query's
 * CheckDistEpipolarLine (epi_ok_f) can accept. Plain C++ (host and device): the kernels and the CPU test
 * (tests/cpp/tri_cull_host.cpp) share every line. The ordering only decides how many tiles survive; the cull test
 * alone has to be right, and it fails safe (DESIGN.md "Matcher semantics").
 */
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ORB_HD __host__ __device__ inline
#else
#define ORB_HD inline
#endif

namespace orbamd {

constexpr int kTriOrdIdxBits = 12;
constexpr int kTriOrdCap = 1 << kTriOrdIdxBits;  // features per frame the LDS sort holds (sort key: scalar << 12 | index)
constexpr int kTriTile = 32;                     // candidates per tile = rows of one MFMA

/* one 32-candidate tile of the ordered candidates: bounding box of its live candidates (threshold >= 0) and the
 * largest of their thresholds th384f[octave]; no live candidate: thf = -1 (and an empty box) */
struct TriTile {
    float xmin, xmax, ymin, ymax, thf, pad0, pad1, pad2;
};

/* What k_tri_order leaves for k_tri_mfma, per pair p of a launch (S = the launch's row stride, a multiple of 64,
 * <= kTriOrdCap; device pointers into the context's scratch):
 *   permQ[p * S + k]        original index of the k-th query in query order
 *   sdesc[(p * S + k) * 32] descriptor of the k-th candidate in candidate order (rows of a tile ascend in the
 *                           original index), srec[(p * S + k) * 4] its record: x, y, the threshold th384f[octave]
 *                           or -1 when it takes no part, and the bits original index | near-epipole flag << 16
 *   tiles[p * S / 32 + t]   the record of tile t
 * stats (measurement hook, or null): tiles whose MFMAs ran / tiles of every wave with a query, summed */
struct TriPlan {
    uint16_t* permQ;
    uint8_t* sdesc;
    float* srec;
    TriTile* tiles;
    unsigned long long* stats;
    int S;
};

/* Every epipolar line F12^T x1 passes through the epipole e (F12 e = 0), so a line is named by where it meets a
 * fixed reference line r, and a candidate by where the line through e and itself meets r. r passes through c0,
 * perpendicular to the direction n from c0 to e: an epipole at infinity (parallel lines) then gives the signed
 * distance to the centre line, an epipole in the image a monotone function of the angle about it.
 * kappa = 1 / |e - c0| (signed, 0 at infinity). */
struct TriOrd {
    float nx, ny, ux, uy, kappa, c0x, c0y;
};

ORB_HD TriOrd tri_ord_make(const float* F) {
    // e = the cross product of two rows of F12 (each row is perpendicular to e): the pair of largest norm
    // (of F over its largest entry: F is homogeneous, and the products of a small one would underflow)
    float s = 0.f, G[9];
    for (int i = 0; i < 9; i++) s = fmaxf(s, fabsf(F[i]));
    for (int i = 0; i < 9; i++) G[i] = F[i] / s;
    float best = -1.f, ex = 0.f, ey = 0.f, ew = 0.f;
    for (int i = 0; i < 3; i++) {
        const float* r0 = G + 3 * i;
        const float* r1 = G + 3 * ((i + 1) % 3);
        const float cx = r0[1] * r1[2] - r0[2] * r1[1], cy = r0[2] * r1[0] - r0[0] * r1[2];
        const float cw = r0[0] * r1[1] - r0[1] * r1[0];
        const float nn = cx * cx + cy * cy + cw * cw;
        if (nn > best) { best = nn; ex = cx; ey = cy; ew = cw; }
    }
    TriOrd o;
    o.c0x = 0.f;
    o.c0y = 0.f;
    if (ex * ex + ey * ey < 4096.f * ew * ew) o.c0x = 1024.f;  // e within 64 px of the origin: measure from elsewhere
    const float dx = ex - ew * o.c0x, dy = ey - ew * o.c0y;
    const float L = sqrtf(dx * dx + dy * dy);
    o.nx = dx / L;
    o.ny = dy / L;
    o.ux = -o.ny;
    o.uy = o.nx;
    o.kappa = ew / L;
    return o;  // F = 0: NaNs, every key below is then 0 and the order is the index order
}

/* position t along r squashed to 20 bits, monotone; NaN / inf (a line parallel to r, F = 0, NaN coordinates): 0 */
ORB_HD uint32_t tri_ord_key(float t) {
    float g = t / (fabsf(t) + 512.f) + 1.f;  // (0, 2)
    if (!(g >= 0.f)) g = 0.f;
    if (g > 2.f) g = 2.f;
    return (uint32_t)(g * 524287.5f);
}
/* candidate (x, y): with d = (x, y) - c0, the line through e and (x, y) meets r at u.d / (1 - kappa n.d) */
ORB_HD uint32_t tri_cand_key(const TriOrd& o, float x, float y) {
    const float dx = x - o.c0x, dy = y - o.c0y;
    return tri_ord_key((o.ux * dx + o.uy * dy) / (1.f - o.kappa * (o.nx * dx + o.ny * dy)));
}
/* query line (a, b, c): its meet with r = (n, -n.c0) is l x r; position along u from c0 */
ORB_HD uint32_t tri_query_key(const TriOrd& o, float a, float b, float c) {
    const float rz = -(o.nx * o.c0x + o.ny * o.c0y);
    const float px = b * rz - c * o.ny, py = c * o.nx - a * rz, pw = a * o.ny - b * o.nx;
    return tri_ord_key((o.ux * px + o.uy * py) / pw - (o.ux * o.c0x + o.uy * o.c0y));
}

/* True when no candidate of tile t can pass epi_ok_f(a, b, c, x2, y2, thf2) for the query line (a, b, c).
 *
 * Exact arithmetic: num(x, y) = a x + b y + c is linear, so over the tile's box |num| >= m, with m = 0 when the
 * four corner values differ in sign and their smallest magnitude otherwise. A candidate passes only with
 * num^2 / den < thf2 <= thf_max, den = a^2 + b^2, so m^2 >= thf_max den rules the whole tile out.
 *
 * Float arithmetic (u = 2^-24): epi_ok_f rounds num three times (two products, two sums, of which the first sum's
 * error and the products' combine to at most 3u E with E = |a| X + |b| Y + |c| >= every partial sum, X / Y the
 * largest |x| / |y| of the box), so its num is within 3u E of the exact one, as is each corner value computed here
 * (an fma only tightens that): 6u E between the m computed here and the |num| epi_ok_f sees. den has two rounded
 * products and a rounded sum, the square and the divide one rounding each, the product thf_max den here one more:
 * a relative error below 6u on the comparison of m^2 with thf_max den. The slacks applied are 2^-14 E = 1024u E
 * absolute (170 times 6u E) and a factor 1 + 2^-13 = 1 + 2048u (340 times 6u); at E ~ 1e3 lines-in-pixels that is
 * 0.06 px against a band of +-2 px or more, so no tile is kept for it.
 *
 * Fail safe: a NaN in any comparison leaves the tile alive; so does a den outside [1e-30, 1e30], where squares
 * and products leave the normal range. den == 0 or thf_max < 0: epi_ok_f rejects every candidate, the tile is
 * dead. */
ORB_HD bool tri_tile_dead(float a, float b, float c, const TriTile& t) {
    const float den = a * a + b * b;
    if (den == 0.f || t.thf < 0.f) return true;
    if (!(den >= 1e-30f && den <= 1e30f)) return false;
    const float v0 = a * t.xmin + b * t.ymin + c, v1 = a * t.xmax + b * t.ymin + c;
    const float v2 = a * t.xmin + b * t.ymax + c, v3 = a * t.xmax + b * t.ymax + c;
    float m = 0.f;
    if (v0 > 0.f && v1 > 0.f && v2 > 0.f && v3 > 0.f) m = fminf(fminf(v0, v1), fminf(v2, v3));
    else if (v0 < 0.f && v1 < 0.f && v2 < 0.f && v3 < 0.f) m = -fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
    const float X = fmaxf(fabsf(t.xmin), fabsf(t.xmax)), Y = fmaxf(fabsf(t.ymin), fabsf(t.ymax));
    const float E = fabsf(a) * X + fabsf(b) * Y + fabsf(c);
    const float mm = m - 6.103515625e-5f * E;  // 2^-14 E
    return mm > 0.f && mm * mm > t.thf * den * 1.0001220703125f;  // 1 + 2^-13
}

}  // namespace orbamd
