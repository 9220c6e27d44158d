/* check_atan2f.c -- check that the device's restatement of glibc atan2f in the first quadrant
 * (cooperative-orb-slam_amd/csrc/orb_math.h: glibc_atanf_pos / glibc_atan2f, the atan2 of cosParallaxStereo in
 * LocalMapping::CreateNewMapPoints, LocalMapping.cc:312) equals the host libm. The device form states every
 * operation with __fmul_rn / __fadd_rn / __fdiv_rn; this file states the same sequence in C (build it with
 * -ffp-contract=off).
 * glibc 2.35 sysdeps/ieee754/flt-32/s_atanf.c, e_atan2f.c (the fdlibm float forms): atanf has the break points
 * 0.4375, 0.6875, 1.1875, 2.4375, the 4-entry atanhi / atanlo tables and the 11-term aT polynomial split into odd
 * and even parts; it returns x below 2^-29 and atanhi[3] + atanlo[3] from ATAN_BIG up. atan2f(y, x), y > 0, x > 0:
 * atanf(y) for x == 1, pi/2 for an exponent gap above 60, else atanf(fabsf(y / x)).
 * Build: gcc -O2 -ffp-contract=off tools/check_atan2f.c -o /tmp/check_atan2f -lm && /tmp/check_atan2f [stride]
 * Part 1: atanf on every stride-th positive finite float (stride 1: all 2,139,095,039). Part 2: atan2f on
 * 20,000,000 / stride (at least 20,000) pseudo-random first-quadrant pairs over the whole exponent range, plus
 * directed pairs (x == 1, exponent gaps 59..62, denormal quotients). The test suite runs stride 997; stride 3 is the
 * manual check (about 5 s on one core). Result with glibc 2.35: see RESULT below. Exit status 1 on any mismatch. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* RESULT (glibc 2.35, x86-64): stride 3: atanf 713,031,680 floats, 0 mismatches; atan2f 8,356,859 pairs (random and
 * directed), 0 mismatches. The constants are the bits of fdlibm's decimal literals: aT[0] is 0x3eaaaaab, not the
 * 0x3eaaaaaa of its comment, and the big-argument branch starts at 2^25. */

static float fu(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t uf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

#define ATAN_BIG 0x4c000000u /* 2^25 */

static float atanf_pos(float x) {
    static const uint32_t hi[4] = {0x3eed6338u, 0x3f490fdau, 0x3f7b985eu, 0x3fc90fdau};
    static const uint32_t lo[4] = {0x31ac3769u, 0x33222168u, 0x33140fb4u, 0x33a22168u};
    static const uint32_t aT[11] = {0x3eaaaaabu, 0xbe4ccccdu, 0x3e124925u, 0xbde38e38u, 0x3dba2e6eu, 0xbd9d8795u,
                                    0x3d886b35u, 0xbd6ef16bu, 0x3d4bda59u, 0xbd15a221u, 0x3c8569d7u};
    const uint32_t ix = uf(x);
    int id = -1;
    if (ix >= ATAN_BIG) return fu(hi[3]) + fu(lo[3]);
    if (ix < 0x3ee00000u) {
        if (ix < 0x31000000u) return x;
    } else if (ix < 0x3f980000u) {
        if (ix < 0x3f300000u) {
            id = 0;
            x = (2.0f * x - 1.0f) / (2.0f + x);
        } else {
            id = 1;
            x = (x - 1.0f) / (x + 1.0f);
        }
    } else if (ix < 0x401c0000u) {
        id = 2;
        x = (x - 1.5f) / (1.0f + 1.5f * x);
    } else {
        id = 3;
        x = -1.0f / x;
    }
    const float z = x * x, w = z * z;
    const float s1 =
        z * (fu(aT[0]) + w * (fu(aT[2]) + w * (fu(aT[4]) + w * (fu(aT[6]) + w * (fu(aT[8]) + w * fu(aT[10]))))));
    const float s2 = w * (fu(aT[1]) + w * (fu(aT[3]) + w * (fu(aT[5]) + w * (fu(aT[7]) + w * fu(aT[9])))));
    if (id < 0) return x - x * (s1 + s2);
    return fu(hi[id]) - ((x * (s1 + s2) - fu(lo[id])) - x);
}

static float atan2f_q1(float y, float x) {
    const int32_t hx = (int32_t)uf(x), hy = (int32_t)uf(y);
    if (hx == 0x3f800000) return atanf_pos(y);
    const int k = (hy - hx) >> 23;
    if (k > 60) return fu(0x3fc90fdbu) + 0.5f * fu(0xb3bbbd2eu);
    return atanf_pos(fabsf(y / x));
}

static uint64_t rng = 0x9e3779b97f4a7c15ull;
static uint32_t next(void) {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return (uint32_t)(rng >> 16);
}

static long pair_bad(float y, float x) {
    const float a = atan2f_q1(y, x), b = atan2f(y, x);
    return memcmp(&a, &b, 4) != 0;
}

int main(int argc, char** argv) {
    const uint32_t stride = argc > 1 ? (uint32_t)strtoul(argv[1], 0, 10) : 1;
    if (stride == 0) return 2;
    long n = 0, tot = 0;
    for (uint64_t u = 1; u < 0x7f800000u; u += stride) {
        const float x = fu((uint32_t)u);
        const float a = atanf_pos(x), b = atanf(x);
        n += memcmp(&a, &b, 4) != 0;
        tot++;
    }
    printf("atanf: %ld floats, mismatches %ld\n", tot, n);
    long n2 = 0, tot2 = 0;
    long pairs = 20000000 / stride;
    if (pairs < 20000) pairs = 20000;
    for (long i = 0; i < pairs; i++) { /* any positive finite float on either side */
        const float y = fu(1 + next() % (0x7f800000u - 1)), x = fu(1 + next() % (0x7f800000u - 1));
        n2 += pair_bad(y, x);
        tot2++;
    }
    for (long i = 0; i < pairs / 4; i++) { /* quotients of ordinary size: y / x in 2^-8 .. 2^8 */
        const float x = fu(0x3c000000u + next() % 0x08000000u);
        const float y = x * fu(0x3b800000u + next() % 0x08000000u);
        n2 += pair_bad(y, x);
        tot2++;
    }
    for (int e = 1; e < 254; e++) /* x == 1; exponent gaps around 60; quotients that underflow */
        for (uint32_t m = 0; m < 0x800000u; m += 0x155555u) {
            const float y = fu(((uint32_t)e << 23) | m);
            n2 += pair_bad(y, 1.0f);
            tot2++;
            for (int gap = 58; gap <= 63; gap++) {
                if (e - gap >= 1) {
                    n2 += pair_bad(y, fu(((uint32_t)(e - gap) << 23) | (m ^ 0x2aaaaau)));
                    n2 += pair_bad(y, fu((uint32_t)(e - gap) << 23));
                    tot2 += 2;
                }
                if (e + 2 * gap <= 254) {
                    n2 += pair_bad(y, fu(((uint32_t)(e + 2 * gap) << 23) | (m ^ 0x2aaaaau)));
                    tot2++;
                }
            }
        }
    printf("atan2f: %ld pairs, mismatches %ld\n", tot2, n2);
    return (n | n2) != 0;
}
