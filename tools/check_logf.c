/* check_logf.c -- exhaustive check that the device's restatement of glibc logf
 * (cooperative-orb-slam_amd/csrc/orb_math.h: glibc_logf, the log of MapPoint::PredictScale) equals the host
 * libm for every positive normal float, in both evaluation orders glibc ships (the FMA ifunc variant and
 * the plain one, which differ only in contraction). The device form is the plain one, stated with
 * __dmul_rn / __dadd_rn.
 * glibc 2.35 sysdeps/ieee754/flt-32/e_logf.c: a 16-entry {invc, logc} table indexed by the top mantissa
 * bits of ix - 0x3f330000, r = z * invc - 1, a degree-3 polynomial in double, one rounding to float; the
 * constants below were read from libm's .rodata (__logf_data).
 * Build: gcc -O2 -ffp-contract=off tools/check_logf.c -o /tmp/check_logf -lm && /tmp/check_logf [stride]
 * stride (default 1) checks every stride-th bit pattern; the test suite runs stride 997, the full range is
 * the manual check (about 15 s on one core). Result with glibc 2.35: 0 mismatches of 2,130,706,432 in
 * either evaluation. Exit status 1 on any mismatch. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const double T[16][2] = {
    {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2}, {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2},
    {0x1.49539f0f010bp+0, -0x1.01eae7f513a67p-2},  {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3},
    {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3}, {0x1.25e227b0b8eap+0, -0x1.1aa2bc79c81p-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4}, {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4},
    {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5},  {0x1.ca4b31f026aap-1, 0x1.c5e53aa362eb4p-4},
    {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d22477p-3},
    {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2},  {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2}};
static const double Ln2 = 0x1.62e42fefa39efp-1;
static const double A[3] = {-0x1.00ea348b88334p-2, 0x1.5575b0be00b6ap-2, -0x1.ffffef20a4123p-2};

static int use_fma = 0;
static double F(double a, double b, double c) { return use_fma ? fma(a, b, c) : a * b + c; }

/* a positive normal float only */
static float emu(float x) {
    uint32_t ix;
    memcpy(&ix, &x, 4);
    if (ix == 0x3f800000) return 0;
    const uint32_t tmp = ix - 0x3f330000;
    const int i = (tmp >> 19) & 15;
    const int k = (int32_t)tmp >> 23;
    const uint32_t iz = ix - (tmp & 0xff800000u);
    float zf;
    memcpy(&zf, &iz, 4);
    const double z = (double)zf;
    const double r = F(z, T[i][0], -1.0);
    const double y0 = F((double)k, Ln2, T[i][1]);
    const double r2 = r * r;
    double y = F(A[1], r, A[2]);
    y = F(A[0], r2, y);
    y = F(y, r2, y0 + r);
    return (float)y;
}

int main(int argc, char** argv) {
    const uint32_t stride = argc > 1 ? (uint32_t)strtoul(argv[1], 0, 10) : 1;
    if (stride == 0) return 2;
    long bad = 0;
    for (use_fma = 1; use_fma >= 0; use_fma--) {
        long n = 0, tot = 0;
        for (uint64_t u = 0x00800000u; u < 0x7f800000u; u += stride) {
            const uint32_t w = (uint32_t)u;
            float x;
            memcpy(&x, &w, 4);
            const float a = emu(x), b = logf(x);
            n += memcmp(&a, &b, 4) != 0;
            tot++;
        }
        printf("%s evaluation: %ld floats, logf mismatches %ld\n", use_fma ? "FMA" : "no-FMA", tot, n);
        bad += n;
    }
    return bad != 0;
}
