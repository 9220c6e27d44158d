/*
 * check_so3_sincos.c -- measures the distance of so3_sincos (csrc/pose_math.h, the project's own double sin / cos of
 * SE3Quat::exp) from the host libm: a dense sample of [1e-5, pi] plus directed values (the reduction's breakpoints
 * (2k+1) pi/4 and their neighbours, 1e-5, multiples of pi/2 +- 1 ulp, large arguments), the largest difference in
 * ULP of the libm value. A record (DESIGN.md "Pinned semantics"), not a gate: the routine is not libm's and is not
 * meant to be; a wrong coefficient shows as thousands of ULP.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -I cooperative-orb-slam_amd/csrc tools/check_so3_sincos.c -lm
 *   ./a.out [samples]      (default 4000000)
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define PM_FN static inline
#include "pose_math.h"

static double ulps(double got, double ref) {
    if (got == ref) return 0;
    int e;
    frexp(ref, &e);
    double ulp = ldexp(1.0, e - 53);
    if (ref == 0) ulp = 0x1p-1074;
    return fabs(got - ref) / ulp;
}

static double worst_s, worst_c, at_s, at_c;
/* near a zero of sin or cos the reduced argument's own rounding dominates; the absolute error is reported too */
static double worst_abs;

static void probe(double th) {
    double s, c;
    so3_sincos(th, &s, &c);
    const double us = ulps(s, sin(th)), uc = ulps(c, cos(th));
    if (us > worst_s) worst_s = us, at_s = th;
    if (uc > worst_c) worst_c = uc, at_c = th;
    const double a = fmax(fabs(s - sin(th)), fabs(c - cos(th)));
    if (a > worst_abs) worst_abs = a;
}

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 4000000;
    const double pi = acos(-1.0);
    for (long i = 0; i <= n; i++) probe(1e-5 + (pi - 1e-5) * (double)i / (double)n);
    printf("dense [1e-5, pi], %ld samples: sin %.3f ulp at %.17g, cos %.3f ulp at %.17g, abs %.3g\n", n + 1, worst_s,
           at_s, worst_c, at_c, worst_abs);
    const double dense_s = worst_s, dense_c = worst_c;
    worst_s = worst_c = worst_abs = 0;
    probe(1e-5);
    for (int k = 1; k <= 16; k++) {
        double v[2] = {k * (pi / 4), k * (pi / 2)};
        for (int j = 0; j < 2; j++) {
            probe(v[j]);
            probe(nextafter(v[j], 0));
            probe(nextafter(v[j], 1e9));
        }
    }
    printf("directed (k pi/4, k pi/2 +- 1 ulp, 1e-5): sin %.3f ulp at %.17g, cos %.3f ulp at %.17g, abs %.3g\n",
           worst_s, at_s, worst_c, at_c, worst_abs);
    /* away from the zeros: the figure DESIGN.md quotes */
    worst_s = worst_c = 0;
    for (long i = 0; i <= n; i++) {
        const double th = 1e-5 + (pi - 1e-5) * (double)i / (double)n;
        if (fabs(sin(th)) > 0x1p-10 && fabs(cos(th)) > 0x1p-10) probe(th);
    }
    printf("dense, |sin|, |cos| > 2^-10: sin %.3f ulp, cos %.3f ulp\n", worst_s, worst_c);
    printf("max ulp over the dense sample: %.3f\n", fmax(dense_s, dense_c));
    return 0;
}
