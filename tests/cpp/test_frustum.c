/* test_frustum.c -- the host unit of Frame::isInFrustum (csrc/frustum.c, orbx_is_in_frustum) over the vectors the
 * Python restatement wrote (tests/golden/frustum_vectors.txt, tests/frustum_py.py), bit for bit, with its argument
 * checks and the contract's exclusions. Plain C with its own main: built once normally and once under ASan + UBSan
 * (tests/cpp/build_frustum.sh), from this file and csrc/frustum.c alone, no library.
 *   test_frustum <fixture> */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "orbslam_amd.h"

static int fails = 0;
#define CHECK(c)                                               \
    do {                                                       \
        if (!(c)) {                                            \
            fails++;                                           \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                      \
    } while (0)

static float fbits(unsigned u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

typedef struct {
    uint8_t* in_view;
    float *x, *y, *xr, *vc;
    int32_t* level;
} outs;

static outs outs_alloc(int n) { /* exact-size heap arrays: an access past row n - 1 is the sanitizer's to see */
    outs o;
    o.in_view = (uint8_t*)malloc((size_t)n);
    o.x = (float*)malloc(4 * (size_t)n);
    o.y = (float*)malloc(4 * (size_t)n);
    o.xr = (float*)malloc(4 * (size_t)n);
    o.vc = (float*)malloc(4 * (size_t)n);
    o.level = (int32_t*)malloc(4 * (size_t)n);
    return o;
}
static void outs_fill(outs* o, int n, int byte) {
    memset(o->in_view, byte, (size_t)n);
    memset(o->x, byte, 4 * (size_t)n);
    memset(o->y, byte, 4 * (size_t)n);
    memset(o->xr, byte, 4 * (size_t)n);
    memset(o->vc, byte, 4 * (size_t)n);
    memset(o->level, byte, 4 * (size_t)n);
}
static int outs_all(const outs* o, int n, int byte) {
    int ok = 1;
    for (int i = 0; i < n; i++)
        ok &= o->in_view[i] == byte && ((unsigned char*)o->x)[4 * i] == byte && ((unsigned char*)o->y)[4 * i] == byte &&
              ((unsigned char*)o->xr)[4 * i] == byte && ((unsigned char*)o->vc)[4 * i] == byte &&
              ((unsigned char*)o->level)[4 * i] == byte;
    return ok;
}
static void outs_free(outs* o) {
    free(o->in_view);
    free(o->x);
    free(o->y);
    free(o->xr);
    free(o->vc);
    free(o->level);
}

static int call(const orbm_track_geom* g, float lsf, const float* T, float lim, int n, const float* pos,
                const float* nrm, const float* mind, const float* maxd, outs* o) {
    return orbx_is_in_frustum(g, lsf, T, lim, n, pos, nrm, mind, maxd, o->in_view, o->x, o->y, o->xr, o->level, o->vc);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        printf("usage: test_frustum <tests/golden/frustum_vectors.txt>\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        printf("cannot open %s\n", argv[1]);
        return 2;
    }
    char name[64];
    unsigned u[16], ulsf, ulim;
    int ncases = 0, nin = 0, nout = 0, nlevels = 0, level_seen = 0;
    while (fscanf(f, " case %63s %x %x %x %x %x %x %x %x %x %d %x %x", name, &u[0], &u[1], &u[2], &u[3], &u[4], &u[5],
                  &u[6], &u[7], &u[8], &nlevels, &ulsf, &ulim) == 13) {
        orbm_track_geom g;
        memset(&g, 0, sizeof(g));
        g.fx = fbits(u[0]);
        g.fy = fbits(u[1]);
        g.cx = fbits(u[2]);
        g.cy = fbits(u[3]);
        g.bf = fbits(u[4]);
        g.min_x = fbits(u[5]);
        g.min_y = fbits(u[6]);
        g.max_x = fbits(u[7]);
        g.max_y = fbits(u[8]);
        g.nlevels = nlevels;
        const float lsf = fbits(ulsf), lim = fbits(ulim);
        float T[16];
        if (fscanf(f, " pose %x %x %x %x %x %x %x %x %x %x %x %x %x %x %x %x", &u[0], &u[1], &u[2], &u[3], &u[4], &u[5],
                   &u[6], &u[7], &u[8], &u[9], &u[10], &u[11], &u[12], &u[13], &u[14], &u[15]) != 16)
            break;
        for (int i = 0; i < 16; i++) T[i] = fbits(u[i]);
        int n = 0;
        if (fscanf(f, " points %d", &n) != 1 || n < 1) break;
        float* pos = (float*)malloc(12 * (size_t)n);
        float* nrm = (float*)malloc(12 * (size_t)n);
        float* mind = (float*)malloc(4 * (size_t)n);
        float* maxd = (float*)malloc(4 * (size_t)n);
        unsigned* want = (unsigned*)malloc(sizeof(unsigned) * 4 * (size_t)n);
        int* wview = (int*)malloc(sizeof(int) * (size_t)n);
        int* wlevel = (int*)malloc(sizeof(int) * (size_t)n);
        outs o = outs_alloc(n);
        int got = 0;
        for (int i = 0; i < n; i++) {
            if (fscanf(f, " %x %x %x %x %x %x %x %x %d %x %x %x %d %x", &u[0], &u[1], &u[2], &u[3], &u[4], &u[5], &u[6],
                       &u[7], &wview[i], &u[8], &u[9], &u[10], &wlevel[i], &u[11]) != 14)
                break;
            for (int k = 0; k < 3; k++) {
                pos[3 * i + k] = fbits(u[k]);
                nrm[3 * i + k] = fbits(u[3 + k]);
            }
            mind[i] = fbits(u[6]);
            maxd[i] = fbits(u[7]);
            memcpy(want + 4 * i, u + 8, 16); /* x, y, xr, view_cos */
            got++;
        }
        CHECK(got == n);
        outs_fill(&o, n, 0xA5);
        CHECK(call(&g, lsf, T, lim, n, pos, nrm, mind, maxd, &o) == 0);
        int bad = 0;
        for (int i = 0; i < n; i++) {
            bad += o.in_view[i] != wview[i] || o.level[i] != wlevel[i] || memcmp(o.x + i, want + 4 * i, 4) ||
                   memcmp(o.y + i, want + 4 * i + 1, 4) || memcmp(o.xr + i, want + 4 * i + 2, 4) ||
                   memcmp(o.vc + i, want + 4 * i + 3, 4);
            nin += wview[i];
            nout += !wview[i];
            if (wview[i]) level_seen |= 1 << wlevel[i];
            if (!o.in_view[i]) CHECK(o.x[i] == 0 && o.y[i] == 0 && o.xr[i] == 0 && o.vc[i] == 0 && o.level[i] == 0);
        }
        if (bad) printf("%s case %d: %d points differ\n", name, ncases, bad);
        CHECK(bad == 0);
        /* the contract's exclusions: each rejects its point and leaves the next one alone */
        if (n >= 2) {
            const float keep[3] = {pos[0], nrm[0], maxd[0]};
            const float vals[3] = {NAN, INFINITY, -INFINITY};
            for (int k = 0; k < 3; k++) {
                pos[0] = vals[k];
                CHECK(call(&g, lsf, T, lim, 2, pos, nrm, mind, maxd, &o) == 0 && o.in_view[0] == 0 && o.x[0] == 0);
                CHECK(o.in_view[1] == wview[1] && memcmp(o.x + 1, want + 4, 4) == 0);
                pos[0] = keep[0];
                nrm[0] = vals[k];
                CHECK(call(&g, lsf, T, lim, 2, pos, nrm, mind, maxd, &o) == 0 && o.in_view[0] == 0);
                nrm[0] = keep[1];
                maxd[0] = vals[k];
                CHECK(call(&g, lsf, T, lim, 2, pos, nrm, mind, maxd, &o) == 0 && o.in_view[0] == 0);
                maxd[0] = keep[2];
            }
            float Tn[16];
            memcpy(Tn, T, sizeof(Tn));
            Tn[7] = NAN;
            CHECK(call(&g, lsf, Tn, lim, n, pos, nrm, mind, maxd, &o) == 0);
            for (int i = 0; i < n; i++) CHECK(o.in_view[i] == 0 && o.level[i] == 0);
        }
        /* argument errors write nothing */
        outs_fill(&o, n, 0x11);
        orbm_track_geom gb = g;
        gb.nlevels = 0;
        CHECK(call(NULL, lsf, T, lim, n, pos, nrm, mind, maxd, &o) == ORBX_EARG);
        CHECK(call(&gb, lsf, T, lim, n, pos, nrm, mind, maxd, &o) == ORBX_EARG);
        gb.nlevels = 17;
        CHECK(call(&gb, lsf, T, lim, n, pos, nrm, mind, maxd, &o) == ORBX_EARG);
        CHECK(call(&g, 0.0f, T, lim, n, pos, nrm, mind, maxd, &o) == ORBX_EARG);
        CHECK(call(&g, NAN, T, lim, n, pos, nrm, mind, maxd, &o) == ORBX_EARG);
        CHECK(call(&g, lsf, NULL, lim, n, pos, nrm, mind, maxd, &o) == ORBX_EARG);
        CHECK(call(&g, lsf, T, NAN, n, pos, nrm, mind, maxd, &o) == ORBX_EARG);
        CHECK(call(&g, lsf, T, lim, -1, pos, nrm, mind, maxd, &o) == ORBX_EARG);
        CHECK(call(&g, lsf, T, lim, n, NULL, nrm, mind, maxd, &o) == ORBX_EARG);
        CHECK(call(&g, lsf, T, lim, n, pos, NULL, mind, maxd, &o) == ORBX_EARG);
        CHECK(call(&g, lsf, T, lim, n, pos, nrm, NULL, maxd, &o) == ORBX_EARG);
        CHECK(call(&g, lsf, T, lim, n, pos, nrm, mind, NULL, &o) == ORBX_EARG);
        CHECK(orbx_is_in_frustum(&g, lsf, T, lim, n, pos, nrm, mind, maxd, NULL, o.x, o.y, o.xr, o.level, o.vc) ==
              ORBX_EARG);
        CHECK(orbx_is_in_frustum(&g, lsf, T, lim, n, pos, nrm, mind, maxd, o.in_view, o.x, o.y, o.xr, NULL, o.vc) ==
              ORBX_EARG);
        CHECK(outs_all(&o, n, 0x11));
        /* n == 0 needs no arrays */
        CHECK(orbx_is_in_frustum(&g, lsf, T, lim, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0);
        free(pos);
        free(nrm);
        free(mind);
        free(maxd);
        free(want);
        free(wview);
        free(wlevel);
        outs_free(&o);
        ncases++;
    }
    fclose(f);
    CHECK(ncases == 9);
    CHECK(nin > 60 && nout > 150 && level_seen == 0xFF);
    printf("%d cases, %d points in view, %d rejected\n", ncases, nin, nout);
    if (fails)
        printf("FAILED (%d)\n", fails);
    else
        printf("ALL PASS\n");
    return fails ? 1 : 0;
}
