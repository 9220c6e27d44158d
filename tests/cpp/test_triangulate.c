/* test_triangulate.c -- the host unit of CreateNewMapPoints' per-match loop (csrc/triangulate.c) as a stand-alone C
 * program over the vectors the Python restatement wrote (tests/golden/triangulate_vectors.txt): every status, position
 * and table row as raw bits, the table's order and descriptors, nothing written past n1 rows (the buffers are exactly
 * that long, so the sanitizer build sees an overrun), and the argument checks. No GPU, no library.
 * Usage: test_triangulate <vectors>; prints ALL PASS and exits 0, or the first differences and exits 1. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "orbslam_amd.h"

static int fails = 0;
#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            if (fails++ < 20) {           \
                printf("FAIL: ");         \
                printf(__VA_ARGS__);      \
                printf("\n");             \
            }                             \
        }                                 \
    } while (0)

static float rdf(FILE* f) {
    uint32_t u = 0;
    float v;
    if (fscanf(f, "%x", &u) != 1) {
        printf("FAIL: short file\n");
        exit(1);
    }
    memcpy(&v, &u, 4);
    return v;
}
static int rdi(FILE* f) {
    int v = 0;
    if (fscanf(f, "%d", &v) != 1) {
        printf("FAIL: short file\n");
        exit(1);
    }
    return v;
}
static int same(const float* a, const float* b, int n) { return memcmp(a, b, 4 * (size_t)n) == 0; }
static void* buf(size_t n) { return malloc(n ? n : 1); }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char tag[64], name[64];
    int npairs = 0, created = 0;
    while (fscanf(f, "%63s", tag) == 1) {
        if (strcmp(tag, "pair")) {
            printf("FAIL: expected pair, got %s\n", tag);
            return 1;
        }
        if (fscanf(f, "%63s", name) != 1) return 1;
        const int mono = rdi(f);
        const float med = rdf(f);
        const int n1 = rdi(f), n2 = rdi(f), nnew = rdi(f);
        orbm_tri_geom g;
        memset(&g, 0, sizeof(g));
        float T1[16], T2[16];
        if (fscanf(f, "%63s", tag) != 1) return 1;
        g.fx = rdf(f), g.fy = rdf(f), g.cx = rdf(f), g.cy = rdf(f), g.bf = rdf(f), g.b = rdf(f);
        g.nlevels = rdi(f);
        for (int i = 0; i < 16; i++) g.scale_factors[i] = rdf(f);
        for (int i = 0; i < 16; i++) g.level_sigma2[i] = rdf(f);
        if (fscanf(f, "%63s", tag) != 1) return 1;
        for (int i = 0; i < 16; i++) T1[i] = rdf(f);
        if (fscanf(f, "%63s", tag) != 1) return 1;
        for (int i = 0; i < 16; i++) T2[i] = rdf(f);
        orbx_kp* k1 = buf(sizeof(orbx_kp) * n1);
        orbx_kp* k2 = buf(sizeof(orbx_kp) * n2);
        float *ur1 = buf(4 * n1), *d1 = buf(4 * n1), *ur2 = buf(4 * n2), *d2 = buf(4 * n2);
        int32_t* m = buf(4 * n1);
        int8_t* want_st = buf(n1);
        float* want_pos = buf(12 * n1);
        uint8_t* desc = buf(32 * (size_t)n1);
        memset(k1, 0, sizeof(orbx_kp) * n1);
        memset(k2, 0, sizeof(orbx_kp) * n2);
        for (int i = 0; i < n1; i++) {
            k1[i].x = rdf(f), k1[i].y = rdf(f), k1[i].octave = rdi(f);
            ur1[i] = rdf(f), d1[i] = rdf(f);
            m[i] = rdi(f);
            want_st[i] = (int8_t)rdi(f);
            for (int k = 0; k < 3; k++) want_pos[3 * i + k] = rdf(f);
            for (int b = 0; b < 32; b++) desc[32 * i + b] = (uint8_t)(i * 7 + b * 3 + 1);
        }
        for (int i = 0; i < n2; i++) {
            k2[i].x = rdf(f), k2[i].y = rdf(f), k2[i].octave = rdi(f);
            ur2[i] = rdf(f), d2[i] = rdf(f);
        }
        float *wp = buf(12 * nnew), *wn = buf(12 * nnew), *wmin = buf(4 * nnew), *wmax = buf(4 * nnew);
        int32_t *wf1 = buf(4 * nnew), *wf2 = buf(4 * nnew);
        for (int j = 0; j < nnew; j++) {
            for (int k = 0; k < 3; k++) wp[3 * j + k] = rdf(f);
            for (int k = 0; k < 3; k++) wn[3 * j + k] = rdf(f);
            wmin[j] = rdf(f), wmax[j] = rdf(f);
            wf1[j] = rdi(f), wf2[j] = rdi(f);
        }
        int8_t* st = buf(n1);
        float *pos = buf(12 * n1), *tp = buf(12 * n1), *tn = buf(12 * n1), *tmin = buf(4 * n1), *tmax = buf(4 * n1);
        uint8_t *td = buf(32 * (size_t)n1), *tf = buf(n1);
        int32_t *f1 = buf(4 * n1), *f2 = buf(4 * n1);
        int32_t nn = -1;
        const int rc = orbx_triangulate_matches(&g, mono, med, T1, T2, n1, k1, ur1, d1, desc, n2, k2, ur2, d2, m, st,
                                                pos, tp, tn, tmin, tmax, td, tf, f1, f2, &nn);
        CHECK(rc == 0, "%s: rc %d", name, rc);
        CHECK(nn == nnew, "%s: nnew %d, want %d", name, nn, nnew);
        for (int i = 0; i < n1; i++) {
            CHECK(st[i] == want_st[i], "%s row %d: status %d, want %d", name, i, st[i], want_st[i]);
            CHECK(same(pos + 3 * i, want_pos + 3 * i, 3), "%s row %d: pos3", name, i);
        }
        for (int j = 0; j < nn && j < nnew; j++) {
            CHECK(same(tp + 3 * j, wp + 3 * j, 3) && same(tn + 3 * j, wn + 3 * j, 3), "%s table %d: pos / normal", name, j);
            CHECK(same(tmin + j, wmin + j, 1) && same(tmax + j, wmax + j, 1), "%s table %d: distances", name, j);
            CHECK(f1[j] == wf1[j] && f2[j] == wf2[j] && tf[j] == 9, "%s table %d: features / flags", name, j);
            CHECK(j == 0 || f1[j] > f1[j - 1], "%s table %d: order", name, j);
            CHECK(f1[j] >= 0 && f1[j] < n1 && !memcmp(td + 32 * j, desc + 32 * f1[j], 32), "%s table %d: desc", name, j);
        }
        /* monocular arrays as NULL give the same as all -1 when there is no mvuRight */
        int all_mono = 1;
        for (int i = 0; i < n1; i++) all_mono &= ur1[i] < 0;
        for (int i = 0; i < n2; i++) all_mono &= ur2[i] < 0;
        if (all_mono) {
            int8_t* st2 = buf(n1);
            int32_t nn2 = -1;
            orbx_triangulate_matches(&g, mono, med, T1, T2, n1, k1, NULL, NULL, desc, n2, k2, NULL, NULL, m, st2, pos, tp,
                                     tn, tmin, tmax, td, tf, f1, f2, &nn2);
            CHECK(nn2 == nn && !memcmp(st, st2, n1), "%s: NULL mvuRight differs from all -1", name);
            free(st2);
        }
        /* argument checks: nothing is written */
        int32_t keep = 1234;
        CHECK(orbx_triangulate_matches(NULL, mono, med, T1, T2, n1, k1, ur1, d1, desc, n2, k2, ur2, d2, m, st, pos, tp, tn,
                                       tmin, tmax, td, tf, f1, f2, &keep) == ORBX_EARG && keep == 1234, "NULL geom");
        CHECK(orbx_triangulate_matches(&g, mono, med, T1, T2, -1, k1, ur1, d1, desc, n2, k2, ur2, d2, m, st, pos, tp, tn,
                                       tmin, tmax, td, tf, f1, f2, &keep) == ORBX_EARG && keep == 1234, "n1 < 0");
        orbm_tri_geom bad = g;
        bad.nlevels = 17;
        CHECK(orbx_triangulate_matches(&bad, mono, med, T1, T2, n1, k1, ur1, d1, desc, n2, k2, ur2, d2, m, st, pos, tp,
                                       tn, tmin, tmax, td, tf, f1, f2, &keep) == ORBX_EARG && keep == 1234, "nlevels");
        created += nn;
        npairs++;
        free(k1), free(k2), free(ur1), free(d1), free(ur2), free(d2), free(m), free(want_st), free(want_pos), free(desc);
        free(wp), free(wn), free(wmin), free(wmax), free(wf1), free(wf2);
        free(st), free(pos), free(tp), free(tn), free(tmin), free(tmax), free(td), free(tf), free(f1), free(f2);
    }
    fclose(f);
    CHECK(npairs == 6 && created > 30, "pairs %d, created %d", npairs, created);
    printf("%d pairs, %d new points\n", npairs, created);
    if (fails) {
        printf("%d FAILURES\n", fails);
        return 1;
    }
    printf("ALL PASS\n");
    return 0;
}
