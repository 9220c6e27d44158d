/*
 * test_pose_optimize.c -- the host unit of Optimizer::PoseOptimization (csrc/pose_optimize.c) over the vectors that the
 * Python restatement recorded (tests/golden/pose_vectors.txt): pose, outlier bytes, inlier count, status and diag as
 * raw bits, the untouched bytes of features without a MapPoint, and the argument checks. Stand-alone: its own main, no
 * library, no device; build_pose_optimize.sh also builds it under ASan + UBSan.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "orbslam_amd.h"

static int fails;
#define CHECK(c, ...)                 \
    do {                              \
        if (!(c)) {                   \
            fails++;                  \
            printf("FAIL " __VA_ARGS__); \
            printf("\n");             \
        }                             \
    } while (0)

static float hexf(FILE* f) {
    unsigned u = 0;
    float v;
    if (fscanf(f, "%x", &u) != 1) {
        printf("short file\n");
        exit(2);
    }
    memcpy(&v, &u, 4);
    return v;
}

static int rdint(FILE* f) {
    int v = 0;
    if (fscanf(f, "%d", &v) != 1) {
        printf("short file\n");
        exit(2);
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    const int nscenes = rdint(f);
    for (int sc = 0; sc < nscenes; sc++) {
        char word[16];
        if (fscanf(f, "%15s", word) != 1 || strcmp(word, "scene")) return 2;
        const int n = rdint(f), M = rdint(f), nlevels = rdint(f);
        orbm_track_geom g;
        memset(&g, 0, sizeof(g));
        g.fx = hexf(f), g.fy = hexf(f), g.cx = hexf(f), g.cy = hexf(f), g.bf = hexf(f);
        g.nlevels = nlevels;
        float inv[16] = {0}, T0[16], T[16], Tref[16];
        for (int k = 0; k < nlevels; k++) inv[k] = hexf(f);
        for (int k = 0; k < 16; k++) T0[k] = hexf(f);
        orbx_kp* kps = calloc((size_t)n + 1, sizeof(orbx_kp));
        float* ur = calloc((size_t)n + 1, sizeof(float));
        int32_t* mp = calloc((size_t)n + 1, sizeof(int32_t));
        uint8_t* out = calloc((size_t)n + 1, 1);
        uint8_t* oref = calloc((size_t)n + 1, 1);
        float* pos = calloc((size_t)M * 3 + 1, sizeof(float));
        int any_mono_only = 1;
        for (int i = 0; i < n; i++) {
            kps[i].x = hexf(f);
            kps[i].y = hexf(f);
            kps[i].octave = rdint(f);
            ur[i] = hexf(f);
            mp[i] = rdint(f);
            if (ur[i] >= 0) any_mono_only = 0;
        }
        for (int k = 0; k < 3 * M; k++) pos[k] = hexf(f);
        for (int k = 0; k < 16; k++) Tref[k] = hexf(f);
        if (n == 0) {
            if (fscanf(f, "%15s", word) != 1) return 2;
        }
        for (int i = 0; i < n; i++) oref[i] = (uint8_t)rdint(f);
        const int ninl_ref = rdint(f), st_ref = rdint(f);
        int32_t dref[8], diag[8], ninl = -1, st = -1;
        for (int k = 0; k < 8; k++) dref[k] = rdint(f);
        /* features without a MapPoint keep the byte they came in with */
        for (int i = 0; i < n; i++) out[i] = mp[i] < 0 ? 0xA5 : 0x5A;
        memcpy(T, T0, sizeof(T));
        int rc = orbx_pose_optimization(&g, inv, nlevels, T, n, kps, ur, mp, pos, out, &ninl, &st, diag);
        CHECK(rc == 0, "scene %d rc %d", sc, rc);
        CHECK(!memcmp(T, Tref, sizeof(T)), "scene %d pose", sc);
        CHECK(ninl == ninl_ref && st == st_ref, "scene %d ninliers %d/%d status %d/%d", sc, ninl, ninl_ref, st, st_ref);
        CHECK(!memcmp(diag, dref, sizeof(diag)), "scene %d diag", sc);
        for (int i = 0; i < n; i++)
            CHECK(out[i] == (mp[i] < 0 ? 0xA5 : oref[i]), "scene %d outlier %d: %d", sc, i, out[i]);
        if (any_mono_only) { /* uright == NULL is all monocular */
            memcpy(T, T0, sizeof(T));
            rc = orbx_pose_optimization(&g, inv, nlevels, T, n, kps, NULL, mp, pos, out, &ninl, &st, NULL);
            CHECK(rc == 0 && !memcmp(T, Tref, sizeof(T)) && ninl == ninl_ref, "scene %d without uright", sc);
        }
        /* argument errors: nothing is written */
        memcpy(T, T0, sizeof(T));
        ninl = st = -7;
        CHECK(orbx_pose_optimization(NULL, inv, nlevels, T, n, kps, ur, mp, pos, out, &ninl, &st, diag) == ORBX_EARG, "geom");
        CHECK(orbx_pose_optimization(&g, NULL, nlevels, T, n, kps, ur, mp, pos, out, &ninl, &st, diag) == ORBX_EARG, "inv");
        CHECK(orbx_pose_optimization(&g, inv, 0, T, n, kps, ur, mp, pos, out, &ninl, &st, diag) == ORBX_EARG, "nlevels 0");
        CHECK(orbx_pose_optimization(&g, inv, 17, T, n, kps, ur, mp, pos, out, &ninl, &st, diag) == ORBX_EARG, "nlevels 17");
        CHECK(orbx_pose_optimization(&g, inv, nlevels, NULL, n, kps, ur, mp, pos, out, &ninl, &st, diag) == ORBX_EARG, "Tcw");
        CHECK(orbx_pose_optimization(&g, inv, nlevels, T, -1, kps, ur, mp, pos, out, &ninl, &st, diag) == ORBX_EARG, "n");
        CHECK(orbx_pose_optimization(&g, inv, nlevels, T, n, kps, ur, mp, pos, out, NULL, &st, diag) == ORBX_EARG, "ninl");
        CHECK(orbx_pose_optimization(&g, inv, nlevels, T, n, kps, ur, mp, pos, out, &ninl, NULL, diag) == ORBX_EARG, "st");
        if (n) {
            CHECK(orbx_pose_optimization(&g, inv, nlevels, T, n, NULL, ur, mp, pos, out, &ninl, &st, diag) == ORBX_EARG, "kps");
            CHECK(orbx_pose_optimization(&g, inv, nlevels, T, n, kps, ur, NULL, pos, out, &ninl, &st, diag) == ORBX_EARG, "mp");
            CHECK(orbx_pose_optimization(&g, inv, nlevels, T, n, kps, ur, mp, NULL, out, &ninl, &st, diag) == ORBX_EARG, "pos");
            CHECK(orbx_pose_optimization(&g, inv, nlevels, T, n, kps, ur, mp, pos, NULL, &ninl, &st, diag) == ORBX_EARG, "out");
        }
        CHECK(!memcmp(T, T0, sizeof(T)) && ninl == -7 && st == -7, "scene %d: an argument error wrote", sc);
        free(kps), free(ur), free(mp), free(out), free(oref), free(pos);
    }
    fclose(f);
    printf(fails ? "%d FAILED\n" : "ALL PASS (%d scenes)\n", fails ? fails : nscenes);
    return fails ? 1 : 0;
}
