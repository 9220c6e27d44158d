/* test_unproject.c -- the host unit of Frame::UnprojectStereo (csrc/unproject.c, orbx_unproject_stereo) over the
 * vectors the Python restatement wrote (tests/golden/unproject_vectors.txt, tests/unproject_py.py), bit for bit, with
 * its argument checks. Plain C with its own main: built once normally and once under ASan + UBSan
 * (tests/cpp/build_unproject.sh), from this file and csrc/unproject.c alone, no library.
 *   test_unproject <fixture> */
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

int main(int argc, char** argv) {
    if (argc < 2) {
        printf("usage: test_unproject <tests/golden/unproject_vectors.txt>\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        printf("cannot open %s\n", argv[1]);
        return 2;
    }
    char name[64];
    unsigned u[16];
    int ncases = 0, nvalid = 0, ninvalid = 0, nidentity = 0;
    while (fscanf(f, " case %63s %x %x %x %x", name, &u[0], &u[1], &u[2], &u[3]) == 5) {
        orbx_camera cam;
        memset(&cam, 0, sizeof(cam));
        cam.fx = fbits(u[0]);
        cam.fy = fbits(u[1]);
        cam.cx = fbits(u[2]);
        cam.cy = fbits(u[3]);
        cam.k1 = 0.5f; /* not read */
        float T[16];
        if (fscanf(f, " pose %x %x %x %x %x %x %x %x %x %x %x %x %x %x %x %x", &u[0], &u[1], &u[2], &u[3], &u[4], &u[5],
                   &u[6], &u[7], &u[8], &u[9], &u[10], &u[11], &u[12], &u[13], &u[14], &u[15]) != 16)
            break;
        for (int i = 0; i < 16; i++) T[i] = fbits(u[i]);
        int n = 0;
        if (fscanf(f, " points %d", &n) != 1 || n < 1) break;
        /* exact-size heap arrays: an access past row n - 1 is the sanitizer's to see */
        orbx_kp* kps = (orbx_kp*)calloc((size_t)n, sizeof(orbx_kp));
        float* depth = (float*)malloc(sizeof(float) * (size_t)n);
        unsigned* want = (unsigned*)malloc(sizeof(unsigned) * 3 * (size_t)n);
        int* wvalid = (int*)malloc(sizeof(int) * (size_t)n);
        float* pos = (float*)malloc(sizeof(float) * 3 * (size_t)n);
        uint8_t* valid = (uint8_t*)malloc((size_t)n);
        int got = 0;
        for (int i = 0; i < n; i++) {
            if (fscanf(f, " %x %x %x %d %x %x %x", &u[0], &u[1], &u[2], &wvalid[i], &u[3], &u[4], &u[5]) != 7) break;
            kps[i].x = fbits(u[0]);
            kps[i].y = fbits(u[1]);
            kps[i].octave = i % 8;
            depth[i] = fbits(u[2]);
            memcpy(want + 3 * i, u + 3, 12);
            got++;
        }
        CHECK(got == n);
        memset(pos, 0xA5, sizeof(float) * 3 * (size_t)n);
        memset(valid, 0xA5, (size_t)n);
        CHECK(orbx_unproject_stereo(&cam, T, n, kps, depth, pos, valid) == 0);
        int bad = 0;
        for (int i = 0; i < n; i++) {
            bad += memcmp(pos + 3 * i, want + 3 * i, 12) != 0 || valid[i] != wvalid[i];
            nvalid += wvalid[i];
            ninvalid += !wvalid[i];
        }
        if (bad) printf("%s case %d: %d points differ\n", name, ncases, bad);
        CHECK(bad == 0);
        /* valid may be NULL; the positions are the same */
        memset(pos, 0x5A, sizeof(float) * 3 * (size_t)n);
        CHECK(orbx_unproject_stereo(&cam, T, n, kps, depth, pos, NULL) == 0);
        CHECK(memcmp(pos, want, sizeof(float) * 3 * (size_t)n) == 0);
        /* the identity pose: pos = ((u - cx) z invfx, (v - cy) z invfy, z) */
        int ident = 1;
        for (int i = 0; i < 16; i++) ident &= T[i] == (i % 5 == 0 ? 1.0f : 0.0f);
        if (ident) {
            nidentity++;
            const float invfx = 1.0f / cam.fx, invfy = 1.0f / cam.fy;
            for (int i = 0; i < n; i++)
                if (valid[i] || wvalid[i]) {
                    const float x = (kps[i].x - cam.cx) * depth[i] * invfx, y = (kps[i].y - cam.cy) * depth[i] * invfy;
                    CHECK(pos[3 * i] == x && pos[3 * i + 1] == y && pos[3 * i + 2] == depth[i]);
                }
        }
        /* argument errors write nothing */
        memset(pos, 0x11, sizeof(float) * 3 * (size_t)n);
        memset(valid, 0x11, (size_t)n);
        orbx_camera zero = cam;
        zero.fx = 0;
        CHECK(orbx_unproject_stereo(NULL, T, n, kps, depth, pos, valid) == ORBX_EARG);
        CHECK(orbx_unproject_stereo(&zero, T, n, kps, depth, pos, valid) == ORBX_EARG);
        zero = cam;
        zero.fy = 0;
        CHECK(orbx_unproject_stereo(&zero, T, n, kps, depth, pos, valid) == ORBX_EARG);
        CHECK(orbx_unproject_stereo(&cam, NULL, n, kps, depth, pos, valid) == ORBX_EARG);
        CHECK(orbx_unproject_stereo(&cam, T, -1, kps, depth, pos, valid) == ORBX_EARG);
        CHECK(orbx_unproject_stereo(&cam, T, n, NULL, depth, pos, valid) == ORBX_EARG);
        CHECK(orbx_unproject_stereo(&cam, T, n, kps, NULL, pos, valid) == ORBX_EARG);
        CHECK(orbx_unproject_stereo(&cam, T, n, kps, depth, NULL, valid) == ORBX_EARG);
        for (int i = 0; i < n; i++) CHECK(valid[i] == 0x11 && ((unsigned char*)pos)[12 * i] == 0x11);
        /* n == 0 needs no arrays */
        CHECK(orbx_unproject_stereo(&cam, T, 0, NULL, NULL, NULL, NULL) == 0);
        free(kps);
        free(depth);
        free(want);
        free(wvalid);
        free(pos);
        free(valid);
        ncases++;
    }
    fclose(f);
    CHECK(ncases == 9 && nidentity == 3);
    CHECK(nvalid > 100 && ninvalid > 20);
    printf("%d cases, %d points, %d without depth\n", ncases, nvalid + ninvalid, ninvalid);
    if (fails)
        printf("FAILED (%d)\n", fails);
    else
        printf("ALL PASS\n");
    return fails ? 1 : 0;
}
