/*
 * host_util.h -- shared by the host side of the C ABI (include/orbslam_amd.h), one unit per subsystem: extract.cpp,
 * stereo.cpp, matcher.cpp, slots.cpp, projection.cpp, vocabulary.cpp, db.cpp, comm.cpp.
 *
 * The host side owns the per-handle device state, builds the geometry tables once per frame size with
 * the reference's exact float semantics (ORBextractor.cc:410-470, 765-787, 1107-1112 and
 * OpenCV 3.x resize coefficients), and sequences the gfx950 kernels on a HIP stream.
 * There is no CPU fallback: every compute entry point fails with ORBX_EDEVICE when the
 * device path is unavailable.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/orbslam_amd.h"

/* A failing HIP call is reported once, through the entry point's status (ORBX_EDEVICE), and then cleared from the
 * calling thread's HIP error state: hipGetLastError returns the last error of ANY runtime call on the thread, so a
 * failure left there would be raised again by the caller's next launch check, far from its cause (round 5's first GPU
 * run: hipEventElapsedTime over a never-recorded stage event pair in orbx_profile_read, whose status bench.py did not
 * read, surfaced as "HIP error: invalid resource handle" in torch's dist.barrier; tests/test_gpu_cache.py
 * ::test_library_hip_failure_does_not_leak pins this). */
#define HIPR(expr)                                                                    \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) {                                                       \
            if (getenv("ORBX_DEBUG")) fprintf(stderr, "HIP error %s at %s:%d\n",     \
                                              hipGetErrorString(e_), __FILE__, __LINE__); \
            (void)hipGetLastError();                                                  \
            return ORBX_EDEVICE;                                                      \
        }                                                                             \
    } while (0)

namespace orbamd {

inline long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        if (hipMalloc(&p, need) != hipSuccess) { p = nullptr; return ORBX_EDEVICE; }
        bytes = need;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T* as() const { return (T*)p; }
};

/* bump allocator over the ctx scratch buffer (sizes first, then carve) */
struct Carve {
    size_t off = 0;
    size_t take(size_t b) { size_t o = off; off += align_up((long long)b, 256); return o; }
};

/* Wait for a per-call matcher launch: its last workgroup stores the match count (>= 0; the host
 * pre-filled it with -1) into pinned host memory last, with release at system scope (match_kernels.hip
 * call_tail), so polling that word ends the call ~5 us sooner than hipStreamSynchronize
 * (tools/latency_floor.hip, profiles/r03_latency_floor.jsonl). The launch needs no further wait: the
 * next call's copies and launches are ordered behind it on the stream. A stream that drains without
 * the word, or an error, is ORBX_EDEVICE. */
template <class Ready>
int wait_until(hipStream_t st, Ready ready) {
    {
        // spin (with a pause) for the first ~200 us, which covers a call that is not queued behind other GPU
        // work; after that yield the core to the other SLAM threads between polls instead of burning it
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 1;; spins++) {
            if (ready()) return 0;
            const bool late = (spins & 255) == 0 &&
                              std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200);
            if (late || (spins & 1023) == 0) {
                const hipError_t e = hipStreamQuery(st);
                if (e != hipErrorNotReady) {
                    if (e != hipSuccess) return ORBX_EDEVICE;
                    break;  // drained: the words are visible now if the kernel wrote them
                }
                if (late) {
                    sched_yield();
                    spins = 0;  // next check after another 256 polls
                }
            } else {
                __builtin_ia32_pause();
            }
        }
    }
    HIPR(hipStreamSynchronize(st));
    return ready() ? 0 : ORBX_EDEVICE;
}

}  // namespace orbamd
