/*
 * orb_db.h -- device view of the keyframe database (db_kernels.hip, db.cpp).
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orbamd {

constexpr int kDbMaxWords = 4096;  // words of one BowVector (the transform's limit, orb_bow.h): query staging in LDS

/* fixed-stride entry storage: entry e's words at word[e * stride], values at value[e * stride] */
struct DbDev {
    uint32_t* word;
    double* value;
    int32_t* count;  // [capacity] BowVector entries of entry e (0 for a rejected add)
    int32_t* live;   // [capacity] 1 while the entry is in the database
    int32_t* err;    // sticky error word (orbdb_check_error)
    int capacity, stride;
};

/* queries addressed in place: query q's words at word + q * word_bytes and so on (byte strides) */
struct DbQueries {
    const uint8_t* word;
    const uint8_t* value;
    const uint8_t* count;
    long long word_bytes, value_bytes, count_bytes;
};

hipError_t launch_db_add(const DbDev& db, int entry, const uint32_t* word, const double* value, const int32_t* count,
                         hipStream_t st);
/* entries [e0, e1): count and live flag set (erase, clear, the host add) */
hipError_t launch_db_mark(const DbDev& db, int e0, int e1, int count, int live, hipStream_t st);
/* entries [0, nentries) x nq queries -> ncommon / score / first_word at [q * capacity + e] */
hipError_t launch_db_query(const DbDev& db, int nentries, const DbQueries& q, int nq, int32_t* ncommon, float* score,
                           uint32_t* first_word, hipStream_t st);

}  // namespace orbamd
