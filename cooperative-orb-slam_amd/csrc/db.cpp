/*
 * db.cpp -- host side of the keyframe database (orbdb_* of include/orbslam_amd.h): the key -> entry map, the
 * free list and the insertion sequence numbers of KeyFrameDatabase's inverted file (KeyFrameDatabase.cc:40-73),
 * and the sequencing of db_kernels.hip on the caller's stream. The candidate selection is db_select.c.
 */
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "host_util.h"
#include "launch.h"
#include "orb_db.h"

using namespace orbamd;

struct orbdb_handle {
    int device = 0, capacity = 0, stride = 0;
    std::mutex mu;
    struct Entry {
        int slot;
        uint64_t seq;
    };
    std::unordered_map<uint64_t, Entry> by_key;
    std::map<uint64_t, std::pair<uint64_t, int>> by_seq;  // insertion sequence number -> (key, entry index)
    std::vector<int> free_slots;                          // entry indices given back by erase (reused last-freed first)
    int next_slot = 0;                                    // entry indices [next_slot, capacity) were never used
    uint64_t next_seq = 0;
    void* storage = nullptr;  // word | value | count | live | err words | host-query staging and results
    DbDev d{};
    uint32_t* q_word = nullptr;
    double* q_value = nullptr;
    int32_t* q_count = nullptr;
    int32_t* r_ncommon = nullptr;
    float* r_score = nullptr;
    uint32_t* r_first = nullptr;
};

namespace {

/* device storage at first use (orbdb_create needs no device); the caller holds db->mu */
int ensure_storage(orbdb_handle* db) {
    if (db->storage) return 0;
    if (db->device < 0 || db->device >= orbx_device_count()) return ORBX_EDEVICE;
    HIPR(hipSetDevice(db->device));
    const size_t C = (size_t)db->capacity, S = (size_t)db->stride;
    size_t off = 0;
    const size_t o_val = off; off += align_up(8 * C * S, 256);
    const size_t o_word = off; off += align_up(4 * C * S, 256);
    const size_t o_cnt = off; off += align_up(4 * C, 256);
    const size_t o_live = off; off += align_up(4 * C, 256);
    const size_t o_err = off; off += 256;
    const size_t o_qv = off; off += align_up(8 * (size_t)kDbMaxWords, 256);
    const size_t o_qw = off; off += align_up(4 * (size_t)kDbMaxWords, 256);
    const size_t o_qc = off; off += 256;
    const size_t o_rn = off; off += align_up(4 * C, 256);
    const size_t o_rs = off; off += align_up(4 * C, 256);
    const size_t o_rf = off; off += align_up(4 * C, 256);
    void* p = nullptr;
    HIPR(hipMalloc(&p, off));
    uint8_t* b = (uint8_t*)p;
    // count, live and the error words start at zero (one contiguous range)
    if (hipMemset(b + o_cnt, 0, o_qv - o_cnt) != hipSuccess) {
        (void)hipFree(p);
        (void)hipGetLastError();
        return ORBX_EDEVICE;
    }
    db->storage = p;
    db->d.value = (double*)(b + o_val);
    db->d.word = (uint32_t*)(b + o_word);
    db->d.count = (int32_t*)(b + o_cnt);
    db->d.live = (int32_t*)(b + o_live);
    db->d.err = (int32_t*)(b + o_err);
    db->d.capacity = db->capacity;
    db->d.stride = db->stride;
    db->q_value = (double*)(b + o_qv);
    db->q_word = (uint32_t*)(b + o_qw);
    db->q_count = (int32_t*)(b + o_qc);
    db->r_ncommon = (int32_t*)(b + o_rn);
    db->r_score = (float*)(b + o_rs);
    db->r_first = (uint32_t*)(b + o_rf);
    return 0;
}

/* the next entry index and sequence number for `key`; the caller holds db->mu */
int take_slot(orbdb_handle* db, uint64_t key, int* slot) {
    if (db->by_key.count(key)) return ORBX_EARG;
    if (!db->free_slots.empty()) {
        *slot = db->free_slots.back();
        db->free_slots.pop_back();
    } else if (db->next_slot < db->capacity) {
        *slot = db->next_slot++;
    } else {
        return ORBX_ECAPACITY;
    }
    const uint64_t seq = db->next_seq++;
    db->by_key[key] = orbdb_handle::Entry{*slot, seq};
    db->by_seq[seq] = std::make_pair(key, *slot);
    return 0;
}

void drop_key(orbdb_handle* db, uint64_t key) {
    auto it = db->by_key.find(key);
    if (it == db->by_key.end()) return;
    db->free_slots.push_back(it->second.slot);
    db->by_seq.erase(it->second.seq);
    db->by_key.erase(it);
}

}  // namespace

extern "C" {

int orbdb_create(int device, int capacity, int word_stride, int scoring, orbdb_handle** out) {
    if (!out) return ORBX_EARG;
    *out = nullptr;
    if (device < 0 || capacity < 1 || capacity > (1 << 24) || word_stride < 1 || word_stride > kDbMaxWords ||
        scoring != ORBDB_SCORING_L1)
        return ORBX_EARG;
    orbdb_handle* db = new orbdb_handle();
    db->device = device;
    db->capacity = capacity;
    db->stride = word_stride;
    *out = db;
    return 0;
}

void orbdb_destroy(orbdb_handle* db) {
    if (!db) return;
    if (db->storage) {
        (void)hipSetDevice(db->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(db->storage);
        (void)hipGetLastError();
    }
    delete db;
}

int orbdb_add(orbdb_handle* db, uint64_t key, const uint32_t* words, const double* values, int n, void* stream) {
    if (!db || n < 0 || n > db->stride || (n && (!words || !values))) return ORBX_EARG;
    for (int i = 1; i < n; i++)
        if (words[i - 1] >= words[i]) return ORBX_EARG;
    std::lock_guard<std::mutex> lock(db->mu);
    if (db->by_key.count(key)) return ORBX_EARG;
    if (int rc = ensure_storage(db)) return rc;
    HIPR(hipSetDevice(db->device));
    int slot = -1;
    if (int rc = take_slot(db, key, &slot)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t base = (size_t)slot * db->stride;
    hipError_t e = hipSuccess;
    if (n) {
        e = hipMemcpyAsync(db->d.word + base, words, 4 * (size_t)n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(db->d.value + base, values, 8 * (size_t)n, hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess) e = launch_db_mark(db->d, slot, slot + 1, n, 1, st);
    // the caller's arrays are pageable and may go away on return: the copies must have left them
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        drop_key(db, key);
        HIPR(e);
    }
    return 0;
}

int orbdb_add_device(orbdb_handle* db, uint64_t key, const uint32_t* d_words, const double* d_values,
                     const int32_t* d_count, void* stream) {
    if (!db || !d_words || !d_values || !d_count || ((uintptr_t)d_words & 3) || ((uintptr_t)d_values & 7) ||
        ((uintptr_t)d_count & 3))
        return ORBX_EARG;
    std::lock_guard<std::mutex> lock(db->mu);
    if (db->by_key.count(key)) return ORBX_EARG;
    if (int rc = ensure_storage(db)) return rc;
    HIPR(hipSetDevice(db->device));
    int slot = -1;
    if (int rc = take_slot(db, key, &slot)) return rc;
    const hipError_t e = launch_db_add(db->d, slot, d_words, d_values, d_count, (hipStream_t)stream);
    if (e != hipSuccess) {
        drop_key(db, key);
        HIPR(e);
    }
    return 0;
}

int orbdb_erase(orbdb_handle* db, uint64_t key, void* stream) {
    if (!db) return ORBX_EARG;
    std::lock_guard<std::mutex> lock(db->mu);
    auto it = db->by_key.find(key);
    if (it == db->by_key.end()) return 0;
    const int slot = it->second.slot;
    HIPR(hipSetDevice(db->device));
    HIPR(launch_db_mark(db->d, slot, slot + 1, 0, 0, (hipStream_t)stream));
    drop_key(db, key);
    return 0;
}

int orbdb_clear(orbdb_handle* db, void* stream) {
    if (!db) return ORBX_EARG;
    std::lock_guard<std::mutex> lock(db->mu);
    if (db->storage && db->next_slot > 0) {
        HIPR(hipSetDevice(db->device));
        HIPR(launch_db_mark(db->d, 0, db->next_slot, 0, 0, (hipStream_t)stream));
    }
    db->by_key.clear();
    db->by_seq.clear();
    db->free_slots.clear();
    db->next_slot = 0;
    return 0;
}

int orbdb_entries(orbdb_handle* db, int cap, uint64_t* keys, int32_t* slots, int* n) {
    if (!db || !n || cap < 0) return ORBX_EARG;
    std::lock_guard<std::mutex> lock(db->mu);
    *n = (int)db->by_seq.size();
    if (!keys && !slots) return 0;
    if (cap < *n) return ORBX_ECAPACITY;
    int i = 0;
    for (const auto& kv : db->by_seq) {
        if (keys) keys[i] = kv.second.first;
        if (slots) slots[i] = kv.second.second;
        i++;
    }
    return 0;
}

int orbdb_query_device(orbdb_handle* db, int nq, const void* d_words, size_t word_stride_bytes, const void* d_values,
                       size_t value_stride_bytes, const void* d_counts, size_t count_stride_bytes, int32_t* d_ncommon,
                       float* d_score, uint32_t* d_first_word, void* stream) {
    if (!db || nq < 0 || (nq && (!d_words || !d_values || !d_counts || !d_ncommon || !d_score || !d_first_word)) ||
        (((uintptr_t)d_words | word_stride_bytes | (uintptr_t)d_counts | count_stride_bytes) & 3) ||
        (((uintptr_t)d_values | value_stride_bytes) & 7))
        return ORBX_EARG;
    if (nq == 0) return 0;
    std::lock_guard<std::mutex> lock(db->mu);
    if (int rc = ensure_storage(db)) return rc;
    HIPR(hipSetDevice(db->device));
    DbQueries q;
    q.word = (const uint8_t*)d_words, q.value = (const uint8_t*)d_values, q.count = (const uint8_t*)d_counts;
    q.word_bytes = (long long)word_stride_bytes, q.value_bytes = (long long)value_stride_bytes;
    q.count_bytes = (long long)count_stride_bytes;
    HIPR(launch_db_query(db->d, db->next_slot, q, nq, d_ncommon, d_score, d_first_word, (hipStream_t)stream));
    return 0;
}

int orbdb_query(orbdb_handle* db, const uint32_t* words, const double* values, int n, int cap, uint64_t* keys,
                int32_t* ncommon, float* score, uint32_t* first_word, int* nout, void* stream) {
    if (!db || n < 0 || n > kDbMaxWords || (n && (!words || !values)) || cap < 0 || !nout) return ORBX_EARG;
    std::lock_guard<std::mutex> lock(db->mu);
    const int live = (int)db->by_seq.size();
    *nout = live;
    if (cap < live) return ORBX_ECAPACITY;
    if (live == 0) return 0;
    if (int rc = ensure_storage(db)) return rc;
    HIPR(hipSetDevice(db->device));
    hipStream_t st = (hipStream_t)stream;
    const int32_t cnt = n;
    if (n) {
        HIPR(hipMemcpyAsync(db->q_word, words, 4 * (size_t)n, hipMemcpyHostToDevice, st));
        HIPR(hipMemcpyAsync(db->q_value, values, 8 * (size_t)n, hipMemcpyHostToDevice, st));
    }
    HIPR(hipMemcpyAsync(db->q_count, &cnt, 4, hipMemcpyHostToDevice, st));
    DbQueries q;
    q.word = (const uint8_t*)db->q_word, q.value = (const uint8_t*)db->q_value, q.count = (const uint8_t*)db->q_count;
    q.word_bytes = q.value_bytes = q.count_bytes = 0;
    const int ne = db->next_slot;
    HIPR(launch_db_query(db->d, ne, q, 1, db->r_ncommon, db->r_score, db->r_first, st));
    std::vector<int32_t> rn(ne);
    std::vector<float> rs(ne);
    std::vector<uint32_t> rf(ne);
    HIPR(hipMemcpyAsync(rn.data(), db->r_ncommon, 4 * (size_t)ne, hipMemcpyDeviceToHost, st));
    HIPR(hipMemcpyAsync(rs.data(), db->r_score, 4 * (size_t)ne, hipMemcpyDeviceToHost, st));
    HIPR(hipMemcpyAsync(rf.data(), db->r_first, 4 * (size_t)ne, hipMemcpyDeviceToHost, st));
    HIPR(hipStreamSynchronize(st));
    int i = 0;
    for (const auto& kv : db->by_seq) {
        const int slot = kv.second.second;
        if (keys) keys[i] = kv.second.first;
        if (ncommon) ncommon[i] = rn[slot];
        if (score) score[i] = rs[slot];
        if (first_word) first_word[i] = rf[slot];
        i++;
    }
    return 0;
}

int orbdb_check_error(orbdb_handle* db, void* stream) {
    if (!db) return ORBX_EARG;
    std::lock_guard<std::mutex> lock(db->mu);
    if (!db->storage) return 0;
    HIPR(hipSetDevice(db->device));
    // atomic read-and-clear on the device (word 0 -> word 8)
    int flag = 0;
    HIPR(launch_flag_take(db->d.err, db->d.err + 8, (hipStream_t)stream));
    HIPR(hipMemcpyAsync(&flag, db->d.err + 8, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPR(hipStreamSynchronize((hipStream_t)stream));
    return flag ? ORBX_EDEVICE : 0;
}

}  // extern "C"
