"""KeyFrameDatabase -- the BoW scoring and candidate selection of ORB_SLAM2::KeyFrameDatabase
(KeyFrameDatabase.cc:33-309) over the C ABI (orbdb_*).

The BowVectors of the keyframes stay in HBM; one query scores a BowVector against all of them
(DBoW2 L1Scoring::score restated, parity unpinned) and returns per keyframe the common-word count
(mnLoopWords / mnRelocWords), the score and the smallest common word (the keyframe's place in
lKFsSharingWords). DetectLoopCandidates / DetectRelocalizationCandidates' selection runs on the
host over those arrays (orbdb_select_candidates). Keyframes are identified by integer keys.
"""
import ctypes as C

import numpy as np

from ._lib import ORBX_EDEVICE, ORBX_OK, check, load

L1_NORM = 0
MODE_LOOP, MODE_RELOC = 0, 1
MAX_WORDS = 4096
_HDR_NBOW, _HDR_OFF = 16, 32  # byte offsets of orbx_slot_header.nbow / .off[]
_SEC_BOWWORD, _SEC_BOWVALUE = 7, 8


def _ptr(a):
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    if isinstance(a, int):
        return a
    return a.ctypes.data


def select_candidates(mode, ncommon, score, first_word, neighbours, last_score, connected=None, min_score=0.0):
    """orbdb_select_candidates over entries in insertion order. neighbours[i] = entry indices of entry i's
    GetBestCovisibilityKeyFrames(10) (-1 = not in the database); last_score (float32 array) is updated in place.
    Returns the candidates' entry indices in the reference's order."""
    n = len(ncommon)
    ncommon = np.ascontiguousarray(ncommon, np.int32)
    score = np.ascontiguousarray(score, np.float32)
    first_word = np.ascontiguousarray(first_word, np.uint32)
    if not (isinstance(last_score, np.ndarray) and last_score.dtype == np.float32 and last_score.flags.c_contiguous
            and len(last_score) == n):
        raise ValueError("last_score must be a contiguous float32 array with one value per entry")
    off = np.zeros(n + 1, np.int32)
    for i in range(n):
        off[i + 1] = off[i] + len(neighbours[i])
    flat = np.array([j for nb in neighbours for j in nb] or [0], np.int32)
    conn = None if connected is None else np.ascontiguousarray(connected, np.uint8)
    out = np.zeros(max(n, 1), np.int32)
    nout = C.c_int()
    check(load().orbdb_select_candidates(int(mode), n, _ptr(ncommon), _ptr(score), _ptr(first_word), _ptr(conn),
                                         _ptr(off), _ptr(flat), float(min_score), _ptr(last_score), _ptr(out),
                                         C.byref(nout)), "orbdb_select_candidates")
    return out[:nout.value].tolist()


class KeyFrameDatabase:
    """ORB_SLAM2::KeyFrameDatabase with device-resident BowVectors.

    mLoopScore / mRelocScore of the reference's KeyFrames are kept per key in loop_score / reloc_score; they
    outlive erase, as the KeyFrame members do."""

    def __init__(self, capacity, word_stride=MAX_WORDS, device=0, scoring=L1_NORM):
        self._lib = load()
        h = C.c_void_p()
        check(self._lib.orbdb_create(int(device), int(capacity), int(word_stride), int(scoring), C.byref(h)),
              "orbdb_create")
        self._h = h
        self.capacity, self.word_stride, self.device = int(capacity), int(word_stride), int(device)
        self.loop_score, self.reloc_score = {}, {}
        self.last = None  # (keys, ncommon, score, first_word) of the last detect_* call

    # -- entries ---------------------------------------------------------------------------------
    def add(self, key, words, values, stream=None):
        w = np.ascontiguousarray(words, np.uint32)
        v = np.ascontiguousarray(values, np.float64)
        if len(w) != len(v):
            raise ValueError("words and values differ in length")
        check(self._lib.orbdb_add(self._h, int(key), _ptr(w), _ptr(v), len(w), stream), "orbdb_add")

    def add_device(self, key, d_words, d_values, d_count, stream=None):
        """d_words (uint32) / d_values (float64) / d_count (int32): device tensors or raw device addresses."""
        check(self._lib.orbdb_add_device(self._h, int(key), _ptr(d_words), _ptr(d_values), _ptr(d_count), stream),
              "orbdb_add_device")

    def _slot_sections(self, all_slots, cap):
        if cap is None:
            hdr = all_slots[:80].cpu().numpy().view(np.uint32)
            return int(hdr[8 + _SEC_BOWWORD]), int(hdr[8 + _SEC_BOWVALUE])
        from .exchange import layout
        off, _ = layout(cap)
        return off[_SEC_BOWWORD], off[_SEC_BOWVALUE]

    def add_slots_device(self, all_slots, slot_bytes, keys, cap=None, stream=None):
        """One entry per slot of an all-gather receive buffer (uint8 device tensor of len(keys) slots), filled in
        place from the slot's BOWWORD / BOWVALUE sections and header nbow. cap = the slots' capacity (read from
        the first slot's header when omitted)."""
        ow, ov = self._slot_sections(all_slots, cap)
        base = _ptr(all_slots)
        for i, k in enumerate(keys):
            b = base + i * int(slot_bytes)
            self.add_device(k, b + ow, b + ov, b + _HDR_NBOW, stream)

    def erase(self, key, stream=None):
        check(self._lib.orbdb_erase(self._h, int(key), stream), "orbdb_erase")

    def clear(self, stream=None):
        check(self._lib.orbdb_clear(self._h, stream), "orbdb_clear")

    def entries(self):
        """(keys uint64, entry indices int32) of the live entries in insertion order."""
        n = C.c_int()
        check(self._lib.orbdb_entries(self._h, 0, None, None, C.byref(n)), "orbdb_entries")
        keys = np.zeros(max(n.value, 1), np.uint64)
        slots = np.zeros(max(n.value, 1), np.int32)
        check(self._lib.orbdb_entries(self._h, len(keys), _ptr(keys), _ptr(slots), C.byref(n)), "orbdb_entries")
        return keys[:n.value], slots[:n.value]

    def __len__(self):
        n = C.c_int()
        check(self._lib.orbdb_entries(self._h, 0, None, None, C.byref(n)), "orbdb_entries")
        return n.value

    # -- queries ---------------------------------------------------------------------------------
    def query(self, words, values, stream=None):
        """One host query -> (keys, ncommon, score, first_word) of the live entries in insertion order."""
        w = np.ascontiguousarray(words, np.uint32)
        v = np.ascontiguousarray(values, np.float64)
        if len(w) != len(v):
            raise ValueError("words and values differ in length")
        cap = max(len(self), 1)
        keys, nc = np.zeros(cap, np.uint64), np.zeros(cap, np.int32)
        sc, fw = np.zeros(cap, np.float32), np.zeros(cap, np.uint32)
        n = C.c_int()
        check(self._lib.orbdb_query(self._h, _ptr(w), _ptr(v), len(w), cap, _ptr(keys), _ptr(nc), _ptr(sc), _ptr(fw),
                                    C.byref(n), stream), "orbdb_query")
        m = n.value
        return keys[:m], nc[:m], sc[:m], fw[:m]

    def query_device(self, nq, d_words, word_stride_bytes, d_values, value_stride_bytes, d_counts,
                     count_stride_bytes, stream=None):
        """nq queries in place (base addresses and byte strides) -> device tensors (ncommon int32, score float32,
        first_word as int32 bits), each (nq, capacity), indexed by entry index (entries())."""
        import torch
        dev = "cuda:%d" % self.device
        nc = torch.empty((nq, self.capacity), dtype=torch.int32, device=dev)
        sc = torch.empty((nq, self.capacity), dtype=torch.float32, device=dev)
        fw = torch.empty((nq, self.capacity), dtype=torch.int32, device=dev)
        check(self._lib.orbdb_query_device(self._h, int(nq), _ptr(d_words), int(word_stride_bytes), _ptr(d_values),
                                           int(value_stride_bytes), _ptr(d_counts), int(count_stride_bytes),
                                           _ptr(nc), _ptr(sc), _ptr(fw), stream), "orbdb_query_device")
        return nc, sc, fw

    def query_slots_device(self, all_slots, slot_bytes, nq, cap=None, stream=None):
        """query_device with each query's words, values and count taken in place from its slot."""
        ow, ov = self._slot_sections(all_slots, cap)
        base = _ptr(all_slots)
        return self.query_device(nq, base + ow, slot_bytes, base + ov, slot_bytes, base + _HDR_NBOW, slot_bytes,
                                 stream)

    def compact(self, ncommon, score, first_word):
        """One query's rows of query_device -> (keys, ncommon, score, first_word) in insertion order (host)."""
        keys, slots = self.entries()
        nc = ncommon.cpu().numpy()[slots]
        sc = score.cpu().numpy()[slots]
        fw = first_word.cpu().numpy().view(np.uint32)[slots]
        return keys, nc, sc, fw

    def check_error(self, stream=None):
        """True if a device add or query since the last call rejected its input (the flag is cleared)."""
        rc = self._lib.orbdb_check_error(self._h, stream)
        if rc not in (ORBX_OK, ORBX_EDEVICE):
            check(rc, "orbdb_check_error")
        return rc == ORBX_EDEVICE

    # -- candidates ------------------------------------------------------------------------------
    def _detect(self, mode, words, values, neighbours, connected, min_score, store, stream):
        keys, nc, sc, fw = self.query(words, values, stream)
        self.last = (keys, nc, sc, fw)
        index = {int(k): i for i, k in enumerate(keys)}
        neigh = [[index.get(int(j), -1) for j in list(neighbours.get(int(k), ()))[:10]] for k in keys]
        conn = None
        if connected is not None:
            conn = np.array([int(k) in connected for k in keys], np.uint8)
        last = np.array([store.get(int(k), 0.0) for k in keys], np.float32)
        out = select_candidates(mode, nc, sc, fw, neigh, last, conn, min_score)
        for k, v in zip(keys, last):
            store[int(k)] = np.float32(v)
        return [int(keys[i]) for i in out]

    def detect_loop_candidates(self, words, values, connected, neighbours, min_score, stream=None):
        """DetectLoopCandidates(pKF, minScore): (words, values) = pKF->mBowVec, connected = the keys of
        pKF->GetConnectedKeyFrames(), neighbours[key] = the keys of that keyframe's
        GetBestCovisibilityKeyFrames(10). Returns the candidates' keys."""
        return self._detect(MODE_LOOP, words, values, neighbours, set(int(c) for c in connected), min_score,
                            self.loop_score, stream)

    def detect_relocalization_candidates(self, words, values, neighbours, stream=None):
        """DetectRelocalizationCandidates(F): (words, values) = F->mBowVec."""
        return self._detect(MODE_RELOC, words, values, neighbours, None, 0.0, self.reloc_score, stream)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.orbdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
