"""NumPy twin of the track-lifecycle rule (include/target_estimation_amd/target_batch_c.h, target_manager_lifecycle):
the per-slot counters, the stale list, the move order of Batch::erase_slots, the born list with its cap and finiteness rule, and the
slot -> id layout a call leaves.  Nothing here touches the library: the GPU tests hold the device path to it, and
tests/test_lifecycle_reference.py holds it to an independent plain-Python model."""
import numpy as np


def count(has, miss, hits):
    """The counters behind one call: a mask byte != 0 resets miss and counts a hit, 0 lengthens the run; both saturate at 255."""
    has = np.asarray(has).astype(bool)
    miss = np.asarray(miss, dtype=np.uint8).astype(np.int64)
    hits = np.asarray(hits, dtype=np.uint8).astype(np.int64)
    new_miss = np.where(has, 0, np.minimum(miss + 1, 255))
    new_hits = np.where(has, np.minimum(hits + 1, 255), hits)
    return new_miss.astype(np.uint8), new_hits.astype(np.uint8)


def stale_slots(new_miss, max_misses):
    """ascending slots with K >= 1 and miss >= K"""
    if max_misses < 1:
        return np.zeros(0, dtype=np.int64)
    return np.nonzero(np.asarray(new_miss).astype(np.int64) >= max_misses)[0]


def erase_moves(n, stale):
    """(src, dst) of Batch::erase_slots given the ascending list: the holes below the new size are filled, in order, by the survivors
    at or above it."""
    stale = np.asarray(stale, dtype=np.int64)
    new_n = n - len(stale)
    gone = np.zeros(n, dtype=bool)
    gone[stale] = True
    dst = np.nonzero(gone[:new_n])[0]
    src = new_n + np.nonzero(~gone[new_n:])[0]
    assert len(src) == len(dst)
    return src, dst


def erase(columns, stale):
    """every per-slot array of `columns` after the erase: moved survivors, then cut to the new size"""
    n = len(columns[0])
    src, dst = erase_moves(n, stale)
    out = []
    for c in columns:
        c = np.array(c, copy=True)
        c[dst] = c[src]
        out.append(c[:n - len(stale)])
    return out


def born(det, slot_of_det, births_on, max_births):
    """(born detection indices ascending, unmatched not born because of the cap, unmatched not born because non-finite)"""
    if not births_on or det is None or len(det) == 0:
        return np.zeros(0, dtype=np.int64), 0, 0
    det = np.asarray(det, dtype=np.float64).reshape(-1, 7)
    unmatched = np.asarray(slot_of_det) < 0
    finite = np.isfinite(det).all(axis=1)
    cand = np.nonzero(unmatched & finite)[0]
    k = min(len(cand), max_births)
    return cand[:k], len(cand) - k, int((unmatched & ~finite).sum())


class Tracker:
    """The population as the rule sees it: per batch the slot -> id list and the two counters.  step() is one lifecycle call."""

    def __init__(self, n_batches=1):
        self.ids = [np.zeros(0, dtype=np.uint32) for _ in range(n_batches)]
        self.miss = [np.zeros(0, dtype=np.uint8) for _ in range(n_batches)]
        self.hits = [np.zeros(0, dtype=np.uint8) for _ in range(n_batches)]

    def create(self, batch, ids):
        """targets created by any means: counters 0, appended in order"""
        while batch >= len(self.ids):
            self.ids.append(np.zeros(0, dtype=np.uint32))
            self.miss.append(np.zeros(0, dtype=np.uint8))
            self.hits.append(np.zeros(0, dtype=np.uint8))
        ids = np.asarray(ids, dtype=np.uint32)
        self.ids[batch] = np.concatenate([self.ids[batch], ids])
        self.miss[batch] = np.concatenate([self.miss[batch], np.zeros(len(ids), dtype=np.uint8)])
        self.hits[batch] = np.concatenate([self.hits[batch], np.zeros(len(ids), dtype=np.uint8)])

    def step(self, has, max_misses, det=None, slot_of_det=None, birth_batch=None, first_id=0, max_births=0):
        """has: one mask per batch.  Returns (retired ids, born detection indices, capped, non_finite); the births go to
        birth_batch (None: no births)."""
        retired = []
        for b in range(len(self.ids)):
            self.miss[b], self.hits[b] = count(has[b][:len(self.ids[b])], self.miss[b], self.hits[b])
        for b in range(len(self.ids)):
            stale = stale_slots(self.miss[b], max_misses)
            retired.extend(int(i) for i in self.ids[b][stale])
            self.ids[b], self.miss[b], self.hits[b] = erase([self.ids[b], self.miss[b], self.hits[b]], stale)
        rows, capped, non_finite = born(det, slot_of_det, birth_batch is not None, max_births)
        if len(rows):
            self.create(birth_batch, first_id + np.arange(len(rows), dtype=np.uint32))
        return np.array(retired, dtype=np.uint32), rows, capped, non_finite
