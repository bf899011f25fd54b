"""The NumPy twin of the track lifecycle (tests/lifecycle_ref.py) against an independent plain-Python model that keeps a dict
id -> (miss, hits) and a slot list per batch, and calls nothing of the twin: random lives of 30 frames, K in {0, 1, 3, 255},
saturation at 255, the cap, non-finite rows.  No GPU, no library."""
import math
import random

import numpy as np
import pytest

import lifecycle_ref as ref


class Model:
    """Plain Python.  slots[b] = list of ids in slot order; counters by id."""

    def __init__(self, n_batches):
        self.slots = [[] for _ in range(n_batches)]
        self.ctr = {}

    def create(self, b, ids):
        for i in ids:
            assert i not in self.ctr
            self.ctr[i] = (0, 0)
            self.slots[b].append(i)

    def step(self, has, K, det, slot_of_det, birth_batch, first_id, max_births):
        for b, ids in enumerate(self.slots):
            for s, i in enumerate(ids):
                miss, hits = self.ctr[i]
                if has[b][s]:
                    miss, hits = 0, min(hits + 1, 255)
                else:
                    miss = min(miss + 1, 255)
                self.ctr[i] = (miss, hits)
        retired = []
        for b, ids in enumerate(self.slots):
            stale = [s for s, i in enumerate(ids) if K >= 1 and self.ctr[i][0] >= K]
            retired += [ids[s] for s in stale]
            new_n = len(ids) - len(stale)
            gone = set(stale)
            tail = [s for s in range(new_n, len(ids)) if s not in gone]    # survivors at or above the new size, ascending
            holes = [s for s in stale if s < new_n]
            assert len(tail) == len(holes)
            for hole, src in zip(holes, tail):
                ids[hole] = ids[src]
            for i in retired:
                self.ctr.pop(i, None)
            del ids[new_n:]
        born, capped, non_finite = [], 0, 0
        if birth_batch is not None:
            for j, row in enumerate(det):
                if slot_of_det[j] >= 0:
                    continue
                if any(math.isnan(v) or math.isinf(v) for v in row):
                    non_finite += 1
                elif len(born) < max_births:
                    born.append(j)
                else:
                    capped += 1
            self.create(birth_batch, [first_id + r for r in range(len(born))])
        return retired, born, capped, non_finite


def _agree(model, twin):
    for b, ids in enumerate(model.slots):
        assert list(twin.ids[b]) == ids
        assert [(int(m), int(h)) for m, h in zip(twin.miss[b], twin.hits[b])] == [model.ctr[i] for i in ids]


@pytest.mark.parametrize("K", [0, 1, 3, 255])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_lives(K, seed):
    rnd = random.Random(1000 * K + seed)
    nb = 1 + seed % 2
    model, twin = Model(nb), ref.Tracker(nb)
    next_id = 0
    for b in range(nb):
        n = rnd.choice([0, 1, 63, 65, 130])
        ids = list(range(next_id, next_id + n))
        next_id += n
        model.create(b, ids)
        twin.create(b, ids)
    p_match = {0: 0.5, 1: 0.9, 3: 0.6, 255: 0.3}[K]
    for frame in range(30):
        has = [[1 if rnd.random() < p_match else 0 for _ in ids] for ids in model.slots]
        M = rnd.choice([0, 1, 7, 40])
        det = [[rnd.uniform(-5, 5) for _ in range(7)] for _ in range(M)]
        for row in det:
            if rnd.random() < 0.1:
                row[rnd.randrange(7)] = rnd.choice([float("nan"), float("inf"), -float("inf")])
        slot_of_det = [rnd.choice([-1, -1, 3]) for _ in range(M)]
        birth_batch = rnd.choice([None, 0, nb - 1])
        cap = rnd.choice([0, 3, 1000])
        got = twin.step([np.array(h, dtype=np.uint8) for h in has], K, np.array(det).reshape(-1, 7), np.array(slot_of_det, dtype=np.int32),
                        birth_batch, next_id, cap)
        want = model.step(has, K, det, slot_of_det, birth_batch, next_id, cap)
        assert list(got[0]) == want[0] and list(got[1]) == want[1] and got[2:] == want[2:]
        next_id += len(want[1])
        _agree(model, twin)


def test_saturation_at_255():
    model, twin = Model(1), ref.Tracker(1)
    model.create(0, [7, 8])
    twin.create(0, [7, 8])
    for frame in range(300):
        has = [[1, 0]]
        twin.step([np.array(has[0], dtype=np.uint8)], 0)
        model.step(has, 0, [], [], None, 0, 0)
    _agree(model, twin)
    assert model.ctr[7] == (0, 255) and model.ctr[8] == (255, 0)
    # K = 255 retires exactly at the saturated run
    assert list(twin.step([np.array([1, 0], dtype=np.uint8)], 255)[0]) == [8] and list(twin.ids[0]) == [7]


def test_erase_moves_cases():
    # the tail alone: no moves; more holes than tail survivors; all
    assert [list(a) for a in ref.erase_moves(6, [4, 5])] == [[], []]
    assert [list(a) for a in ref.erase_moves(6, [0, 1, 2, 4])] == [[3, 5], [0, 1]]
    assert [list(a) for a in ref.erase_moves(5, [0, 1, 2, 3, 4])] == [[], []]
    assert [list(a) for a in ref.erase_moves(7, [1, 5])] == [[6], [1]]
