"""tests/exact_filter_slots_ref.py (no GPU): the per-query restatement of the exact _slots calls equals exact_filter_ref run
per slot on the slot's queries, and the slot sets, assignments and grid of the GPU tests contain every case they claim."""
import numpy as np
import pytest

import exact_filter_ref as fr
import exact_filter_slots_ref as sr

N, D, NQ = 700, 16, 60


def _data():
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, size=(N, D), dtype=np.uint8)
    base[1] = base[0]
    base[7] = base[0]
    q = rng.integers(0, 256, size=(NQ, D), dtype=np.uint8)
    q[0] = base[0]
    return base, q


@pytest.mark.parametrize("assign", sr.ASSIGNMENTS)
def test_the_restatement_equals_the_single_filter_one_per_slot(assign):
    base, q = _data()
    nq = max(NQ, sr.MIN_NQ[assign])
    q = np.resize(q, (nq, D))
    masks = sr.slot_masks(N, sr.slot_sets(N))
    qslots = sr.assignment(assign, nq)
    radius = np.float32(16 * 90 * 90)
    for k in (1, 10, 100):
        got = sr.search(base, q, k, masks, qslots)
        blk = sr.search_blocked(base, q, k, masks, qslots)
        assert np.array_equal(got[1], blk[1]) and np.array_equal(got[0].view(np.uint32), blk[0].view(np.uint32))
        for b in np.unique(qslots):  # exact_filter_ref on the slot's queries
            idx = np.flatnonzero(qslots == b)
            mask = np.ones(N, bool) if b == sr.NONE else masks.get(int(b), np.zeros(N, bool))
            wd, wl = fr.search(base, q[idx], k, mask)
            assert np.array_equal(got[1][idx], wl) and np.array_equal(got[0][idx].view(np.uint32), wd.view(np.uint32))
    lims, d, l = sr.range_search(base, q, radius, masks, qslots)
    bl = sr.range_blocked(base, q, radius, masks, qslots)
    assert np.array_equal(lims, bl[0]) and np.array_equal(l, bl[2]) and np.array_equal(d.view(np.uint32), bl[1].view(np.uint32))
    assert int(lims[-1]) == l.size > 0
    for b in np.unique(qslots):
        idx = np.flatnonzero(qslots == b)
        mask = np.ones(N, bool) if b == sr.NONE else masks.get(int(b), np.zeros(N, bool))
        wlims, wd, wl = fr.range_search(base, q[idx], radius, mask)
        for j, qi in enumerate(idx):
            lo, hi = int(lims[qi]), int(lims[qi + 1])
            assert np.array_equal(l[lo:hi], wl[int(wlims[j]):int(wlims[j + 1])])
            assert np.array_equal(d[lo:hi].view(np.uint32), wd[int(wlims[j]):int(wlims[j + 1])].view(np.uint32))


def test_unset_slots_pass_nothing_and_none_passes_everything():
    masks = sr.slot_masks(N, sr.slot_sets(N))
    assert not sr.query_mask(N, masks, sr.UNSET[0]).any() and sr.query_mask(N, masks, sr.NONE).all()
    assert not set(sr.UNSET) & set(sr.SET) and all(0 <= s < sr.SLOTS for s in sr.SET + sr.UNSET)


def test_the_slot_sets_have_the_forms_they_claim():
    n = 6001
    npass = {s: int(m.sum()) for s, m in sr.slot_masks(n, sr.slot_sets(n)).items()}
    names = {name: npass[s] for s, name in sr.SLOT_PATTERNS.items()}
    assert len(sr.SLOT_PATTERNS) >= 12
    assert names["none"] == 0 and names["all"] == n                      # empty and full
    assert 0 < names["rand03"] <= n // 8 and 0 < names["last"] <= n // 8  # the rule keeps their lists
    assert names["rand50"] > n // 8 and names["gap"] > n // 8            # ... and sweeps these behind their pass words
    assert 33 <= names["rand64"] <= 99                                   # k = 100 is padded, on the 64-row strips
    assert names["deny0"] == n - 1 and names["only7"] == 1               # the tied rows {0, 1, 7}
    small = {s: int(m.sum()) for s, m in sr.slot_masks(33, sr.slot_sets(33)).items()}
    assert max(small.values()) == 33 and min(small.values()) == 0


def test_the_assignments_and_the_grid_have_the_cases_they_claim():
    grid = sr.grid()
    for i, axis in enumerate((sr.NS, sr.DS, sr.KS)):
        assert {c[i] for c in grid} == set(axis)
    assert {c[3] for c in grid} == set(sr.NQS) | {13}
    assert {c[4] for c in grid} == set(sr.ASSIGNMENTS) and {c[5] for c in grid} == set(sr.SPLITS) and {c[6] for c in grid} == set(sr.MAPS)
    assert all(c[3] >= sr.MIN_NQ[c[4]] for c in grid)
    for a in sr.ASSIGNMENTS:  # every assignment at every nq it fits, and with k = 100 (the 64-row strips) somewhere
        assert {c[3] for c in grid if c[4] == a} >= {q for q in sr.NQS if q >= sr.MIN_NQ[a]}
    assert {c[4] for c in grid if c[2] == 100} >= {"g129", "each", "sizes"}

    def groups(a, nq):
        b, c = np.unique(sr.assignment(a, nq), return_counts=True)
        return dict(zip(b.tolist(), c.tolist()))

    assert groups("none", 129) == {sr.NONE: 129} and groups("one", 33) == {0: 33}
    assert set(groups("each", 13).values()) == {1} and len(groups("each", 13)) == 13  # every strip 31 rows of padding
    g = groups("sizes", 129)
    assert (g[0], g[1], g[7]) == (31, 32, 33)
    assert groups("g129", 129) == {6: 129} and groups("g129", 300)[6] >= 129
    inter = sr.assignment("interleaved", 300)
    assert len(set(inter.tolist())) == 13 and (np.diff(inter.astype(int)) != 0).mean() > 0.8  # no sorted runs
    un = groups("unset", 300)
    assert all(un.get(s, 0) > 0 for s in sr.UNSET) and len(un) > 4
    # groups that are no multiple of 32: padded strips in every assignment but the whole-strip one
    assert any(v % 32 for v in groups("interleaved", 300).values())
