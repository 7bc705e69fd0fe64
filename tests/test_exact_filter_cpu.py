"""tests/exact_filter_ref.py on the host (no GPU): the restatement of the exact calls under a base filter equals the
unfiltered restatements (exact_ref.search, exact_range_ref.search, themselves pinned to fvec_L2sqr by test_exact_cpu.py
and test_exact_range_cpu.py) run on base[pass], with the labels mapped back through np.flatnonzero(pass) -- for every
pass pattern the GPU tests use; and ALLOW of a set and DENY of its complement are the same mask."""
import numpy as np
import pytest

import exact_filter_ref as fr
import exact_range_ref
import exact_ref


def _base(rng, n, d):
    b = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    if n > 7:
        b[1] = b[0]
        b[7] = b[0]
        b[n - 1] = b[3]
        b[4] = 0
        b[5] = 255
    return b


CASES = [(name, n) for name in fr.PATTERNS for n in (1, 31, 33, 6001)]


@pytest.mark.parametrize("name,n", CASES)
def test_restatement_equals_the_unfiltered_one_on_the_passing_rows(name, n):
    rng = np.random.default_rng(n * 131 + len(name))
    d, nq = 16, 9
    base = _base(rng, n, d)
    q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
    q[0] = base[0]
    labels, deny = fr.pattern(name, n)
    mask = fr.pass_mask(n, labels, deny)
    rows = np.flatnonzero(mask)
    for k in (1, 10, 100):
        got_d, got_l = fr.search(base, q, k, mask)
        if rows.size:
            want_d, sub_l = exact_ref.search(base[rows], q, k)
            want_l = np.where(sub_l >= 0, rows[np.maximum(sub_l, 0)], -1)
        else:
            want_d, want_l = np.full((nq, k), fr.FLT_MAX, np.float32), np.full((nq, k), -1, np.int64)
        assert np.array_equal(got_l, want_l)
        assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    dist = exact_ref.distances(base, q)
    for radius in (0.0, float(np.median(dist)), float("inf")):
        lims, dd, ll = fr.range_search(base, q, radius, mask)
        if rows.size:
            wl, wd, sub = exact_range_ref.search(base[rows], q, radius)
            wlab = rows[sub]
        else:
            wl, wd, wlab = np.zeros(nq + 1, np.uint64), np.zeros(0, np.float32), np.zeros(0, np.int64)
        assert np.array_equal(lims, wl) and np.array_equal(ll, wlab)
        assert np.array_equal(dd.view(np.uint32), wd.view(np.uint32))
        assert int(lims[-1]) == ll.size


def test_patterns_are_what_their_names_say():
    n = 6001
    m = {name: fr.pass_mask(n, *fr.pattern(name, n)) for name in fr.PATTERNS}
    w = lambda a: np.add.reduceat(a.astype(int), np.arange(0, n, 32))  # noqa: E731  passing rows per word
    assert m["all"].all() and not m["none"].any()
    assert np.flatnonzero(m["last"]).tolist() == [n - 1] and np.flatnonzero(m["first"]).tolist() == [0]
    a = w(m["alt_first_empty"])
    assert a[0] == 0 and a[1] == 32 and set(a[:-1]) == {0, 32}
    b = w(m["alt_last_empty"])
    assert b[-1] == 0 and b[-2] == 32
    g = w(m["gap"])
    assert (g[5:9] == 0).all() and g[4] == 32 and g[9] == 32
    assert 0 < m["rand03"].sum() <= n // 8 < m["rand50"].sum()
    assert not m["deny0"][0] and m["deny0"][1:].all()
    assert np.flatnonzero(m["only7"]).tolist() == [7]


@pytest.mark.parametrize("n", (1, 33, 6001))
def test_allow_of_a_set_is_deny_of_its_complement(n):
    rng = np.random.default_rng(n)
    s = rng.random(n) < 0.3
    allow = np.flatnonzero(s).astype(np.uint32)
    deny = np.flatnonzero(~s).astype(np.uint32)
    a = fr.pass_mask(n, allow, deny=False)
    assert np.array_equal(a, s) and np.array_equal(a, fr.pass_mask(n, deny, deny=True))
    # labels at or beyond n and repeats change nothing, in either mode
    junk = np.array([n, n + 1, 2 ** 32 - 1], np.uint32)
    assert np.array_equal(a, fr.pass_mask(n, np.concatenate([allow, allow, junk]), deny=False))
    assert np.array_equal(a, fr.pass_mask(n, np.concatenate([deny, deny, junk]), deny=True))
