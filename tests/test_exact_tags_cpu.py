"""tests/exact_tags_ref.py (no GPU): the restatement of the exact _tags calls is pinned to
exact_filter_ref run per tag on that tag's queries, and the shared fixture is shown to hold what the GPU tests rely on --
padding at k = 10 and k = 100, a tag of half the store and one of a single row, tags on both sides of a byte boundary and
the largest one, untagged rows, a tie at the k-th place inside a tag, absent tags, and more strips than the slot bound."""
import numpy as np
import pytest

import exact_filter_ref as fr
import exact_tags_ref as tr

N = tr.MANY_N


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


@pytest.mark.parametrize("n,d,nq,assign", [(33, 16, 33, "each"), (33, 48, 20, "absent"), (601, 16, 40, "interleaved"), (601, 32, 97, "sizes")])
def test_restatement_is_exact_filter_ref_per_tag(n, d, nq, assign):
    base = tr.make_base(n, d)
    q = tr.make_queries(nq, d, base)
    btags = tr.base_tags(n)
    qtags = tr.assignment(assign, n, nq)
    radius = np.float32(np.median(fr.search(base, q, min(10, n), np.ones(n, bool))[0][:, -1]))
    for k in (1, 10, 100):
        want_d = np.full((nq, k), tr.FLT_MAX, np.float32)
        want_l = np.full((nq, k), -1, np.int64)
        for t in np.unique(qtags):  # the loop the one call replaces: the tag's rows as an allow set, the tag's queries
            idx = np.flatnonzero(qtags == t)
            mask = np.ones(n, bool) if t == tr.NONE else fr.pass_mask(n, np.flatnonzero(btags == t))
            want_d[idx], want_l[idx] = fr.search(base, q[idx], k, mask)
        _same(tr.search(base, q, k, btags, qtags), (want_d, want_l))
        _same(tr.search_blocked(base, q, k, btags, qtags), (want_d, want_l))
    for r in (np.float32(0), radius, np.float32(np.inf)):
        per_q = [None] * nq
        for t in np.unique(qtags):
            idx = np.flatnonzero(qtags == t)
            mask = np.ones(n, bool) if t == tr.NONE else fr.pass_mask(n, np.flatnonzero(btags == t))
            lims, dd, ll = fr.range_search(base, q[idx], r, mask)
            for j, qi in enumerate(idx):
                per_q[qi] = (dd[int(lims[j]):int(lims[j + 1])], ll[int(lims[j]):int(lims[j + 1])])
        lims = np.zeros(nq + 1, np.uint64)
        lims[1:] = np.cumsum([p[0].size for p in per_q], dtype=np.uint64)
        want = (lims, np.concatenate([p[0] for p in per_q]), np.concatenate([p[1] for p in per_q]))
        _same(tr.range_search(base, q, r, btags, qtags), want)
        _same(tr.range_blocked(base, q, r, btags, qtags), want)


def test_apply_sets_is_incremental():
    t = tr.apply_sets(10, [([1, 2, 3, 10, 99], [5, 5, 6, 7, 7]), ([2, 9], [tr.NONE, 8])])
    assert t.tolist() == [tr.NONE, 5, tr.NONE, 6] + [tr.NONE] * 5 + [8]


@pytest.mark.parametrize("n", tr.NS)
def test_fixture_tags(n):
    t = tr.base_tags(n)
    assert t.dtype == np.uint16 and t.shape == (n,)
    cnt = {int(x): int(c) for x, c in zip(*np.unique(t, return_counts=True))}
    # (b) a tag holding at least half the rows and one holding exactly one row
    assert 2 * cnt[tr.BIG] >= n and cnt[tr.ONE] == 1
    # (c) tags 255, 256 and 0xfffe are in use, and some rows are untagged
    assert tr.FEW == 255 and tr.SOME == 256 and tr.ONE == 0xfffe and all(x in cnt for x in (255, 256, 0xfffe))
    assert cnt[tr.NONE] > 0
    # (e) tags queries name that no row carries
    assert all(a not in cnt for a in tr.ABSENT)
    qa = tr.assignment("absent", n, 33)
    assert np.isin(qa, tr.ABSENT).sum() >= 16
    if n > max(tr.TIED):
        assert (t[list(tr.TIED)] == tr.BIG).all()


def test_fixture_padding_ties_and_strips():
    t = tr.base_tags(N)
    cnt = {int(x): int(c) for x, c in zip(*np.unique(t, return_counts=True))}
    # (a) padding at k = 10 and at k = 100
    assert cnt[tr.FEW] < 10 and 10 <= cnt[tr.SOME] < 100
    assert (tr.assignment("g129", N, 300) == tr.SOME).sum() >= 129 and tr.FEW in tr.assignment("each", N, 33)
    # the tags of about 4 rows
    many = [cnt[tr.MANY0 + i] for i in range(tr.many_tags(N))]
    assert tr.many_tags(N) == 300 and min(many) >= 3 and max(many) == 4
    # (d) the k-th and (k + 1)-th nearest rows of query 0 inside its tag are at the same distance, k = 1 (and 2)
    for d in tr.DS:
        base = tr.make_base(N, d)
        q = tr.make_queries(33, d, base)
        for a in ("one", "each", "sizes"):
            assert tr.assignment(a, N, 33 if a != "sizes" else 129)[0] == tr.BIG
        dd, ll = fr.search(base, q[:1], 3, t == tr.BIG)
        assert dd[0].tolist() == [0, 0, 0] and ll[0].tolist() == list(tr.TIED)
    # (f) in "many" the strips outnumber the bound of the slot plan, m / 32 + 33
    qm = tr.assignment("many", N, 300)
    assert np.unique(qm).size == 300 and tr.strips(qm, t) == 300 > 300 // 32 + 33
    # ... and stay within the tag bound, m / 32 + min(m, tags in use + 1)
    for a in tr.ASSIGNMENTS:
        for nq in tr.NQS:
            if tr.fits(a, N, nq):
                qt = tr.assignment(a, N, nq)
                assert tr.strips(qt, t) <= nq // 32 + min(nq, tr.tags_in_use(t).size + 1)


def test_grid_covers_every_axis():
    g = tr.grid()
    for i, vals in enumerate((tr.NS, tr.DS, tr.KS, tr.NQS, tr.ASSIGNMENTS, tr.SPLITS, tr.MAPS)):
        assert {c[i] for c in g} == set(vals)
    assert all(tr.fits(c[4], c[0], c[3]) for c in g)
    assert (tr.MANY_N, 48, 10, 300, "many", 64, 1) in g
