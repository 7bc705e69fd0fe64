"""Exact range search of the float16 store under a base tag per query (ivfhnsw_gpu_exact_range_search_f16_tags, DESIGN.md
3.30): integer rows bit for bit against the restatement of the uint8 _tags call, the per-wave tile map on a sparse store,
the bits of exact_search_f16_tags on real rows, float64 within the bound of 3.27, and the state and the refusals."""
import numpy as np
import pytest

import exact_ref
import exact_tags_ref as tr
from test_gpu_base_f16 import _real

pytestmark = pytest.mark.gpu

F = np.float32
NQS, DS = (1, 33, 129, 300), (16, 96, 256)


def _same(got, want):
    assert np.array_equal(got[0], want[0]), np.nonzero(got[0] != want[0])[0][:5]
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _mine(btags, qtags):
    """bool [nq, n]: the rows each query searches."""
    return np.stack([tr.tag_mask(btags, t) for t in qtags])


def _grid():
    """(n, d, nq, assignment, exact_splits, exact_range_map), the axes cycling as test_gpu_base_f16_tags.py's _grid() cycles
    them, plus the corners: Dense ranges of 5 and 2 strips (a partial workgroup), a 4-row tag under 3 splits with and without
    the map, one query per tag on the 33-row store, and a call of two chunks (16 384 + 33 queries), each with its own plan."""
    names = ("none", "each", "sizes", "g129", "absent")
    cases = []
    for i, (n, d, use_map) in enumerate((n, d, u) for n in tr.NS for d in DS for u in (0, 1)):
        a = names[i % len(names)]
        nqs = [q for q in NQS if tr.fits(a, n, q)]
        cases.append((n, d, nqs[i % len(nqs)], a, (1, 3)[(i // 2) % 2], use_map))
    i = 0
    for a in names + ("many",):
        for nq in NQS:
            if tr.fits(a, tr.MANY_N, nq):
                cases.append((tr.MANY_N, DS[i % 3], nq, a, (1, 3)[(i // 3) % 2], (i // 2) % 2))
                i += 1
    cases += [(tr.MANY_N, 96, 129, "none", 3, 1), (tr.MANY_N, 256, 33, "none", 1, 1), (tr.MANY_N, 16, 300, "many", 3, 1),
              (tr.MANY_N, 96, 300, "many", 3, 0), (33, 16, 33, "each", 3, 1), (33, 16, 16384 + 33, "each", 3, 1)]
    return sorted(set(cases))


_STORES = {}


@pytest.fixture(scope="module")
def int_store(pkg):
    """(rows u8, tags, handle with both installed) per (n, d), made once; values 0..127 at d = 256, where bytes are not exact."""
    def get(n, d):
        if (n, d) not in _STORES:
            base = tr.make_base(n, d) >> np.uint8(d == 256)
            g = pkg.GpuIndex(0)
            g.upload_base_f16(base.astype(F))
            g.set_base_tags(np.arange(n, dtype=np.uint32), tr.base_tags(n))
            _STORES[n, d] = base, tr.base_tags(n), g
        return _STORES[n, d]
    yield get
    for _, _, g in _STORES.values():
        g.close()
    _STORES.clear()


# ---- 1. integer rows: every operation exact, so lims, labels and distance bits are the restatement's
@pytest.mark.parametrize("n,d,nq,assign,splits,use_map", _grid())
def test_integer_rows_equal_the_restatement(int_store, n, d, nq, assign, splits, use_map):
    base, btags, g = int_store(n, d)
    q = tr.make_queries(nq, d, tr.make_base(n, d)) >> np.uint8(d == 256)
    qtags = tr.assignment(assign, n, nq)
    g.set_option("exact_splits", splits)
    g.set_option("exact_range_map", use_map)
    own = np.sort(exact_ref.distances(base, q)[_mine(btags, qtags)])  # the distances of the pairs a query may return
    low = float(own[own.size // 100]) if own.size else 1.0           # an integer some pair sits ON (strict <)
    for radius in (low, low + 0.5) + ((np.inf,) if n == 33 else ()):
        _same(g.exact_range_search_f16_tags(q.astype(F), radius, qtags), tr.range_blocked(base, q, radius, btags, qtags))


# ---- 2. a handful of near rows in a far store: each wave skips by its own bits, beside a neighbour that visits
def test_sparse_hits_with_and_without_the_map(pkg):
    rng = np.random.default_rng(3)
    n, nq, d = 4133, 129, 128
    x = rng.integers(100, 128, (n, d), dtype=np.uint8)
    q = rng.integers(0, 4, (nq, d), dtype=np.uint8)
    btags = (np.arange(n) % 3).astype(np.uint16)  # a list of 1378 rows: 44 tiles, the last one partial, 15 to a split
    qtags = np.repeat(np.array([0, 1, 2, tr.NONE], np.uint16), 40)[:nq]  # two strips a tag, four of them in the first workgroup
    qtags[120:] = tr.NONE                                               # ... and a Dense strip of 9
    # (row, query): the first, a middle and the last tile of the row's tag's LIST, for queries of both strips of a tag; rows
    # 2001 and 5 serve an untagged query and a query of ANOTHER tag, which must not see it
    for row, qi in ((3, 0), (94, 41), (2067, 35), (2000, 100), (4132, 70), (2001, 128), (5, 1)):
        x[row] = q[qi]
        x[row, 0] += 2
    want = tr.range_blocked(x, q, 50.0, btags, qtags)
    assert want[0][-1] == 6
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x.astype(F))
    g.set_base_tags(np.arange(n, dtype=np.uint32), btags)
    g.set_option("exact_splits", 3)
    for use_map in (1, 0):  # (both equal the restatement, so each other)
        g.set_option("exact_range_map", use_map)
        _same(g.exact_range_search_f16_tags(q.astype(F), 50.0, qtags), want)
    g.close()


# ---- 3. real rows: the pairs and the bits of exact_search_f16_tags, wherever a column falls in a list, tile or split
@pytest.mark.parametrize("d", [96, 256])
def test_same_bits_as_the_k_search(pkg, d):
    rng = np.random.default_rng(d)
    n, nq = 100, 33
    x, q = rng.standard_normal((n, d), dtype=F), rng.standard_normal((nq, d), dtype=F)
    btags = (np.arange(n) % 3).astype(np.uint16)
    qtags = np.array([0, 1, 2, tr.NONE, 7], np.uint16)[np.arange(nq) % 5]  # (no row carries 7)
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x)
    g.set_base_tags(np.arange(n, dtype=np.uint32), btags)
    dist, lab = g.exact_search_f16_tags(q, n, qtags)
    found = lab >= 0
    assert np.array_equal(found.sum(1), _mine(btags, qtags).sum(1))
    radius = float(np.median(dist[found]))
    lims, rd, rl = g.exact_range_search_f16_tags(q, radius, qtags)
    g.close()
    for i in range(nq):
        keep = found[i] & (dist[i] < F(radius))
        order = np.argsort(lab[i][keep])
        a, b = int(lims[i]), int(lims[i + 1])
        assert np.array_equal(rl[a:b], lab[i][keep][order])
        assert np.array_equal(rd[a:b].view(np.uint32), dist[i][keep][order].view(np.uint32))
    assert 0 < lims[-1] == len(rl)


# ---- 4. real rows against float64, within tol(q, x) = (d + 3) 2^-23 (|q^| + |x^|)^2, each query inside its tag's rows
def test_real_rows_within_the_bound_of_float64(pkg):
    x, q, D, tol = _real(96)
    n, nq, radius = len(x), len(q), 120.0
    btags, qtags = tr.base_tags(n), tr.assignment("interleaved", n, nq)
    qtags[::4] = tr.NONE  # (two Dense strips are wanted)
    mine = _mine(btags, qtags)
    undecided = int((mine & (np.abs(D - radius) <= tol)).sum())
    assert undecided < 0.01 * (mine & (D < radius - tol)).sum(), undecided
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x)
    g.set_base_tags(np.arange(n, dtype=np.uint32), btags)
    lims, dist, lab = g.exact_range_search_f16_tags(q, radius, qtags)
    none = np.flatnonzero(qtags == tr.NONE)
    plain = g.exact_range_search_f16(q[none], radius)
    g.close()
    qi = np.repeat(np.arange(nq), np.diff(lims).astype(np.int64))
    returned = np.zeros(D.shape, bool)
    returned[qi, lab] = True
    assert returned.sum() == len(lab) and not returned[~mine].any()
    assert returned[mine & (D < radius - tol)].all() and not returned[D > radius + tol].any()
    err = np.abs(dist.astype(np.float64) - D[qi, lab])
    print("undecided %d of %d returned; largest |returned - float64| / tol = %.4f" % (undecided, len(lab), (err / tol[qi, lab]).max()))
    assert (err <= tol[qi, lab]).all()
    assert ((np.diff(lab) > 0) | (np.diff(qi) > 0)).all()  # ascending label inside a query
    # the untagged queries run the staged arithmetic of the plain call
    assert none.size > 32
    sel = np.isin(qi, none)
    assert np.array_equal(np.diff(lims)[none], np.diff(plain[0])) and np.array_equal(lab[sel], plain[2])
    assert np.array_equal(dist[sel].view(np.uint32), plain[1].view(np.uint32))


# ---- 5. state and refusals
@pytest.mark.parametrize("case", ["none_is_plain", "on_u8", "before_upload", "no_tags", "nan", "view", "dev", "nq0"])
def test_state_and_refusals(pkg, case):
    n, d, nq, radius = 1000, 32, 40, 70000.0
    base = tr.make_base(n, d)  # (bytes are exact at d = 32)
    q = tr.make_queries(nq, d, base)
    xf, qf = base.astype(F), q.astype(F)
    btags, qtags = tr.base_tags(n), tr.assignment("absent", n, nq)
    rows = np.arange(n, dtype=np.uint32)
    want = tr.range_blocked(base, q, radius, btags, qtags)
    g = pkg.GpuIndex(0)

    def code(*a):
        with pytest.raises(pkg.IvfHnswError) as e:
            g.exact_range_search_f16_tags(*a)
        return e.value.code

    def held():  # the results the handle holds are the tagged call's
        got = g.exact_range_results(0, int(want[0][-1]))
        return np.array_equal(got[1], want[2]) and np.array_equal(got[0].view(np.uint32), want[1].view(np.uint32))

    if case in ("on_u8", "before_upload"):
        if case == "on_u8":
            g.upload_base(base)
            g.set_base_tags(rows, btags)
        assert code(qf, radius, qtags) == pkg.ERR_STATE
        g.close()
        return
    g.upload_base_f16(xf)
    if case == "no_tags":  # every row untagged: a tagged query finds nothing, an untagged one the whole store
        _same(g.exact_range_search_f16_tags(qf, radius, qtags), tr.range_blocked(base, q, radius, np.full(n, tr.NONE, np.uint16), qtags))
    g.set_base_tags(rows, btags)
    _same(g.exact_range_search_f16_tags(qf, radius, qtags), want)
    if case == "none_is_plain":
        plain = g.exact_range_search_f16(qf, radius)
        _same(g.exact_range_search_f16_tags(qf, radius, None), plain)
        _same(g.exact_range_search_f16_tags(qf, radius, np.full(nq, tr.NONE, np.uint16)), plain)
    elif case == "nan":
        assert code(qf, np.nan, qtags) == pkg.ERR_INVALID and held()  # a refused call leaves the earlier results readable
    elif case == "view":
        v = g.view()
        _same(v.exact_range_search_f16_tags(qf, radius, qtags), want)
        v.close()
    elif case == "dev":
        import torch
        dev = torch.device("cuda", 0)
        tq, tt = torch.from_numpy(qf).to(dev), torch.from_numpy(qtags.view(np.int16)).to(dev)
        tl = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        assert g.exact_range_search_f16_tags_dev(nq, tq, d, tt, radius, tl) == want[0][-1]
        assert np.array_equal(tl.cpu().numpy().view(np.uint64), want[0]) and held()
    elif case == "nq0":
        lims, dist, lab = g.exact_range_search_f16_tags(qf[:0], radius, qtags[:0])
        assert lims.tolist() == [0] and len(dist) == 0 and len(lab) == 0
    g.close()
