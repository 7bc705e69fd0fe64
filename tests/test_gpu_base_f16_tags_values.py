"""A base tag AND an interval of base values per query on the float16 store (ivfhnsw_gpu_exact_search_f16_tags_values,
DESIGN.md 3.33) against a plain numpy reference, bit for bit: rows and queries are integers 0..127, for which norms, dot
products and their combination are exact in float32 at every d <= 256."""
import contextlib
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F, NONE, VNONE, WHOLE = np.float32, 0xffff, 0xffffffff, (0, 0xffffffff)
FLT_MAX = np.finfo(F).max
SIZES = (1, 31, 32, 33, 300)  # the rows of tags 1 .. 5, as far as the store has room; tag 9 is never used


def _same(got, want):
    assert np.array_equal(got[1], want[1]), np.nonzero((got[1] != want[1]).any(1))[0][:5]
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def _code(pkg, f, *a):
    with pytest.raises(pkg.IvfHnswError) as e:
        f(*a)
    return e.value.code


def _ref(dist, btags, bvals, qt, qr, k):
    """dist [nq, n]: the distances; per query the k nearest of the rows that pass the rule, by (distance, row)."""
    out_d, out_l = np.full((len(qt), k), FLT_MAX, F), np.full((len(qt), k), -1, np.int64)
    for i, (t, (lo, hi)) in enumerate(zip(qt, qr)):
        rows = np.nonzero(((t == NONE) | (btags == t)) & (lo <= bvals) & (bvals <= hi))[0]
        rows = rows[np.lexsort((rows, dist[i, rows]))][:k]
        out_d[i, :len(rows)], out_l[i, :len(rows)] = dist[i, rows], rows
    return out_d, out_l


def _dists(q, x):
    q, x = q.astype(np.int64), x.astype(np.int64)
    return (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2 * q @ x.T


def _layout(n, seed=7):
    """tags: lists scattered over the store; values: ascending with the row number, valueless among the untagged rows and tag 5's"""
    rng = np.random.default_rng(seed)
    perm, btags, off = rng.permutation(n), np.full(n, NONE, np.uint16), 0
    for t, size in enumerate(SIZES, 1):
        if off + size < n:
            btags[perm[off:off + size]] = t
            off += size
    bvals = (10 * np.arange(n) + 5).astype(np.uint32)
    bvals[((btags == NONE) | (btags == 5)) & (np.arange(n) % 7 == 3)] = VNONE
    return btags, bvals


def _queries(nq, btags, bvals):
    """the mix of (tag, interval), cycling; B the largest tag in use"""
    B = int(btags[btags != NONE].max())
    mine = np.sort(bvals[(btags == B) & (bvals != VNONE)])
    everyone = np.sort(bvals[bvals != VNONE])
    other = int(bvals[(btags != B) & (bvals != VNONE)][0])
    at = lambda t, c: (t, (int(bvals[np.nonzero(btags == t)[0][c]]),) * 2) if (btags == t).sum() > c else (B, WHOLE)
    small = lambda t: t if (btags == t).any() else B
    kinds = [(NONE, WHOLE), (B, (int(mine[len(mine) // 4]), int(mine[len(mine) // 2]))),
             (NONE, (int(everyone[len(everyone) // 3]), int(everyone[len(everyone) // 2]))), (B, WHOLE), (B, (5, 4)), (9, WHOLE),
             (B, (other, other)), at(4, 31), at(4, 32), (B, (int(mine[0]), int(mine[min(2, len(mine) - 1)]))), (small(1), WHOLE),
             (small(2), (int(everyone[2]), int(everyone[-3]))), (small(3), WHOLE)]
    pick = [kinds[(i + 1) % len(kinds)] for i in range(nq)]
    return np.array([t for t, _ in pick], np.uint16), np.array([r for _, r in pick], np.uint32)


_STORES = {}


@pytest.fixture(scope="module")
def store(pkg):
    """per (d, n), made once: rows, 129 queries, their distances, tags, the two value layouts, the handle"""
    def get(d, n):
        if (d, n) not in _STORES:
            rng = np.random.default_rng(1000 * d + n)
            x, q = rng.integers(0, 128, (n, d)).astype(F), rng.integers(0, 128, (129, d)).astype(F)
            btags, asc = _layout(n)
            g = pkg.GpuIndex(0)
            g.upload_base_f16(x)
            g.set_base_tags(np.arange(n, dtype=np.uint32), btags)
            _STORES[d, n] = dict(g=g, q=q, dist=_dists(q, x).astype(F), btags=btags, asc=asc, shuffled=rng.permutation(asc))
        return _STORES[d, n]
    yield get
    for s in _STORES.values():
        s["g"].close()
    _STORES.clear()


# ---- 1. the grid: every path of the sweep (one step / late pieces, one tile plus a column, a strip plus a row, the CAP
# classes, splits longer than short lists) under values that leave dead tiles (ascending) and that leave none (shuffled)
@pytest.mark.parametrize("d,n,nq,k,splits,values", list(itertools.product((16, 96, 256), (33, 4133), (1, 33, 129), (1, 33, 100), (1, 3),
                                                                          ("asc", "shuffled"))))
def test_grid_equals_the_reference(store, d, n, nq, k, splits, values):
    s = store(d, n)
    g, bvals = s["g"], s[values]
    g.set_base_values(np.arange(n, dtype=np.uint32), bvals)
    g.set_option("exact_splits", splits)
    qt, qr = _queries(nq, s["btags"], bvals)
    _same(g.exact_search_f16_tags_values(s["q"][:nq], k, qt, qr), _ref(s["dist"], s["btags"], bvals, qt, qr, k))


# ---- 2. ties: a tag whose 640 rows repeat 8 vectors over 20 tiles, every other one inside the interval
@pytest.mark.parametrize("splits", (1, 3))
def test_ties_come_in_ascending_label(pkg, splits):
    n, d, nq, k = 1300, 32, 33, 100
    rng = np.random.default_rng(5)
    x, q = rng.integers(0, 128, (n, d)).astype(F), rng.integers(0, 128, (nq, d)).astype(F)
    mine = np.arange(10, 1290, 2)
    x[mine] = x[:8][np.arange(len(mine)) % 8]
    btags, bvals = np.full(n, NONE, np.uint16), np.full(n, 7, np.uint32)
    btags[mine], bvals[mine[::2]] = 3, 100
    qt, qr = np.full(nq, 3, np.uint16), np.tile(np.array([(50, 100)], np.uint32), (nq, 1))
    with contextlib.closing(pkg.GpuIndex(0)) as g:
        g.upload_base_f16(x)
        g.set_base_tags(np.arange(n, dtype=np.uint32), btags)
        g.set_base_values(np.arange(n, dtype=np.uint32), bvals)
        g.set_option("exact_splits", splits)
        got = g.exact_search_f16_tags_values(q, k, qt, qr)
    assert (np.diff(got[0], axis=1) == 0).sum() > nq * k // 2
    _same(got, _ref(_dists(q, x).astype(F), btags, bvals, qt, qr, k))


# ---- 3. the NULL forms are the siblings, bit for bit; 6. the refusals; a view answers as its parent
@pytest.mark.parametrize("case", ["null_forms", "on_u8", "bad_k", "view"])
def test_null_forms_and_refusals(pkg, store, case):
    s = store(96, 4133)
    g, q, k = s["g"], s["q"], 10
    g.set_base_values(np.arange(4133, dtype=np.uint32), s["asc"])
    g.set_option("exact_splits", -1)
    qt, qr = _queries(129, s["btags"], s["asc"])
    if case == "null_forms":
        _same(g.exact_search_f16_tags_values(q, k, qt, None), g.exact_search_f16_tags(q, k, qt))
        _same(g.exact_search_f16_tags_values(q, k, None, qr), g.exact_search_f16_values(q, k, qr))
        _same(g.exact_search_f16_tags_values(q, k, None, None), g.exact_search_f16(q, k))
    elif case == "on_u8":
        with contextlib.closing(pkg.GpuIndex(0)) as u:
            u.upload_base(np.zeros((33, 96), np.uint8))
            assert _code(pkg, u.exact_search_f16_tags_values, q, k, qt, qr) == pkg.ERR_STATE
    elif case == "bad_k":
        assert _code(pkg, g.exact_search_f16_tags_values, q, 0, qt, qr) == pkg.ERR_INVALID
        assert _code(pkg, g.exact_search_f16_tags_values, q, 101, qt, qr) == pkg.ERR_INVALID
    else:
        v = g.view()
        _same(v.exact_search_f16_tags_values(q, k, qt, qr), g.exact_search_f16_tags_values(q, k, qt, qr))
        v.close()


# ---- 4. real values: the bound of the plain call against float64 over the rounded halves
def test_real_values_within_the_bound(pkg):
    n, d, nq, k = 1000, 96, 40, 10
    rng = np.random.default_rng(11)
    x, q = rng.normal(size=(n, d)).astype(F), rng.normal(size=(nq, d)).astype(F)
    btags, bvals = _layout(n)
    qt, qr = _queries(nq, btags, bvals)
    with contextlib.closing(pkg.GpuIndex(0)) as g:
        g.upload_base_f16(x)
        g.set_base_tags(np.arange(n, dtype=np.uint32), btags)
        g.set_base_values(np.arange(n, dtype=np.uint32), bvals)
        dist, lab = g.exact_search_f16_tags_values(q, k, qt, qr)
    xh, qh = x.astype(np.float16).astype(np.float64), q.astype(np.float16).astype(np.float64)
    for i in range(nq):
        true = ((qh[i] - xh) ** 2).sum(1)
        bound = (d + 3) * 2.0 ** -23 * (np.linalg.norm(qh[i]) + np.linalg.norm(xh, axis=1)) ** 2
        ok = ((qt[i] == NONE) | (btags == qt[i])) & (qr[i, 0] <= bvals) & (bvals <= qr[i, 1])
        got = lab[i][lab[i] >= 0]
        assert len(got) == min(k, ok.sum()) and ok[got].all() and len(set(got)) == len(got)
        assert (np.abs(dist[i, :len(got)] - true[got]) <= bound[got]).all()
        if len(got) == k:
            must = np.nonzero(ok & (true < dist[i, k - 1] - 2 * bound))[0]
            assert set(must) <= set(got)


# ---- 5. the device form: strided queries, tag and range tensors, two chunks of at most 16 384 queries on a 33-row store
def test_dev_form_over_two_chunks(pkg):
    import torch
    n, d, k, nq = 33, 16, 1, 16384 + 33
    rng = np.random.default_rng(3)
    x, q = rng.integers(0, 128, (n, d)).astype(F), rng.integers(0, 128, (nq, d)).astype(F)
    btags, bvals = _layout(n)
    qt, qr = _queries(nq, btags, bvals)
    dev = torch.device("cuda", 0)
    wide = np.full((nq, d + 1), np.nan, F)  # an .fvecs image's stride; the header column is never read
    wide[:, 1:] = q
    tw, tt, tr = (torch.from_numpy(a).to(dev) for a in (wide, qt.view(np.int16), qr.view(np.int32)))
    od, ol = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev), torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    with contextlib.closing(pkg.GpuIndex(0)) as g:
        g.upload_base_f16(x)
        g.set_base_tags(np.arange(n, dtype=np.uint32), btags)
        g.set_base_values(np.arange(n, dtype=np.uint32), bvals)
        torch.cuda.synchronize(dev)
        g.exact_search_f16_tags_values_dev(nq, tw.data_ptr() + 4, d + 1, k, tt, tr, od, ol)
        g.sync()
    _same((od.cpu().numpy(), ol.cpu().numpy()), _ref(_dists(q, x).astype(F), btags, bvals, qt, qr, k))
