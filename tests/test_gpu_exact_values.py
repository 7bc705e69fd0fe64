"""The exact calls with an interval of base values per query (ivfhnsw_gpu_exact_search_values /
ivfhnsw_gpu_exact_range_search_values).  Every case is checked twice: (A) against the numpy restatement
(tests/exact_values_ref.py) -- labels, distance BITS, lims in the caller's order, range results in ascending label -- and
(B) against a second handle that installs each distinct interval's rows with set_base_filter and runs the plain calls on
that interval's queries.  The shapes are where the windowed sweep can break: strips of identical and of distinct
intervals, one near-full window among 31 narrow ones, windows at the two ends of the value order in one strip, single-row
windows, absent and inverted intervals, k larger than the window, a block of byte-identical rows whose values descend
(ties at the k-th distance arrive in the wrong order), forced column splits, with and without the tile map, more than one
chunk.  Everything is exact: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import exact_filter_ref as fr
import exact_ref
import exact_values_ref as vr

pytestmark = pytest.mark.gpu

F = np.float32


def _same(got, want):
    (gd, gl), (wd, wl) = got, want
    assert gl.dtype == np.int64 and gd.dtype == np.float32
    assert np.array_equal(gl, wl), np.nonzero((gl != wl).any(1))[0][:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _same_range(got, want):
    (gl, gd, gb), (wl, wd, wb) = got, want
    assert gl.dtype == np.uint64 and gd.dtype == np.float32 and gb.dtype == np.int64
    assert np.array_equal(gl, wl), np.nonzero(gl != wl)[0][:5]
    assert np.array_equal(gb, wb), np.nonzero(gb != wb)[0][:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
    assert int(gl[-1]) == gb.size


_SHARED = {}


def _shared(n, d, nq):
    """(base, queries, radii: 0, the median 10th-nearest distance over the whole store, +inf), computed once."""
    if (n, d, nq) not in _SHARED:
        base = vr.make_base(n, d)
        q = vr.make_queries(nq, d, base)
        kth = fr.search(base, q[:64], 10, np.ones(n, bool))[0][:, -1]
        _SHARED[n, d, nq] = (base, q, (F(0), F(np.median(kth)), F(np.inf)))
    return _SHARED[n, d, nq]


def _check_state(g, bvals):
    """base_values_info and base_value_rows against numpy, over the cross product of DESIGN.md 3.24's boundary values."""
    n = bvals.size
    assert g.base_values_info() == (int((bvals != vr.NONE).sum()), n)
    for lo in vr.EDGES:
        for hi in vr.EDGES:
            assert g.base_value_rows(lo, hi) == int(vr.value_mask(bvals, lo, hi).sum()) * (lo <= hi), (lo, hi)
    for lo, hi in vr.pool(n):
        assert g.base_value_rows(int(lo), int(hi)) == int(vr.value_mask(bvals, lo, hi).sum()), (lo, hi)


def _install(g, bvals):
    g.set_base_values(np.arange(bvals.size, dtype=np.uint32), bvals)


def _per_interval_plain(g2, bvals, q, qr, k, radii):
    """(B): what the parent commit's calls answer, interval by interval, put back in the caller's order."""
    nq = q.shape[0]
    out_d = np.full((nq, k), exact_ref.FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    rng_q = [[None] * nq for _ in radii]
    for lo, hi, idx in vr._distinct(qr):
        g2.set_base_filter(np.flatnonzero(vr.value_mask(bvals, lo, hi)).astype(np.uint32))  # nothing inside: the empty allow set
        out_d[idx], out_l[idx] = g2.exact_search(q[idx], k)
        for r, radius in enumerate(radii):
            lims, d, l = g2.exact_range_search(q[idx], radius)
            for j, qi in enumerate(idx):
                rng_q[r][qi] = (d[int(lims[j]):int(lims[j + 1])], l[int(lims[j]):int(lims[j + 1])])
    g2.clear_base_filter()
    ranges = []
    for per_q in rng_q:
        lims = np.zeros(nq + 1, np.uint64)
        lims[1:] = np.cumsum([p[0].size for p in per_q], dtype=np.uint64)
        ranges.append((lims, np.concatenate([p[0] for p in per_q]), np.concatenate([p[1] for p in per_q])))
    return (out_d, out_l), ranges


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k,nq,assign,splits,use_map", vr.grid())
def test_value_calls_equal_the_restatement_and_the_per_interval_calls(gpu, n, d, k, nq, assign, splits, use_map):
    base, q, radii = _shared(n, d, nq)
    bvals = vr.base_values(n)
    qr = vr.assignment(assign, n, nq)
    g = gpu()
    g.upload_base(base)
    g.set_option("exact_splits", splits)
    g.set_option("exact_range_map", use_map)
    _install(g, bvals)
    want = vr.search_blocked(base, q, k, bvals, qr)
    _same(g.exact_search_values(q, k, qr), want)  # (A)
    want_r = [vr.range_blocked(base, q, r, bvals, qr) for r in radii]
    for r, w in zip(radii, want_r):
        _same_range(g.exact_range_search_values(q, r, qr), w)
    assert int(want_r[0][0][-1]) == 0 and int(want_r[2][0][-1]) == sum(int(vr.value_mask(bvals, lo, hi).sum()) for lo, hi in qr)
    g2 = gpu()
    g2.upload_base(base)
    g2.set_option("exact_splits", splits)
    g2.set_option("exact_range_map", use_map)
    b_k, b_r = _per_interval_plain(g2, bvals, q, qr, k, radii)  # (B)
    _same(want, b_k)
    for w, b in zip(want_r, b_r):
        _same_range(w, b)
    # query_ranges None is the plain call, and so is (0, 0xffffffff) for every query
    _same(g.exact_search_values(q, k, None), g2.exact_search(q, k))
    _same(g.exact_search_values(q, k, np.tile(np.array(vr.FULL, np.uint32), (nq, 1))), g2.exact_search(q, k))
    _same_range(g.exact_range_search_values(q, radii[1], None), g2.exact_range_search(q, radii[1]))
    g.close()
    g2.close()


# ---- 2. ties at the k-th distance arrive in value order, not in label order ---------------------------------------------------
@pytest.mark.parametrize("d,splits", [(16, 1), (128, 3), (48, 64)])
def test_tie_block_returns_its_lowest_rows(gpu, d, splits):
    n, nq = vr.BIG_N, 40
    base = vr.make_base(n, d)
    t0, tn = vr.tie_block(n)
    assert tn >= 300
    q = np.repeat(base[t0:t0 + 1], nq, 0)  # every query equals the block: tn rows at distance 0, highest row first in value order
    bvals = vr.base_values(n)
    ivs = [(vr.TIE_TOP, vr.TIE_TOP + tn - 1), (vr.TIE_TOP + 10, vr.TIE_TOP + tn - 1), (vr.TIE_TOP, vr.TIE_TOP + 149),
           (1, 0xfffffffd), vr.VALUED, vr.FULL, (vr.TIE_TOP + 7, vr.TIE_TOP + 11)]
    qr = np.array(ivs, np.uint32)[np.arange(nq) % len(ivs)]
    g = gpu()
    g.upload_base(base)
    g.set_option("exact_splits", splits)
    _install(g, bvals)
    for k in (1, 10, 100):
        gd, gl = g.exact_search_values(q, k, qr)
        _same((gd, gl), vr.search_blocked(base, q, k, bvals, qr))
        for i, (lo, hi) in enumerate(qr):
            rows = np.flatnonzero(vr.value_mask(bvals, lo, hi) & (np.arange(n) >= t0) & (np.arange(n) < t0 + tn))
            m = min(k, rows.size)
            assert gl[i, :m].tolist() == rows[:m].tolist() and (gd[i, :m] == 0).all(), (k, i)
    # ... and the range results of a query are in ascending label
    lims, dd, ll = g.exact_range_search_values(q, F(1), qr)
    _same_range((lims, dd, ll), vr.range_blocked(base, q, F(1), bvals, qr))
    for i in range(nq):
        assert (np.diff(ll[int(lims[i]):int(lims[i + 1])]) > 0).all()
    g.close()


# ---- 3. more than one chunk ----------------------------------------------------------------------------------------------------
def test_range_search_over_more_than_one_chunk(gpu):
    n, d, nq = vr.BIG_N, 16, 16500  # crosses the 16384 queries of a chunk
    base = vr.make_base(n, d)
    q = vr.make_queries(nq, d, base)
    bvals = vr.base_values(n)
    P = vr.pool(n)
    qr = P[np.random.default_rng(5).integers(0, len(P), nq)]
    dist = exact_ref.distances(base, q[:64])
    radius = F(np.sort(dist, axis=None)[dist.size // 50])
    g = gpu()
    g.upload_base(base)
    _install(g, bvals)
    want = vr.range_blocked(base, q, radius, bvals, qr)
    assert int(want[0][-1]) > 1000
    for use_map in (0, 1):
        g.set_option("exact_range_map", use_map)
        _same_range(g.exact_range_search_values(q, radius, qr), want)
    _same(g.exact_search_values(q, 10, qr), vr.search_blocked(base, q, 10, bvals, qr))  # two chunks of the k-search as well
    g.close()


# ---- 4. the device forms -------------------------------------------------------------------------------------------------------
def test_dev_forms_with_misaligned_queries_and_a_row_stride(gpu):
    n, d, k, nq = vr.BIG_N, 48, 10, 300
    base, q, radii = _shared(n, d, nq)
    bvals = vr.base_values(n)
    qr = vr.assignment("absent", n, nq)
    g = gpu()
    g.upload_base(base)
    dev = torch.device("cuda:0")
    d_rows = torch.arange(n, dtype=torch.int32, device=dev)
    d_vals = torch.from_numpy(bvals.view(np.int32)).to(dev)
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    g.set_base_values_dev(n, d_rows, d_vals)
    _check_state(g, bvals)
    host_k = g.exact_search_values(q, k, qr)
    host_r = g.exact_range_search_values(q, radii[1], qr)
    _same(host_k, vr.search_blocked(base, q, k, bvals, qr))
    # the queries at an odd address, d + 4 bytes apart
    stride = d + 4
    raw = torch.zeros(nq * stride + 16, dtype=torch.uint8, device=dev)
    raw[3:3 + nq * stride].view(nq, stride)[:, :d] = torch.from_numpy(q).to(dev)
    dq = raw.data_ptr() + 3
    dr = torch.from_numpy(qr.view(np.int32)).to(dev)
    od, ol = torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    g.exact_search_values_dev(nq, dq, stride, k, dr, od, ol)
    g.sync()
    _same((od.cpu().numpy(), ol.cpu().numpy()), host_k)
    dl = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    total = g.exact_range_search_values_dev(nq, dq, stride, dr, float(radii[1]), dl)
    _same_range((dl.cpu().numpy().view(np.uint64), *g.exact_range_results(0, total)), host_r)
    g.close()


# ---- 5. incremental sets -------------------------------------------------------------------------------------------------------
def test_incremental_sets_revalue_and_unvalue(gpu):
    n, d, k, nq = vr.BIG_N, 16, 10, 129
    base, q, radii = _shared(n, d, nq)
    bvals = vr.base_values(n)
    qr = vr.assignment("interleaved", n, nq)
    rows = np.arange(n, dtype=np.uint32)
    one, three = gpu(), gpu()
    one.upload_base(base)
    three.upload_base(base)
    one.set_base_values(rows, bvals)
    _check_state(one, bvals)
    perm = np.random.default_rng(3).permutation(n)  # in three calls of scattered rows, with rows beyond the store and repeats
    state = None
    for part in np.array_split(perm, 3):
        r = np.concatenate([rows[part], rows[part][:5], np.array([n, n + 100], np.uint32)])
        v = np.concatenate([bvals[part], bvals[part][:5], np.array([1, 2], np.uint32)])
        three.set_base_values(r, v)
        state = vr.apply_sets(n, [(r, v)], state)
        assert three.base_values_info() == (int((state != vr.NONE).sum()), n)
    assert np.array_equal(state, bvals)
    _check_state(three, bvals)
    want = vr.search_blocked(base, q, k, bvals, qr)
    _same(one.exact_search_values(q, k, qr), want)
    _same(three.exact_search_values(q, k, qr), want)
    _same_range(three.exact_range_search_values(q, radii[1], qr), vr.range_blocked(base, q, radii[1], bvals, qr))
    # re-value a row of value 0 into the band, un-value a tied row, value a valueless one
    free = int(np.flatnonzero(bvals == vr.NONE)[0])
    calls = [(np.array([10, 0, free], np.uint32), np.array([0x80000000, vr.NONE, 77], np.uint32))]
    three.set_base_values(*calls[0])
    now = vr.apply_sets(n, calls, bvals)
    _check_state(three, now)
    qv = np.array([(0, 0), (0x80000000, 0x80000000), vr.FULL, (77, 77), vr.VALUED], np.uint32)[np.arange(nq) % 5]
    _same(three.exact_search_values(q, k, qv), vr.search_blocked(base, q, k, now, qv))
    _same_range(three.exact_range_search_values(q, radii[2], qv), vr.range_blocked(base, q, radii[2], now, qv))
    _same(one.exact_search_values(q, k, qv), vr.search_blocked(base, q, k, bvals, qv))  # the other handle's store: untouched
    # every row un-valued again: the arrays stay, no row holds a value
    none = np.full(n, vr.NONE, np.uint32)
    three.set_base_values(rows, none)
    _check_state(three, none)
    _same(three.exact_search_values(q, k, qv), vr.search_blocked(base, q, k, none, qv))
    one.close()
    three.close()
