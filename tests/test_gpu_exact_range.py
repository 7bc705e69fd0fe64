"""Exact range search of the uint8 base store (ivfhnsw_gpu_exact_range_search[_dev], kernels_exact.hip):
lims, labels and distance BITS against the numpy restatement (tests/exact_range_ref.py) and against the device's own
exact_search, over the step counts, tails, strip, tile, map-word and split boundaries, the call forms, the documented
errors and tools/ground_truth.py --radius end to end.  Everything is exact: no tolerance anywhere."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

from conftest import corpus
import exact_ref
import exact_range_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ground_truth  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
INF = F(np.inf)


def _base(rng, n, d):
    b = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    if n > 7:
        b[1] = b[0]          # exact ties: equal rows, so equal distances
        b[7] = b[0]
        b[n - 1] = b[3]
        b[4] = 0
        b[5] = 255
    return b


def _queries(rng, nq, d, base):
    q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
    q[0] = base[0]
    if nq > 2:
        q[1] = 0
        q[2] = 255
    return q


def _same(got, want):
    gl, gd, gb = got
    wl, wd, wb = want
    assert gl.dtype == np.uint64 and gd.dtype == np.float32 and gb.dtype == np.int64
    assert np.array_equal(gl, wl), np.nonzero(gl != wl)[0][:5]
    assert np.array_equal(gb, wb), np.nonzero(gb != wb)[0][:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _bvecs(rows):
    n, d = rows.shape
    img = np.empty((n, d + 4), np.uint8)
    img[:, :4] = np.frombuffer(np.int32(d).tobytes(), np.uint8)
    img[:, 4:] = rows
    return img


def _quantile(dist, x):
    """An occurring distance, as float32: the x quantile of the whole matrix."""
    flat = np.sort(dist, axis=None)
    return F(flat[min(flat.size - 1, int(x * flat.size))])


DS, NS, NQS = (16, 48, 96, 128, 256), (1, 31, 33, 6001), (1, 33, 129)
GRID = [(d, n, NQS[i % 3]) for i, (d, n) in enumerate(itertools.product(DS, NS))]  # every (d, n), nq cycling
assert all({c[i] for c in GRID} == set(ax) for i, ax in enumerate((DS, NS, NQS)))


# ---- 1. the grid -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,nq", GRID)
def test_exact_range_equals_the_restatement(gpu, d, n, nq):
    base = _base(np.random.default_rng(1000 * d + n), n, d)
    q = _queries(np.random.default_rng(d * 7919 + n * 31 + nq * 7), nq, d, base)
    dist = exact_ref.distances(base, q)
    g = gpu()
    g.upload_base(base)
    for r in (F(0.0), F(1.0), _quantile(dist, 0.02), _quantile(dist, 0.5), INF):
        got = g.exact_range_search(q, r)
        _same(got, exact_range_ref.from_distances(dist, r))
        if r == INF:
            assert got[0][-1] == nq * n and np.array_equal(got[2], np.tile(np.arange(n), nq))
    if n > 7:
        lims, _, lab = g.exact_range_search(q, F(1.0))
        assert lab[:int(lims[1])].tolist() == [0, 1, 7]  # query 0 is row 0: its copies, ascending label
    g.close()


# ---- 2. strict, in float ---------------------------------------------------------------------------------------------
def test_the_comparison_is_strict_and_in_float(gpu):
    rng = np.random.default_rng(53)
    n, d, nq = 6001, 128, 8
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    dist = exact_ref.distances(base, q)
    D = int(np.sort(dist[3])[40])  # an occurring distance of query 3
    j = int(np.nonzero(dist[3] == D)[0][0])
    g = gpu()
    g.upload_base(base)

    def labels3(res):
        return res[2][int(res[0][3]):int(res[0][4])]
    for r, inside in ((F(D), False), (np.nextafter(F(D), INF), True), (np.nextafter(F(D), -INF), False), (F(D + 0.5), True)):
        got = g.exact_range_search(q, r)
        _same(got, exact_range_ref.from_distances(dist, r))
        assert (j in labels3(got)) == inside, float(r)
    for r in (F(-1.0), -INF, F(-0.0)):
        lims, dd, lab = g.exact_range_search(q, r)
        assert lims.shape == (nq + 1,) and not lims.any() and dd.size == 0 and lab.size == 0
        assert g.exact_range_results_dev() == (0, 0, 0)
        g.exact_range_results(0, 0)
    g.close()


# ---- 3. tile, map-word and split boundaries --------------------------------------------------------------------------
def test_hits_at_tile_word_and_split_boundaries(gpu):
    rng = np.random.default_rng(59)
    n, d, nq = 6001, 16, 40
    base = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
    # copies of query 0's vector at the ends of tiles, of the first map word and of the store; query 39's at rows 0 and
    # n - 1.  n - 1 IS row 6000, so the two queries share one vector: the first row of the first strip and the last row of
    # the partial second strip each have to return all eight
    q[39] = q[0]
    planted = [0, 31, 32, 1023, 1024, 1025, 3000, 6000]
    base[planted] = q[0]
    want = exact_range_ref.search(base, q, 1.0)
    assert want[2][:int(want[0][1])].tolist() == planted
    assert want[2][int(want[0][39]):].tolist() == planted and want[0][-1] == 16
    g = gpu()
    g.upload_base(base)
    dense = exact_range_ref.search(base, q, 170000.0)
    for s in (-1, 1, 2, 7, 64):  # with 64 most splits are shorter than one map word
        g.set_option("exact_splits", s)
        for use_map in (1, 0, -1):  # the second pass by the tile map, and as a whole sweep: the same arrays
            g.set_option("exact_range_map", use_map)
            _same(g.exact_range_search(q, 1.0), want)
            _same(g.exact_range_search(q, 170000.0), dense)
    g.set_option("exact_splits", -1)
    g.close()


# ---- 4. default splits -------------------------------------------------------------------------------------------------
def test_default_splits_on_a_store_that_needs_them(gpu):
    rng = np.random.default_rng(61)
    n, d, nq = 200_003, 128, 7
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    dist = exact_ref.distances(base, q)
    r = _quantile(dist, 0.001)
    g = gpu()
    g.upload_base(base)
    got = g.exact_range_search(q, r)
    assert got[0][-1] >= nq * n // 1000
    _same(got, exact_range_ref.from_distances(dist, r))
    g.close()


# ---- 5. more queries than one pass ---------------------------------------------------------------------------------------
def test_more_queries_than_one_pass_holds(gpu):
    rng = np.random.default_rng(67)
    n, d, nq = 33, 16, 16384 + 5
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    dist = exact_ref.distances(base, q)
    r = _quantile(dist, 0.5)
    g = gpu()
    g.upload_base(base)
    _same(g.exact_range_search(q, r), exact_range_ref.from_distances(dist, r))
    g.close()


def test_a_coarsened_tile_map_gives_the_same_arrays(gpu):
    """So many queries on so small a store that one bit per tile would exceed a sixteenth of the store: 66 tiles in one
    split and 264 strips of 32 queries make 3168 bytes at one bit per tile and 2112 at one per two tiles against the
    2100 allowed, so a bit stands for FOUR tiles, and the second pass has to visit whole groups and skip whole groups."""
    rng = np.random.default_rng(69)
    n, d, nq = 2100, 16, 8416 + 5
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    dist = exact_ref.distances(base, q)
    g = gpu()
    g.upload_base(base)
    for r in (F(1.0), _quantile(dist, 0.002), _quantile(dist, 0.3)):
        want = exact_range_ref.from_distances(dist, r)
        for use_map in (1, 0):
            g.set_option("exact_range_map", use_map)
            _same(g.exact_range_search(q, r), want)
    g.close()


# ---- 6. against exact_search -------------------------------------------------------------------------------------------
def test_the_range_result_starts_with_the_k_nearest(gpu):
    rng = np.random.default_rng(71)
    n, d, nq, k = 4096, 128, 20, 100
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    g = gpu()
    g.upload_base(base)
    kd, kl = g.exact_search(q, k)
    for i in range(nq):
        lims, dd, lab = g.exact_range_search(q[i:i + 1], np.nextafter(kd[i, k - 1], INF))
        assert lims[1] >= k and (np.diff(lab) > 0).all()
        order = np.lexsort((lab, dd))[:k]  # by (distance, label)
        assert np.array_equal(lab[order], kl[i])
        assert np.array_equal(dd[order].view(np.uint32), kd[i].view(np.uint32))
    g.close()


# ---- 7. call forms -----------------------------------------------------------------------------------------------------
SMALL_IVF = dict(seed=7, nc=128, d=128, M=16, n_base=8000, nq=32, efConstruction=100)


class _DeviceArray:
    """A raw device address as something torch.as_tensor takes."""
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _upload_ivf(g, c):
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"])
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)


def test_call_forms_views_and_the_life_of_the_results(gpu):
    import torch
    rng = np.random.default_rng(73)
    n, d, nq = 3001, 128, 40
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    dist = exact_ref.distances(base, q)
    r = _quantile(dist, 0.05)
    want = exact_range_ref.from_distances(dist, r)
    total = int(want[0][-1])
    g = gpu()
    # the device form on .bvecs images (stride d + 4, pointers 4 bytes past a boundary), queued behind the upload
    tb = torch.from_numpy(_bvecs(base).reshape(-1)).cuda()
    tq = torch.from_numpy(_bvecs(q).reshape(-1)).cuda()
    tl = torch.full((nq + 1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g.upload_base_dev(n, d, 0, n, tb[4:], row_stride=d + 4)
    before = g.memory_bytes()
    assert g.exact_range_search_dev(nq, tq[4:], d + 4, float(r), tl) == total
    assert g.memory_bytes() >= before + 12 * total
    lims = tl.cpu().numpy().view(np.uint64)
    _same((lims,) + g.exact_range_results(0, total), want)
    # the pointers themselves, read back through torch
    pd, pl, tot = g.exact_range_results_dev()
    assert tot == total and pd and pl
    back_d = torch.as_tensor(_DeviceArray(pd, total, "<f4"), device="cuda")
    back_l = torch.as_tensor(_DeviceArray(pl, total, "<i8"), device="cuda")
    assert back_d.data_ptr() == pd and back_l.data_ptr() == pl  # the handle's memory itself, no copy
    _same((lims, back_d.cpu().numpy(), back_l.cpu().numpy()), want)
    # sub-ranges
    a, b = int(want[0][3]), int(want[0][11])
    sd, sl = g.exact_range_results(a, b - a)
    assert np.array_equal(sl, want[2][a:b]) and np.array_equal(sd.view(np.uint32), want[1][a:b].view(np.uint32))
    sd, sl = g.exact_range_results(total, 0)
    assert sd.size == 0 and sl.size == 0
    # the host form on the image's stride
    _same(g.exact_range_search(_bvecs(q)[:, 4:], r), want)
    # a view searches its parent's store and holds its own results; the parent's stay
    v = g.view()
    rv = _quantile(dist, 0.01)
    want_v = exact_range_ref.from_distances(dist[:9], rv)
    _same(v.exact_range_search(q[:9], rv), want_v)
    _same((want[0],) + g.exact_range_results(0, total), want)
    _same((want_v[0],) + v.exact_range_results(0, int(want_v[0][-1])), want_v)
    v.close()
    # the results survive an exact_search, an upload of the same store and an IVF range search on the same handle,
    # and that range search returns what it returns on a handle that never ran the exact call
    c = corpus(**SMALL_IVF)
    g.exact_search(q, 10)
    g.upload_base(base)
    _upload_ivf(g, c)
    kd, _ = g.search(c["queries"], 10, 8, 2000, efSearch=40)
    ivf_r = F(np.median(kd[:, 9]))
    ivf = g.range_search(c["queries"], ivf_r, 8, 2000, efSearch=40)
    assert ivf[0][-1] > 0
    _same((want[0],) + g.exact_range_results(0, total), want)
    assert g.exact_range_results_dev() == (pd, pl, total)  # the very buffers: nothing was reallocated
    _same(g.exact_range_search(q, r), want)       # ... and the other way round
    idist, ilab = g.range_results(0, int(ivf[0][-1]))
    assert np.array_equal(ilab, ivf[2]) and np.array_equal(idist.view(np.uint32), ivf[1].view(np.uint32))
    g2 = gpu()
    _upload_ivf(g2, c)
    alone = g2.range_search(c["queries"], ivf_r, 8, 2000, efSearch=40)
    _same(ivf, alone)
    g2.close()
    g.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_and_earlier_results_usable(gpu, pkg):
    rng = np.random.default_rng(79)
    n, d, nq = 500, 32, 4
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    r = F(150000.0)
    want = exact_range_ref.search(base, q, r)
    total = int(want[0][-1])
    assert 0 < total < nq * n
    g = gpu()

    def code(f, *a, **kw):
        with pytest.raises(pkg.IvfHnswError) as e:
            f(*a, **kw)
        return e.value.code

    def raw(nq_, queries, stride, radius, lims, tot):
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        return pkg.lib().ivfhnsw_gpu_exact_range_search(g._h, nq_, ptr(queries), stride, C.c_float(radius), ptr(lims),
                                                        None if tot is None else C.byref(tot))

    def held():
        _same((want[0],) + g.exact_range_results(0, total), want)

    assert code(g.exact_range_results, 0, 0) == pkg.ERR_STATE                   # before any exact range search
    assert code(g.exact_range_results_dev) == pkg.ERR_STATE
    assert code(g.exact_range_search, q, r) == pkg.ERR_STATE                    # no store
    g.upload_base(np.zeros((8, 512), np.uint8))
    assert code(g.exact_range_search, np.zeros((2, 512), np.uint8), r) == pkg.ERR_INVALID  # d > 256
    assert "256" in pkg.lib().ivfhnsw_gpu_last_error().decode()
    g.upload_base(base)
    _same(g.exact_range_search(q, r), want)
    lims, tot = np.full(nq + 1, 7, np.uint64), C.c_uint64(99)
    assert code(g.exact_range_search, q, float("nan")) == pkg.ERR_INVALID       # NaN radius
    assert raw(nq, None, d, r, lims, tot) == pkg.ERR_INVALID                    # null queries, lims, total
    assert raw(nq, q, d, r, None, tot) == pkg.ERR_INVALID
    assert raw(nq, q, d, r, lims, None) == pkg.ERR_INVALID
    assert raw(nq, q, d - 1, r, lims, tot) == pkg.ERR_INVALID                   # row_stride < d
    many = np.zeros(((1 << 17) + 1, d), np.uint8)
    assert code(g.exact_range_search, many, r) == pkg.ERR_INVALID               # more than 131 072 queries
    assert "131072" in pkg.lib().ivfhnsw_gpu_last_error().decode()
    assert (lims == 7).all() and tot.value == 99                                # nothing was written
    assert code(g.exact_range_results, total, 1) == pkg.ERR_INVALID             # beyond the total
    assert code(g.exact_range_results, total + 1, 0) == pkg.ERR_INVALID
    held()
    assert raw(0, None, d, r, lims, tot) == pkg.OK and lims[0] == 0 and tot.value == 0  # nq = 0
    assert raw(0, None, d, r, None, None) == pkg.OK
    assert g.exact_range_results_dev() == (0, 0, 0)
    _same(g.exact_range_search(q, r), want)

    # the 2^32 limit: 32 768 rows x 131 072 queries, every pair within +inf, is exactly 2^32 results
    g.upload_base(np.zeros((1 << 15, 16), np.uint8))
    small = np.zeros((3, 16), np.uint8)
    want = exact_range_ref.search(np.zeros((1 << 15, 16), np.uint8), small, 1.0)
    total = int(want[0][-1])
    _same(g.exact_range_search(small, 1.0), want)
    before = g.memory_bytes()
    assert code(g.exact_range_search, np.zeros((1 << 17, 16), np.uint8), INF) == pkg.ERR_INVALID
    assert "2^32" in pkg.lib().ivfhnsw_gpu_last_error().decode()
    assert g.memory_bytes() < before + (1 << 30)  # counts and map grew, by far less than 12 bytes x 2^32 of results
    held()
    _same(g.exact_range_search(small, 1.0), want)
    g.close()


# ---- 9. the tool -------------------------------------------------------------------------------------------------------
def test_ground_truth_tool_range_mode_end_to_end(gpu, tmp_path):
    rng = np.random.default_rng(83)
    n, d, nq = 3001, 128, 25
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    dist = exact_ref.distances(base, q)
    r = _quantile(dist, 0.01)
    bp, qp, out = (str(tmp_path / f) for f in ("base.bvecs", "query.bvecs", "gt.npz"))
    _bvecs(base).tofile(bp)
    _bvecs(q).tofile(qp)
    ground_truth.main(["--base", bp, "--queries", qp, "--radius", repr(float(r)), "--out", out])
    lims, dd, lab, radius = ground_truth.read_range(out)
    assert radius == float(r)
    _same((lims, dd, lab), exact_range_ref.from_distances(dist, r))
    ground_truth.main(["--base", bp, "--queries", qp, "--radius", repr(float(r)), "--out", out, "--rows", "1000", "--k", "3"])
    lims, dd, lab, _ = ground_truth.read_range(out)
    _same((lims, dd, lab), exact_range_ref.from_distances(dist[:, :1000], r))
