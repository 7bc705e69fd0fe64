"""Exact brute-force search of the uint8 base store on the int8 matrix cores (ivfhnsw_gpu_exact_search[_dev],
kernels_exact.hip): labels and distance BITS against the integer numpy restatement (tests/exact_ref.py, pinned to
fvec_L2sqr by tests/test_exact_cpu.py) and against the device's own re-rank, the split and merge path, the call forms,
the documented errors and tools/ground_truth.py end to end.  Everything is exact: no tolerance anywhere."""
import itertools
import os
import sys

import numpy as np
import pytest

import exact_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ground_truth  # noqa: E402

pytestmark = pytest.mark.gpu


def _base(rng, n, d):
    b = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    if n > 7:
        b[1] = b[0]          # exact ties: equal rows, so equal distances, ordered by label
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
    gd, gl = got
    wd, wl = want
    assert gl.dtype == np.int64 and gd.dtype == np.float32
    assert np.array_equal(gl, wl), np.nonzero((gl != wl).any(1))[0][:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _bvecs(rows):
    n, d = rows.shape
    img = np.empty((n, d + 4), np.uint8)
    img[:, :4] = np.frombuffer(np.int32(d).tobytes(), np.uint8)
    img[:, 4:] = rows
    return img


DS, NS, NQS, KS = (16, 48, 96, 128, 256), (1, 31, 33, 6001), (1, 33, 129), (1, 10, 100)


def _grid():
    cases = []
    for i, (d, n) in enumerate(itertools.product(DS, NS)):  # every (d, n), nq and k cycling through their values
        cases.append((d, n, NQS[i % 3], KS[(i + i // 3) % 3]))
    for d in (16, 128):  # every (nq, k) where a row strip, a k step and a tile boundary meet
        cases += [(d, 6001, nq, k) for nq in NQS for k in KS]
    for d in DS:  # k = 100 (the 64-row strips) and k > n for every step count
        cases += [(d, 6001, 129, 100), (d, 33, 33, 100)]
    return sorted(set(cases))


GRID = _grid()
assert all({c[i] for c in GRID} == set(ax) for i, ax in enumerate((DS, NS, NQS, KS)))

_BASES = {}


def _shared_base(d, n):
    if (d, n) not in _BASES:
        _BASES[d, n] = _base(np.random.default_rng(1000 * d + n), n, d)
    return _BASES[d, n]


@pytest.mark.parametrize("d,n,nq,k", GRID)
def test_exact_search_equals_the_restatement(gpu, d, n, nq, k):
    base = _shared_base(d, n)
    q = _queries(np.random.default_rng(d * 7919 + n * 31 + nq * 7 + k), nq, d, base)
    g = gpu()
    g.upload_base(base)
    got = g.exact_search(q, k)
    _same(got, exact_ref.search(base, q, k))
    if k > n:
        assert (got[1][:, n:] == -1).all() and (got[0][:, n:] == exact_ref.FLT_MAX).all()
    g.close()


@pytest.mark.parametrize("k", (1, 100))
def test_exact_search_equals_the_rerank_over_every_row(gpu, k):
    rng = np.random.default_rng(17)
    n, d, nq = 4096, 128, 20
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    g = gpu()
    g.upload_base(base)
    cand = np.tile(np.arange(n, dtype=np.int64), (nq, 1))
    _same(g.exact_search(q, k), g.rerank(q.astype(np.float32), cand, k))
    g.close()


def test_every_split_count_gives_the_same_arrays(gpu):
    rng = np.random.default_rng(23)
    n, d, nq, k = 6001, 128, 5, 100
    base = _base(rng, n, d)
    base[3000] = base[0]
    base[6000] = base[0]
    q = _queries(rng, nq, d, base)
    want = exact_ref.search(base, q, k)
    assert want[1][0, :5].tolist() == [0, 1, 7, 3000, 6000]  # the planted copies, one per region of the store
    g = gpu()
    g.upload_base(base)
    _same(g.exact_search(q, k), want)
    for s in (1, 2, 7, 64):
        g.set_option("exact_splits", s)
        _same(g.exact_search(q, k), want)
        _same(g.exact_search(q, 1), exact_ref.search(base, q, 1))
    g.set_option("exact_splits", -1)
    _same(g.exact_search(q, k), want)
    g.close()


def test_default_splits_on_a_store_that_needs_them(gpu):
    rng = np.random.default_rng(29)
    n, d, nq, k = 200_003, 128, 7, 100
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    g = gpu()
    g.upload_base(base)
    _same(g.exact_search(q, k), exact_ref.search(base, q, k))
    g.close()


def test_more_queries_than_one_pass_holds(gpu):
    rng = np.random.default_rng(31)
    n, d, nq, k = 33, 16, 16384 + 5, 1
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    g = gpu()
    g.upload_base(base)
    _same(g.exact_search(q, k), exact_ref.search(base, q, k))
    g.close()


def test_dev_form_on_a_bvecs_image_view_and_missing_chunk(gpu):
    import torch
    rng = np.random.default_rng(37)
    n, d, nq, k = 3001, 128, 40, 10
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    want = exact_ref.search(base, q, k)
    g = gpu()
    before = g.memory_bytes()
    # the device form: base and queries straight from .bvecs images (stride d + 4, pointers 4 bytes past a boundary),
    # the search queued right behind the upload on the handle's stream
    tb = torch.from_numpy(_bvecs(base).reshape(-1)).cuda()
    tq = torch.from_numpy(_bvecs(q).reshape(-1)).cuda()
    od = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    ol = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g.upload_base_dev(n, d, 0, n, tb[4:], row_stride=d + 4)
    g.exact_search_dev(nq, tq[4:], d + 4, k, od, ol)
    g.sync()
    _same((od.cpu().numpy(), ol.cpu().numpy()), want)
    assert g.memory_bytes() > before + n * d  # the store and the search's workspace are counted
    # the host form takes the image's stride too
    _same(g.exact_search(_bvecs(q)[:, 4:], k), want)
    # a view searches its parent's store
    v = g.view()
    _same(v.exact_search(q, k), want)
    v.close()
    # a store uploaded in chunks with one chunk missing: its rows are zeros, and valid rows
    holed = base.copy()
    holed[700:1400] = 0
    for first in range(0, n, 700):
        if first != 700:
            m = min(700, n - first)
            g.upload_base(base[first:first + m], n=n, first=first)
    _same(g.exact_search(q, k), exact_ref.search(holed, q, k))
    g.close()


def test_errors_leave_the_handle_usable(gpu, pkg):
    import ctypes as C
    rng = np.random.default_rng(41)
    n, d, nq, k = 500, 32, 4, 5
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    want = exact_ref.search(base, q, k)
    g = gpu()

    def code(f, *a, **kw):
        with pytest.raises(pkg.IvfHnswError) as e:
            f(*a, **kw)
        return e.value.code

    def raw(nq_, queries, stride, k_, dist, lab):
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        return pkg.lib().ivfhnsw_gpu_exact_search(g._h, nq_, ptr(queries), stride, k_, ptr(dist), ptr(lab))

    assert code(g.exact_search, q, k) == pkg.ERR_STATE                        # no store
    g.upload_base(np.zeros((8, 512), np.uint8))
    assert code(g.exact_search, np.zeros((2, 512), np.uint8), 1) == pkg.ERR_INVALID  # d > 256: not exact in float
    assert "256" in pkg.lib().ivfhnsw_gpu_last_error().decode()
    g.upload_base(base)
    _same(g.exact_search(q, k), want)
    assert code(g.exact_search, q, 0) == pkg.ERR_INVALID                      # k = 0
    assert code(g.exact_search, q, 101) == pkg.ERR_INVALID                    # k > 100
    dist, lab = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
    assert raw(nq, q, d - 1, k, dist, lab) == pkg.ERR_INVALID                 # row_stride < d
    assert raw(nq, None, d, k, dist, lab) == pkg.ERR_INVALID                  # null buffers
    assert raw(nq, q, d, k, None, lab) == pkg.ERR_INVALID
    assert raw(nq, q, d, k, dist, None) == pkg.ERR_INVALID
    assert raw(0, None, d, k, None, None) == pkg.OK                           # nq = 0 does nothing
    assert code(g.set_option, "exact_splits", 0) == pkg.ERR_INVALID           # neither -1 nor 1..64
    assert code(g.set_option, "exact_splits", 65) == pkg.ERR_INVALID
    _same(g.exact_search(q, k), want)                                         # still usable, store untouched
    g.upload_base(np.zeros((0, d), np.uint8), n=0)                            # n = 0 frees the store
    assert code(g.exact_search, q, k) == pkg.ERR_STATE
    g.upload_base(base)
    _same(g.exact_search(q, k), want)
    g.close()


def test_ground_truth_tool_end_to_end(gpu, tmp_path):
    rng = np.random.default_rng(43)
    n, d, nq, k = 3001, 128, 25, 100
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    bp, qp, out = (str(tmp_path / f) for f in ("base.bvecs", "query.bvecs", "gt.ivecs"))
    _bvecs(base).tofile(bp)
    _bvecs(q).tofile(qp)
    ground_truth.main(["--base", bp, "--queries", qp, "--k", str(k), "--out", out])
    assert np.array_equal(ground_truth.read_ivecs(out), exact_ref.search(base, q, k)[1])
    ground_truth.main(["--base", bp, "--queries", qp, "--k", "1", "--out", out, "--rows", "1000"])
    assert np.array_equal(ground_truth.read_ivecs(out), exact_ref.search(base[:1000], q, 1)[1])
