"""Exact range search of the float16 base store (ivfhnsw_gpu_exact_range_search_f16): bit for bit against
exact_range_ref where every operation is exact, with and without the tile map; the bits of exact_search_f16 on real rows;
float64 within the documented bound; refusals."""
import ctypes as C
import itertools

import numpy as np
import pytest

import exact_ref
import exact_range_ref
from test_gpu_base_f16 import _ints, _real

pytestmark = pytest.mark.gpu


def _same(got, want):
    assert np.array_equal(got[0], want[0]), np.nonzero(got[0] != want[0])[0][:5]
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


# ---- 1. integers 0..127: every operation is exact, the result is exact_range_ref's
_STORES = {}


@pytest.fixture(scope="module")
def int_store(pkg):
    """(int64 distances, queries, handle) per (d, n), uploaded once and shared by the cases below; closed with the module."""
    def get(d, n):
        if (d, n) not in _STORES:
            x, q = _ints(100 * d + n, n, 129, d)
            q[0] = x[n // 2]  # a zero distance
            g = pkg.GpuIndex(0)
            g.upload_base_f16(x.astype(np.float32))
            _STORES[d, n] = exact_ref.distances(x, q), q.astype(np.float32), g
        return _STORES[d, n]
    yield get
    for _, _, g in _STORES.values():
        g.close()
    _STORES.clear()


@pytest.mark.parametrize("d,n,nq,splits,use_map", list(itertools.product((16, 96, 256), (7, 33, 1000, 4133), (1, 33, 129),
                                                                         (1, 3), (0, 1))))
def test_integer_rows_are_exact(int_store, d, n, nq, splits, use_map):
    D, q, g = int_store(d, n)
    g.set_option("exact_splits", splits)
    g.set_option("exact_range_map", use_map)
    low = float(np.sort(D[:nq], axis=None)[nq * n // 100])  # the lower 1 % quantile: an integer some pairs sit ON (strict <)
    for radius in (low, low + 0.5) + ((np.inf,) if n == 33 else ()):
        _same(g.exact_range_search_f16(q[:nq], radius), exact_range_ref.from_distances(D[:nq], radius))


# ---- 2. a handful of near rows in a far store: whole tiles are skipped, by all four waves or by none
def test_sparse_hits_with_and_without_the_map(pkg):
    rng = np.random.default_rng(2)
    n, nq, d = 4133, 129, 128
    x = rng.integers(100, 128, (n, d), dtype=np.uint8)
    q = rng.integers(0, 4, (nq, d), dtype=np.uint8)
    # (row, query): the first, a middle and the last tile, in three different splits of 1408 columns, for queries of three
    # different waves and of both workgroups
    for row, qi in ((3, 0), (31, 40), (2000, 100), (2001, 128), (4132, 70)):
        x[row] = q[qi]
        x[row, 0] += 2
    want = exact_range_ref.search(x, q, 50.0)
    assert want[0][-1] >= 5
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x.astype(np.float32))
    g.set_option("exact_splits", 3)
    for use_map in (1, 0):
        g.set_option("exact_range_map", use_map)
        _same(g.exact_range_search_f16(q.astype(np.float32), 50.0), want)
    g.close()


# ---- 3. real rows: the pairs and the bits of exact_search_f16, wherever a column falls in a tile or split
@pytest.mark.parametrize("d", [96, 256])
def test_same_bits_as_the_k_search(pkg, d):
    rng = np.random.default_rng(d)
    n, nq = 100, 33
    x, q = rng.standard_normal((n, d), dtype=np.float32), rng.standard_normal((nq, d), dtype=np.float32)
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x)
    dist, lab = g.exact_search_f16(q, n)
    by_label = np.empty_like(dist)
    by_label[np.arange(nq)[:, None], lab] = dist
    radius = float(np.median(dist))
    _same(g.exact_range_search_f16(q, radius), exact_range_ref.from_distances(by_label, radius))
    g.close()


# ---- 4. real rows against float64, within tol(q, x) = (d + 3) 2^-23 (|q^| + |x^|)^2
def test_real_rows_within_the_bound_of_float64(pkg):
    x, q, D, tol = _real(96)
    radius = 120.0
    undecided = int((np.abs(D - radius) <= tol).sum())
    assert undecided < 0.01 * (D < radius - tol).sum(), undecided
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x)
    lims, dist, lab = g.exact_range_search_f16(q, radius)
    g.close()
    qi = np.repeat(np.arange(len(q)), np.diff(lims).astype(np.int64))
    returned = np.zeros(D.shape, bool)
    returned[qi, lab] = True
    assert returned.sum() == len(lab) and returned[D < radius - tol].all() and not returned[D > radius + tol].any()
    err = np.abs(dist.astype(np.float64) - D[qi, lab])
    print("undecided %d of %d returned; largest |returned - float64| / tol = %.4f" % (undecided, len(lab), (err / tol[qi, lab]).max()))
    assert (err <= tol[qi, lab]).all()
    assert ((np.diff(lab) > 0) | (np.diff(qi) > 0)).all()  # ascending label inside a query


# ---- 5. refusals and state
@pytest.mark.parametrize("case", ["u8_store", "no_store", "nan", "row_stride", "nq0", "dev"])
def test_refusals_and_state(pkg, case):
    x, q = _ints(7, 100, 5, 32)
    xf, qf = x.astype(np.float32), q.astype(np.float32)
    want = exact_range_ref.search(x, q, 70000.0)
    g = pkg.GpuIndex(0)

    def code(f, *a):
        with pytest.raises(pkg.IvfHnswError) as e:
            f(*a)
        return e.value.code

    if case in ("u8_store", "no_store"):
        if case == "u8_store":
            g.upload_base(x)
        assert code(g.exact_range_search_f16, qf, 70000.0) == pkg.ERR_STATE
    else:
        g.upload_base_f16(xf)
        _same(g.exact_range_search_f16(qf, 70000.0), want)
        if case == "nan":
            assert code(g.exact_range_search_f16, qf, np.nan) == pkg.ERR_INVALID
        elif case == "row_stride":
            lims, total = np.zeros(6, np.uint64), C.c_uint64(0)
            assert pkg.lib().ivfhnsw_gpu_exact_range_search_f16(g._h, 5, C.c_void_p(qf.ctypes.data), 31, C.c_float(70000.0),
                                                                C.c_void_p(lims.ctypes.data), C.byref(total)) == pkg.ERR_INVALID
        elif case == "nq0":
            lims, dist, lab = g.exact_range_search_f16(qf[:0], 70000.0)
            assert lims.tolist() == [0] and len(dist) == 0 and len(lab) == 0
        elif case == "dev":
            import torch
            dev = torch.device("cuda", 0)
            tq, tl = torch.from_numpy(qf).to(dev), torch.zeros(6, dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            assert g.exact_range_search_f16_dev(5, tq, 32, 70000.0, tl) == want[0][-1]
            assert np.array_equal(tl.cpu().numpy().view(np.uint64), want[0])
        if case in ("nan", "row_stride", "dev"):  # a refused call leaves the earlier results readable
            got = g.exact_range_results(0, int(want[0][-1]))
            assert np.array_equal(got[1], want[2]) and np.array_equal(got[0].view(np.uint32), want[1].view(np.uint32))
    g.close()
