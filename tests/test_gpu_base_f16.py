"""The float16 base store (ivfhnsw_gpu_upload_base_f16): its exact search on the f16 matrix cores against
int64 numpy where every operation is exact and against float64 within the documented bound where it is not, the re-rank
against it bit for bit, and the upload's chunks, strides and refusals."""
import itertools

import numpy as np
import pytest

import exact_ref
import rerank_ref

pytestmark = pytest.mark.gpu


def _same(got, want):
    assert np.array_equal(got[1], want[1]), np.nonzero((got[1] != want[1]).any(1))[0][:5]
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def _ints(seed, n, nq, d):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 128, (n, d), dtype=np.uint8), rng.integers(0, 128, (nq, d), dtype=np.uint8)


# ---- 1. integers 0..127: 256 * 127^2 * 2 < 2^24, so norms, dot product and their combination are exact in any order
_STORES, _WANT = {}, {}


@pytest.fixture(scope="module")
def int_store(pkg):
    """(rows, queries, handle) per (d, n), uploaded once and shared by the cases below; closed with the module."""
    def get(d, n):
        if (d, n) not in _STORES:
            x, q = _ints(100 * d + n, n, 129, d)
            q[0] = x[n // 2]  # a zero distance
            g = pkg.GpuIndex(0)
            g.upload_base_f16(x.astype(np.float32))
            assert g.base_kind() == pkg.BASE_F16
            _STORES[d, n] = x, q, g
        return _STORES[d, n]
    yield get
    for _, _, g in _STORES.values():
        g.close()
    _STORES.clear()


@pytest.mark.parametrize("d,n,nq,k,splits", list(itertools.product((16, 96, 128, 256), (7, 31, 33, 1000, 4133), (1, 33, 129),
                                                                   (1, 32, 33, 100), (1, 3))))
def test_integer_rows_give_the_integer_order(int_store, d, n, nq, k, splits):
    x, q, g = int_store(d, n)
    if (d, n, k) not in _WANT:
        _WANT[d, n, k] = exact_ref.search(x, q, k)
    want = _WANT[d, n, k]
    g.set_option("exact_splits", splits)
    _same(g.exact_search_f16(q[:nq].astype(np.float32), k), (want[0][:nq], want[1][:nq]))


def test_scaled_rows_are_exact_too(pkg):
    x, q = _ints(5, 1000, 33, 96)
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x.astype(np.float32) / 16)
    want = exact_ref.search(x, q, 33)
    _same(g.exact_search_f16(q.astype(np.float32) / 16, 33), (want[0] / 256, want[1]))
    g.close()


def test_equal_distances_come_in_ascending_label(pkg):
    rows, q = _ints(6, 8, 33, 128)
    x = np.tile(rows, (125, 1))  # 1000 rows, every distance 125 times, across tiles and splits
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x.astype(np.float32))
    for splits in (1, 3):
        g.set_option("exact_splits", splits)
        _same(g.exact_search_f16(q.astype(np.float32), 100), exact_ref.search(x, q, 100))
    g.close()


# ---- 2. real values against float64, within tol(q, x) = (d + 3) 2^-23 (|q^| + |x^|)^2
_REAL = {}


def _real(d):
    if d not in _REAL:
        rng = np.random.default_rng(d)
        x, q = rng.standard_normal((4133, d), dtype=np.float32), rng.standard_normal((129, d), dtype=np.float32)
        xh, qh = x.astype(np.float16).astype(np.float64), q.astype(np.float16).astype(np.float64)
        xn, qn = (xh * xh).sum(1), (qh * qh).sum(1)
        D = qn[:, None] + xn[None, :] - 2.0 * (qh @ xh.T)
        tol = (d + 3) * 2.0 ** -23 * (np.sqrt(qn)[:, None] + np.sqrt(xn)[None, :]) ** 2
        _REAL[d] = x, q, D, tol
    return _REAL[d]


@pytest.mark.parametrize("d,k", [(96, 1), (96, 100), (256, 1), (256, 100)])
def test_real_rows_within_the_bound_of_float64(pkg, d, k):
    x, q, D, tol = _real(d)
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x)
    dist, lab = g.exact_search_f16(q, k)
    g.close()
    assert lab.min() >= 0 and (np.diff(dist, axis=1) >= 0).all()
    rows = np.arange(len(q))[:, None]
    err = np.abs(dist.astype(np.float64) - D[rows, lab])
    print("d %d k %d: largest |returned - float64| / tol = %.4f" % (d, k, (err / tol[rows, lab]).max()))
    assert (err <= tol[rows, lab]).all()
    Dk = np.sort(D, axis=1)[:, k - 1:k]
    assert (D[rows, lab] <= Dk + 2 * tol[rows, lab]).all()
    returned = np.zeros(D.shape, bool)
    returned[rows, lab] = True
    assert returned[D < Dk - 2 * tol].all()
    if k == 1:
        assert np.array_equal(lab[:, 0], D.argmin(1))


# ---- 3. the re-rank: fvec_L2sqr of the unrounded query and the stored halves widened, bit for bit
# (k <= kc is the call's own rule, so kc = 1 goes with k = 1 only)
@pytest.mark.parametrize("d,kc,k", [(d, kc, k) for d in (16, 96, 128, 256) for kc, k in ((1, 1), (100, 1), (100, 10))])
def test_rerank_against_the_half_store_is_bit_exact(pkg, d, kc, k):
    import torch
    rng = np.random.default_rng(d + kc + k)
    n, nq = 300, 9
    x, q = rng.standard_normal((n, d), dtype=np.float32) * 3, rng.standard_normal((nq, d), dtype=np.float32) * 3
    cand = rng.integers(0, n, (nq, kc)).astype(np.int64)
    cand[0, 0] = -1
    cand[1, 0] = n + 5
    cand[2, kc - 1] = cand[2, 0]
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x)
    dev = torch.device("cuda", 0)
    od, ol = torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)
    tq, tc = torch.from_numpy(q).to(dev), torch.from_numpy(cand).to(dev)
    torch.cuda.synchronize(dev)
    g.rerank_dev(nq, kc, tq, tc, k, od, ol)
    g.sync()
    _same((od.cpu().numpy(), ol.cpu().numpy()), rerank_ref.rerank(x.astype(np.float16).astype(np.float32), q, cand, k))
    g.close()


# ---- 4. upload and refusals
@pytest.mark.parametrize("case", ["chunks", "fvecs_stride", "nan", "1e6", "d24", "d272", "k0", "k101", "u8_call_on_half",
                                  "set_base_filter_on_half", "f16_call_on_u8", "f16_call_with_base_filter", "view"])
def test_upload_and_refusals(pkg, case):
    x, q = _ints(7, 100, 5, 32)
    xf, qf = x.astype(np.float32), q.astype(np.float32)
    want = exact_ref.search(x, q, 10)
    g = pkg.GpuIndex(0)

    def code(f, *a, **kw):
        with pytest.raises(pkg.IvfHnswError) as e:
            f(*a, **kw)
        return e.value.code

    if case in ("f16_call_on_u8", "f16_call_with_base_filter"):
        g.upload_base(x)
        if case == "f16_call_with_base_filter":
            g.set_base_filter(np.arange(50, dtype=np.uint32))
        assert g.base_kind() == pkg.BASE_U8
        assert code(g.exact_search_f16, qf, 10) == pkg.ERR_STATE
    elif case in ("d24", "d272"):
        assert code(g.upload_base_f16, np.zeros((4, int(case[1:])), np.float32)) == pkg.ERR_INVALID
        assert g.base_kind() == pkg.BASE_NONE
    else:
        if case == "chunks":
            for first, last in ((0, 33), (33, 34), (34, 100)):
                g.upload_base_f16(xf[first:last], n=100, first=first)
        elif case == "fvecs_stride":
            img = np.zeros((100, 33), np.float32)
            img[:, 1:] = xf
            g.upload_base_f16(img[:, 1:])
            _same(g.exact_search_f16(np.concatenate([qf[:, :1], qf], axis=1)[:, 1:], 10), want)
        else:
            g.upload_base_f16(xf)
        if case in ("nan", "1e6"):
            bad = xf[:40].copy()
            bad[39, 31] = np.nan if case == "nan" else 1e6
            assert code(g.upload_base_f16, bad, n=100, first=20) == pkg.ERR_INVALID
            assert code(g.upload_base_f16, bad) == pkg.ERR_INVALID  # (a new store is refused before the old one goes)
        elif case in ("k0", "k101"):
            assert code(g.exact_search_f16, qf, int(case[1:])) == pkg.ERR_INVALID
        elif case == "u8_call_on_half":
            assert code(g.exact_search, q, 10) == pkg.ERR_STATE
            assert code(g.exact_range_search, q, 100.0) == pkg.ERR_STATE
        elif case == "set_base_filter_on_half":
            assert code(g.set_base_filter, np.arange(50, dtype=np.uint32)) == pkg.ERR_STATE
        elif case == "view":
            v = g.view()
            assert v.base_kind() == pkg.BASE_F16
            _same(v.exact_search_f16(qf, 10), want)
            v.close()
        _same(g.exact_search_f16(qf, 10), want)
    g.close()
