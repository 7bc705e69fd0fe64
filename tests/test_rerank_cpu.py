"""CPU side of the exact re-rank (searchDisk): the numpy restatement the GPU tests compare against equals the host
library's own fvec_L2sqr bit for bit, and the new entry points exist and refuse to run without a device."""
import ctypes
import os

import numpy as np
import pytest

import rerank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTLIB = os.path.join(ROOT, "ivf-hnsw_amd", "libivfhnsw.so")


def _host_fvec_l2sqr():
    assert os.path.exists(HOSTLIB), "run __graft_entry__.build()"
    f = ctypes.CDLL(HOSTLIB)._ZN7ivfhnsw10fvec_L2sqrEPKfS1_m  # ivfhnsw::fvec_L2sqr(const float*, const float*, size_t)
    f.restype = ctypes.c_float
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return f


@pytest.mark.parametrize("d", [16, 96, 128, 256])
@pytest.mark.parametrize("kind", ["float", "integer"])
def test_numpy_restatement_equals_the_host_fvec_L2sqr(d, kind):
    f = _host_fvec_l2sqr()
    rng = np.random.default_rng(d + (0 if kind == "float" else 1000))
    n = 300
    x = rng.integers(0, 256, size=(n, d)).astype(np.float32)
    if kind == "float":
        q = (rng.standard_normal((n, d)) * 60 + 100).astype(np.float32)
        x[: n // 2] = (rng.standard_normal((n // 2, d)) * 1e3).astype(np.float32)  # far from integers, wide range
    else:
        q = rng.integers(0, 256, size=(n, d)).astype(np.float32)
    got = np.array([f(q[i].ctypes.data, x[i].ctypes.data, d) for i in range(n)], np.float32)
    want = np.concatenate([rerank_ref.fvec_l2sqr(q[i], x[i:i + 1]) for i in range(n)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_restated_top_k_orders_by_distance_then_label():
    base = np.array([[3] * 16, [1] * 16, [3] * 16, [0] * 16], np.uint8)
    q = np.zeros((1, 16), np.float32)
    dist, lab = rerank_ref.rerank(base, q, np.array([[2, -1, 0, 1, 7, 2]]), 6)
    assert lab.tolist() == [[1, 0, 2, 2, -1, -1]]
    assert dist[0, :4].tolist() == [16.0, 144.0, 144.0, 144.0] and (dist[0, 4:] == rerank_ref.FLT_MAX).all()


def test_new_entry_points_are_bound_and_refuse_a_null_handle(pkg):
    for m in ("upload_base", "upload_base_dev", "upload_base_bvecs", "rerank", "rerank_dev", "search_rerank"):
        assert callable(getattr(pkg.GpuIndex, m, None)), m
    g = pkg.GpuIndex.__new__(pkg.GpuIndex)  # a handle that was never created
    g._h = ctypes.c_void_p()
    with pytest.raises(pkg.IvfHnswError) as e:
        g.upload_base(np.zeros((4, 16), np.uint8))
    assert e.value.code == pkg.ERR_INVALID
    with pytest.raises(pkg.IvfHnswError) as e:
        g.rerank(np.zeros((1, 16), np.float32), np.zeros((1, 4), np.int64), 2)
    assert e.value.code == pkg.ERR_INVALID


def test_no_device_fails_loudly(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device error path is covered on the CPU box")
    with pytest.raises(pkg.IvfHnswError) as e:
        pkg.GpuIndex(0)
    assert e.value.code == pkg.ERR_HIP
