"""CPU side of the exact brute-force search: the integer restatement (tests/exact_ref.py) gives fvec_L2sqr's bits, the
.ivecs functions of tools/ground_truth.py round-trip, and the library exports the two entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest

import exact_ref
import rerank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ground_truth  # noqa: E402


@pytest.mark.parametrize("d", (16, 96, 128, 256))
def test_integer_distance_is_fvec_l2sqr_bit_for_bit(d):
    """For d <= 256 every partial sum of fvec_L2sqr is an integer below 2^24: the integer distance, converted, is the
    float the re-rank returns with every row as a candidate -- labels and distance bits."""
    rng = np.random.default_rng(d)
    n, nq, k = 300, 9, 40
    base = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    base[1] = base[7] = base[0]
    base[n - 1] = base[3]
    base[10] = 0
    base[11] = 255
    q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
    q[0] = base[0]
    q[1] = 0
    q[2] = 255
    cand = np.tile(np.arange(n, dtype=np.int64), (nq, 1))
    want_d, want_l = rerank_ref.rerank(base, q.astype(np.float32), cand, k)
    got_d, got_l = exact_ref.search(base, q, k)
    assert np.array_equal(got_l, want_l)
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    if d == 256:
        # the largest value there is: all 255 against all 0
        assert exact_ref.distances(base[10:11], q[2:3])[0, 0] == 16646400 == 256 * 255 * 255
        far_d, far_l = exact_ref.search(base[10:11], q[2:3], 1)
        ref_d, _ = rerank_ref.rerank(base[10:11], q[2:3].astype(np.float32), np.zeros((1, 1), np.int64), 1)
        assert far_l[0, 0] == 0 and far_d.view(np.uint32)[0, 0] == ref_d.view(np.uint32)[0, 0]
        assert far_d[0, 0] == np.float32(16646400)


def test_restatement_pads_beyond_the_base():
    base = np.arange(3 * 16, dtype=np.uint8).reshape(3, 16)
    d, l = exact_ref.search(base, base[1:2], 5)
    assert l[0].tolist() == [1, 0, 2, -1, -1]
    assert d[0, :3].tolist() == [0.0, 16 * 256.0, 16 * 256.0] and (d[0, 3:] == exact_ref.FLT_MAX).all()


def test_ivecs_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 1 << 32, size=(17, 100), dtype=np.int64)
    lab[0, 0] = 0
    lab[1, 1] = (1 << 31) - 1
    lab[2, 2] = 1 << 31           # beyond int32: the reference's idx_t is uint32
    lab[3, 3] = (1 << 32) - 2
    path = str(tmp_path / "gt.ivecs")
    ground_truth.write_ivecs(path, lab)
    raw = np.fromfile(path, "<i4").reshape(17, 101)
    assert (raw[:, 0] == 100).all() and os.path.getsize(path) == 17 * 101 * 4  # what readXvec<idx_t> reads
    assert raw[2, 3] == -(1 << 31)
    back = ground_truth.read_ivecs(path)
    assert back.dtype == np.int64 and np.array_equal(back, lab)
    # k = 1, the drivers' ngt
    ground_truth.write_ivecs(path, lab[:, :1])
    assert np.array_equal(ground_truth.read_ivecs(path), lab[:, :1])
    # an empty slot (k beyond the base's rows) is 0xffffffff
    ground_truth.write_ivecs(path, np.array([[5, -1]]))
    assert ground_truth.read_ivecs(path).tolist() == [[5, 0xffffffff]]
    with pytest.raises(AssertionError):
        ground_truth.write_ivecs(path, np.array([[1 << 32]]))
    bad = tmp_path / "bad.ivecs"
    np.array([2, 7, 8, 3, 1, 2], "<i4").tofile(bad)
    with pytest.raises(ValueError):
        ground_truth.read_ivecs(str(bad))


def test_bvecs_image_checks_headers(tmp_path):
    d = 16
    img = np.zeros((5, d + 4), np.uint8)
    img[:, :4] = np.frombuffer(np.int32(d).tobytes(), np.uint8)
    img[:, 4:] = np.arange(5 * d, dtype=np.uint8).reshape(5, d)
    p = tmp_path / "q.bvecs"
    img.tofile(p)
    got, gd = ground_truth.read_bvecs_image(str(p))
    assert gd == d and np.array_equal(got[:, 4:], img[:, 4:]) and got.strides[0] == d + 4
    img[3, 0] = 32
    img.tofile(p)
    with pytest.raises(ValueError):
        ground_truth.read_bvecs_image(str(p))


def test_library_exports_the_exact_search(pkg):
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for sym in ("ivfhnsw_gpu_exact_search", "ivfhnsw_gpu_exact_search_dev"):
        assert sym in pkg.ABI_SYMBOLS and hasattr(raw, sym), sym
    for m in ("exact_search", "exact_search_dev"):
        assert callable(getattr(pkg.GpuIndex, m))
