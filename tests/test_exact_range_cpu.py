"""CPU side of the exact range search: the numpy restatement (tests/exact_range_ref.py) on a case written out by hand,
the radius -> int32 threshold rule of include/ivfhnsw_hip.h against the float comparison it stands for, the exported entry
points, and the range file of tools/ground_truth.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

import exact_range_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ground_truth  # noqa: E402

F = np.float32
INF = F(np.inf)


def test_restatement_on_three_rows():
    base = np.zeros((3, 16), np.uint8)
    base[1, 0] = 3       # 9 from the zero row
    base[2, :2] = 2      # 8 from the zero row, 1 + 4 = 5 from row 1
    q = base[[0, 1]]
    # distances: query 0 -> [0, 9, 8], query 1 -> [9, 0, 5]
    lims, dist, lab = exact_range_ref.search(base, q, 9.0)  # strict: the 9s stay out
    assert lims.dtype == np.uint64 and dist.dtype == np.float32 and lab.dtype == np.int64
    assert lims.tolist() == [0, 2, 4]
    assert lab.tolist() == [0, 2, 1, 2] and dist.tolist() == [0.0, 8.0, 0.0, 5.0]  # ascending label, not distance
    lims, dist, lab = exact_range_ref.search(base, q, 9.5)
    assert lims.tolist() == [0, 3, 6] and lab.tolist() == [0, 1, 2, 0, 1, 2]
    assert dist.tolist() == [0.0, 9.0, 8.0, 9.0, 0.0, 5.0]
    lims, dist, lab = exact_range_ref.search(base, q, 0.0)
    assert lims.tolist() == [0, 0, 0] and dist.size == 0 and lab.size == 0
    lims, dist, lab = exact_range_ref.search(base, q, 1e-30)
    assert lims.tolist() == [0, 1, 2] and lab.tolist() == [0, 1]


DISTS = (0, 1, 2, 1000, 2 ** 24 - 1, 256 * 255 ** 2)


def _radii(D):
    one, fd = F(1), F(D)
    return [-INF, F(-1), F(-0.0), F(0), np.nextafter(F(0), INF), F(0.5), one, np.nextafter(one, INF), np.nextafter(one, -INF),
            fd, np.nextafter(fd, INF), np.nextafter(fd, -INF), F(D + 0.5), F(2 ** 24), F(2 ** 25), INF]


@pytest.mark.parametrize("D", DISTS)
def test_threshold_is_the_float_comparison(D):
    for radius in _radii(D):
        thr = exact_range_ref.threshold(radius)
        assert 0 <= thr <= 2 ** 31 - 1
        for dist in DISTS:
            assert (dist < thr) == bool(F(dist) < radius), (dist, float(radius), thr)


def test_library_exports_the_exact_range_search(pkg):
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for sym in ("ivfhnsw_gpu_exact_range_search", "ivfhnsw_gpu_exact_range_search_dev", "ivfhnsw_gpu_exact_range_results",
                "ivfhnsw_gpu_exact_range_results_dev"):
        assert sym in pkg.ABI_SYMBOLS and hasattr(raw, sym), sym
    for m in ("exact_range_search", "exact_range_search_dev", "exact_range_results", "exact_range_results_dev"):
        assert callable(getattr(pkg.GpuIndex, m))


def test_range_file_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, size=(50, 16), dtype=np.uint8)
    lims, dist, lab = exact_range_ref.search(base, base[:7], 90000.0)
    assert 0 < lab.size < 7 * 50
    path = str(tmp_path / "gt_range.npz")
    ground_truth.write_range(path, lims, dist, lab, 90000.0)
    assert os.path.exists(path)  # exactly the name given, no suffix added
    bl, bd, bb, br = ground_truth.read_range(path)
    assert bl.dtype == np.uint64 and bd.dtype == np.float32 and bb.dtype == np.int64 and br == 90000.0
    assert np.array_equal(bl, lims) and np.array_equal(bb, lab) and np.array_equal(bd.view(np.uint32), dist.view(np.uint32))
    # no results at all is a valid file
    ground_truth.write_range(path, np.zeros(4, np.uint64), np.zeros(0, np.float32), np.zeros(0, np.int64), 0.0)
    bl, bd, bb, br = ground_truth.read_range(path)
    assert bl.tolist() == [0, 0, 0, 0] and bd.size == 0 and bb.size == 0 and br == 0.0
    # lims that does not describe the arrays is refused
    ground_truth.write_range(path, lims[:-1], dist, lab, 1.0)
    with pytest.raises(ValueError):
        ground_truth.read_range(path)
