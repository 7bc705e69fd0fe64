"""range_ref, the helper the range-search tests take their expected values from, checked on the CPU against the oracle's
own statistics (no GPU)."""
import numpy as np

from conftest import corpus
import range_ref
from test_gpu_remove import BASE

NPROBE, MAX_CODES, EF = 16, 2000, 40
GROUPING = dict(seed=43, nc=256, d=96, M=16, n_base=20000, nq=64, nsubc=8)  # tests/test_gpu_filter.py's shape


def test_every_scored_code_is_admitted_ivf():
    c = corpus(**BASE)
    sc = range_ref.scored_batch(c, c["queries"], NPROBE, MAX_CODES, EF, key=("base", NPROBE, MAX_CODES, EF))
    assert len(sc["ncode"]) == 128
    for i in range(128):
        assert len(sc["labels"][i]) == sc["ncode"][i]
        assert len(np.unique(sc["labels"][i])) == sc["ncode"][i]
        assert len(range_ref.ivf_order(c, sc["cid"][i], MAX_CODES)) == sc["ncode"][i]
    assert sc["ncode"].min() >= MAX_CODES // 4 and sc["ncode"].max() < 2 * MAX_CODES + 2000


def test_every_scored_code_is_admitted_grouping():
    c = corpus(**GROUPING)
    sc = range_ref.scored_batch(c, c["queries"], NPROBE, MAX_CODES, 64, pruning=True, key=("grouping", True))
    for i in range(len(c["queries"])):
        assert len(sc["labels"][i]) == sc["ncode"][i] == len(np.unique(sc["labels"][i]))
    assert sc["ncode"].max() <= 1024  # what order check (a) of the GPU test rests on


def test_expected_results_grow_with_the_radius():
    c = corpus(**BASE)
    sc = range_ref.scored_batch(c, c["queries"], NPROBE, MAX_CODES, EF, key=("base", NPROBE, MAX_CODES, EF))
    radii = [range_ref.pooled_quantile(sc, q) for q in (0.0005, 0.01, 0.1)] + [np.float32(np.inf)]
    prev = None
    for r in radii:
        lims, dist, lab = range_ref.expected_ivf(c, sc, MAX_CODES, r)
        per = np.diff(lims.astype(np.int64))
        assert lims[0] == 0 and lims[-1] == len(dist) == len(lab)
        assert (dist < r).all()
        for i in (0, 17, 127):
            assert np.array_equal(range_ref.result_set(lims, dist, lab, i), range_ref.expected_set(sc, i, r))
        if prev is not None:
            assert (per >= prev).all()
        prev = per
    assert np.array_equal(prev, sc["ncode"])  # +inf: every scored code
    low = np.diff(range_ref.expected_ivf(c, sc, MAX_CODES, radii[0])[0].astype(np.int64))
    assert (low == 0).any() and (low > 0).any()


def test_filtered_rebuilds_lims():
    lims = np.array([0, 2, 2, 5], np.uint64)
    dist = np.arange(5, dtype=np.float32)
    lab = np.array([7, 8, 9, 7, 10], np.int64)
    got = range_ref.filtered((lims, dist, lab), np.array([7, 10]))
    assert got[0].tolist() == [0, 1, 1, 3] and got[2].tolist() == [7, 7, 10] and got[1].tolist() == [0.0, 3.0, 4.0]
