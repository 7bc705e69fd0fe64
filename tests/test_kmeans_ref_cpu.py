"""CPU checks of the k-means restatement (tests/kmeans_ref.py) that the device tests compare against: the split rule on
hand-made counts, and the vectorised member-order sum against a literal per-cluster loop."""
import numpy as np

import kmeans_ref as kr

UP = np.float32(1.0) + np.float32(1.0 / 1024.0)
DN = np.float32(1.0) - np.float32(1.0 / 1024.0)


def _scaled(row, even_factor, odd_factor):
    out = row.copy()
    out[0::2] = row[0::2] * even_factor
    out[1::2] = row[1::2] * odd_factor
    return out


def test_split_ties_repeated_donor_and_odd_counts():
    rng = np.random.default_rng(3)
    c = rng.normal(0, 10, (6, 8)).astype(np.float32)
    cnt = np.array([0, 5, 5, 0, 0, 2])
    out, cnt2, pairs = kr.split(c, cnt)
    # ci 0: 1 and 2 tie at 5 -> the lower id; 5 -> 2 + 3.  ci 3: cluster 2 alone at 5.  ci 4: 1 and 2 tie at 3 -> 1 again
    assert pairs == [(0, 1), (3, 2), (4, 1)]
    assert cnt2.tolist() == [2, 2, 3, 2, 1, 2]
    assert cnt2.sum() == cnt.sum()
    r1 = _scaled(c[1], DN, UP)                       # cluster 1 after giving to 0
    assert np.array_equal(out[0], _scaled(c[1], UP, DN))
    assert np.array_equal(out[3], _scaled(c[2], UP, DN))
    assert np.array_equal(out[2], _scaled(c[2], DN, UP))
    assert np.array_equal(out[4], _scaled(r1, UP, DN))  # reads the row the first split changed
    assert np.array_equal(out[1], _scaled(r1, DN, UP))
    assert np.array_equal(out[5], c[5])


def test_split_without_empty_clusters_changes_nothing():
    c = np.arange(12, dtype=np.float32).reshape(3, 4)
    out, cnt2, pairs = kr.split(c, np.array([1, 1, 3]))
    assert pairs == [] and np.array_equal(out, c) and cnt2.tolist() == [1, 1, 3]


def test_split_of_a_count_of_two_and_a_chain():
    c = np.ones((4, 4), np.float32)
    out, cnt2, pairs = kr.split(c, np.array([0, 0, 0, 4]))
    # 4 -> 2 + 2 (ci 0); then 0 and 3 tie at 2 -> 0 gives (1 + 1); then 3 (2) gives to 2
    assert pairs == [(0, 3), (1, 0), (2, 3)]
    assert cnt2.tolist() == [1, 1, 1, 1]


def test_update_sums_members_in_point_order():
    rng = np.random.default_rng(5)
    n, nc, d = 500, 7, 12
    x = (rng.normal(0, 1, (n, d)) * np.float32(1e4) + rng.normal(0, 1, (n, d))).astype(np.float32)
    a = rng.integers(0, nc - 1, n)                   # the last cluster stays empty
    c = rng.normal(0, 1, (nc, d)).astype(np.float32)
    out, cnt = kr.update(x, c, a)
    for k in range(nc):
        m = np.nonzero(a == k)[0]
        assert cnt[k] == len(m)
        if not len(m):
            assert np.array_equal(out[k], c[k])
            continue
        s = np.zeros(d, np.float32)
        for i in m:                                  # ascending point index, float32 adds
            s = (s + x[i]).astype(np.float32)
        assert np.array_equal(out[k], s / np.float32(len(m)))
