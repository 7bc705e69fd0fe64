"""numpy restatement of the exact range search (ivfhnsw_gpu_exact_range_search), the expected values of its tests: on
top of exact_ref.distances, per query the rows with float32(dist) < float32(radius) in ascending label."""
import numpy as np

import exact_ref


def threshold(radius):
    """The int32 threshold the library turns a radius into (include/ivfhnsw_hip.h): dist < threshold(radius) is
    float32(dist) < radius for every integer 0 <= dist < 2^24."""
    r = np.float32(radius)
    if not r > 0:
        return 0
    if r > np.float32(16777216.0):
        return 2 ** 31 - 1
    return int(np.ceil(r))


def from_distances(dist, radius):
    """(lims u64 [nq + 1], distances f32 [total], labels i64 [total]) of an int64 distance matrix [nq, n]."""
    assert dist.max(initial=0) < 1 << 24  # exactly representable as float32
    df = dist.astype(np.float32)
    hit = df < np.float32(radius)
    lims = np.zeros(dist.shape[0] + 1, np.uint64)
    lims[1:] = np.cumsum(hit.sum(1), dtype=np.uint64)
    q, lab = np.nonzero(hit)  # row major: by query, then ascending label
    return lims, df[q, lab], lab.astype(np.int64)


def search(base_u8, queries_u8, radius):
    return from_distances(exact_ref.distances(base_u8, queries_u8), radius)
