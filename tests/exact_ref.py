"""numpy restatement of the exact brute-force search (ivfhnsw_gpu_exact_search), the expected values of its tests:
squared L2 between uint8 rows in int64 arithmetic and a lexicographic (distance, label) top-k."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def distances(base_u8, queries_u8):
    """[nq, n] int64: sum over j of (q[j] - x[j])^2."""
    b = np.asarray(base_u8).astype(np.int32)
    q = np.asarray(queries_u8).astype(np.int32)
    out = np.empty((q.shape[0], b.shape[0]), np.int64)
    for i in range(q.shape[0]):
        diff = b - q[i]
        out[i] = np.einsum("ij,ij->i", diff, diff, dtype=np.int64)
    return out


def search(base_u8, queries_u8, k):
    """(distances f32 [nq, k], labels i64 [nq, k]): the k nearest rows ascending by (distance, label), padded with
    FLT_MAX / -1 when the base has fewer than k rows."""
    dist = distances(base_u8, queries_u8)
    nq, n = dist.shape
    assert dist.max(initial=0) < 1 << 24  # exactly representable as float32
    keys = (dist << 32) | np.arange(n, dtype=np.int64)[None, :]
    m = min(k, n)
    top = np.sort(np.partition(keys, m - 1, axis=1)[:, :m], axis=1)
    out_d = np.full((nq, k), FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    out_d[:, :m] = (top >> 32).astype(np.float32)
    out_l[:, :m] = top & 0xffffffff
    return out_d, out_l
