"""numpy restatement of ivfhnsw_gpu_kmeans (include/ivfhnsw_hip.h), the expected values of the k-means
tests.  One iteration:
  assign   orc.knn(centroids, 1, queries=x): the MFMA form (norm + norm) - 2 dot, fmaf chains, ties to the lower id
  obj      the distances summed in double
  update   per non-empty cluster: float32 sum of the members' rows in ascending point index from 0, then / (float)cnt;
           step r adds every cluster's r-th member at once (never np.sum, which sums pairwise)
  split    faiss's split_clusters with the pick made deterministic: empty ci ascending, cj = first argmax of the current
           counts, row ci = row cj, rows scaled by 1 +- EPS by parity of the component, counts halved"""
import numpy as np

from oracle import orc

EPS = np.float32(1.0 / 1024.0)


def assign(x, c):
    ids, dist = orc.knn(c, 1, queries=x)
    return ids[:, 0], dist[:, 0]


def update(x, c, a):
    """(new centroids, counts): empty clusters keep their row."""
    x = np.asarray(x, np.float32)
    nc, d = c.shape
    cnt = np.bincount(a, minlength=nc).astype(np.int64)
    order = np.argsort(a, kind="stable")           # each cluster's members in ascending point index
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    s = np.zeros((nc, d), np.float32)
    live = np.nonzero(cnt > 0)[0]
    r = 0
    while live.size:
        s[live] = s[live] + x[order[start[live] + r]]
        r += 1
        live = live[cnt[live] > r]
    out = np.array(c, np.float32, copy=True)
    nz = cnt > 0
    out[nz] = s[nz] / cnt[nz].astype(np.float32)[:, None]
    return out, cnt


def split(c, cnt):
    """(centroids, counts, [(ci, cj), ...]) after the empty-cluster splits, applied in order."""
    c = np.array(c, np.float32, copy=True)
    cnt = np.array(cnt, np.int64, copy=True)
    d = c.shape[1]
    even = (np.arange(d) % 2) == 0
    one = np.float32(1.0)
    f_ci = np.where(even, one + EPS, one - EPS).astype(np.float32)
    f_cj = np.where(even, one - EPS, one + EPS).astype(np.float32)
    pairs = []
    for ci in range(len(cnt)):
        if cnt[ci] != 0:
            continue
        cj = int(np.argmax(cnt))                   # first maximum: ties to the lower id
        row = c[cj].copy()
        c[ci] = row * f_ci
        c[cj] = row * f_cj
        cnt[ci] = cnt[cj] // 2
        cnt[cj] -= cnt[ci]
        pairs.append((ci, cj))
    return c, cnt, pairs


def kmeans(x, seeds, niter):
    """(centroids, assign of the last iteration or None, obj [niter]) of niter iterations."""
    x = np.ascontiguousarray(x, np.float32)
    c = np.array(seeds, np.float32, copy=True)
    a = None
    obj = np.zeros(niter, np.float64)
    for t in range(niter):
        a, dist = assign(x, c)
        obj[t] = dist.astype(np.float64).sum()
        c, cnt = update(x, c, a)
        c, _, _ = split(c, cnt)
    return c, a, obj
