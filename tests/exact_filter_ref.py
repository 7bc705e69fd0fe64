"""numpy restatement of the exact calls under a base filter (ivfhnsw_gpu_set_base_filter), the expected
values of their tests.  Written on the whole store, not on the sub-store: the distances of every row, the rows that do
not pass taken out by the mask, labels the original row numbers.  tests/test_exact_filter_cpu.py pins it to the
unfiltered restatements run on base[pass] with the labels mapped back."""
import numpy as np

import exact_ref

FLT_MAX = exact_ref.FLT_MAX


def pass_mask(n, labels, deny=False):
    """bool [n]: the rows of a store of n rows that pass a set of uint32 labels.  A label is a row number; labels >= n
    match nothing, repeats count once.  Allow: a row passes iff it is in the set; deny: iff it is not."""
    lab = np.asarray(labels, dtype=np.uint32).ravel().astype(np.int64)
    in_set = np.zeros(n, bool)
    in_set[lab[lab < n]] = True
    return ~in_set if deny else in_set


def search(base_u8, queries_u8, k, mask):
    """(distances f32 [nq, k], labels i64 [nq, k]): the k nearest PASSING rows ascending by (distance, label), padded with
    FLT_MAX / -1 when fewer than k rows pass."""
    mask = np.asarray(mask, bool)
    dist = exact_ref.distances(base_u8, queries_u8)
    nq, n = dist.shape
    assert mask.shape == (n,) and dist.max(initial=0) < 1 << 24
    keys = (dist << 32) | np.arange(n, dtype=np.int64)[None, :]
    keys[:, ~mask] = np.iinfo(np.int64).max  # behind every real key
    keys.sort(axis=1)
    m = min(k, int(mask.sum()))
    out_d = np.full((nq, k), FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    out_d[:, :m] = (keys[:, :m] >> 32).astype(np.float32)
    out_l[:, :m] = keys[:, :m] & 0xffffffff
    return out_d, out_l


def range_search(base_u8, queries_u8, radius, mask):
    """(lims u64 [nq + 1], distances f32 [total], labels i64 [total]): per query the PASSING rows with
    float32(dist) < float32(radius), in ascending label."""
    mask = np.asarray(mask, bool)
    dist = exact_ref.distances(base_u8, queries_u8)
    assert mask.shape == (dist.shape[1],) and dist.max(initial=0) < 1 << 24
    df = dist.astype(np.float32)
    hit = (df < np.float32(radius)) & mask[None, :]
    lims = np.zeros(dist.shape[0] + 1, np.uint64)
    lims[1:] = np.cumsum(hit.sum(1), dtype=np.uint64)
    q, lab = np.nonzero(hit)
    return lims, df[q, lab], lab.astype(np.int64)


# ---- the pass patterns the tests share: name -> (labels, deny) for a store of n rows -------------------------------------
PATTERNS = ("all", "none", "last", "first", "alt_first_empty", "alt_last_empty", "gap", "rand50", "rand03", "rand64", "deny0", "only7")


def pattern(name, n, seed=0):
    """(labels uint32, deny) of a named pattern.  Whole words of 32 rows are what the masked sweep skips, and the sparse
    patterns are what the rule sends to the list of passing rows.  The allow sets carry labels at and beyond n and a
    repeat: neither changes the mask."""
    rows = np.arange(n)
    word = rows // 32
    last_word = (n - 1) // 32
    extra = [n, n + 37, n]  # match nothing

    def allow(mask):
        lab = np.flatnonzero(mask)
        return np.concatenate([lab, lab[:3], extra]).astype(np.uint32), False

    if name == "all":
        return np.zeros(0, np.uint32), True            # an empty deny set passes everything
    if name == "none":
        return np.zeros(0, np.uint32), False           # an empty allow set passes nothing
    if name == "last":
        return np.array([n - 1], np.uint32), False
    if name == "first":
        return np.array([0, 0], np.uint32), False
    if name == "alt_first_empty":                      # words alternately empty and full, the first one empty
        return allow(word % 2 == 1)
    if name == "alt_last_empty":                       # ... the last, partial word empty
        return allow(word % 2 != last_word % 2)
    if name == "gap":                                  # four empty words in a row inside the first split, by denial
        return np.concatenate([rows[(word >= 5) & (word < 9)], extra]).astype(np.uint32), True
    if name == "rand50":
        return allow(np.random.default_rng(seed + 50).random(n) < 0.5)
    if name == "rand03":                               # npass <= n / 8: the rule picks the list
        return allow(np.random.default_rng(seed + 3).random(n) < 0.03)
    if name == "rand64":                               # 64 rows (or all of a smaller store): k = 100 is padded behind them
        return allow(np.isin(rows, np.random.default_rng(seed + 64).choice(n, min(n, 64), replace=False)))
    if name == "deny0":                                # of the tied rows {0, 1, 7} the lowest label is denied
        return np.array([0], np.uint32), True
    if name == "only7":                                # ... only the highest is allowed
        return np.array([min(7, n - 1)], np.uint32), False
    raise KeyError(name)
