"""numpy restatement of the exact calls with an interval of base values per query (ivfhnsw_gpu_exact_search_values /
ivfhnsw_gpu_exact_range_search_values), the expected values of their tests, and the base value assignment,
the query-to-interval assignments and the grid those tests share.  Every query is answered under ITS OWN mask -- lo <=
value <= hi, unsigned, inclusive, a row without a value holding 0xffffffff -- from the restatements of
tests/exact_filter_ref.py, which stays as it is.  tests/test_exact_values_cpu.py pins this file to exact_filter_ref run per
distinct interval, and asserts what the fixture has to hold for the GPU tests to mean something."""
import itertools

import numpy as np

import exact_filter_ref as fr
import exact_ref
import exact_tags_ref as tr

FLT_MAX = exact_ref.FLT_MAX
NONE = 0xffffffff
FULL = (0, NONE)
VALUED = (0, 0xfffffffe)   # every row that holds a value: a near-full window
ABSENT = (5, 60)           # no row holds a value in it
INVERTED = (0x80000010, 3)
# DESIGN.md 3.24's eleven boundary values
EDGES = (0, 1, 76, 77, 78, 0xffff, 0x10000, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff)
RUN0, RUN_ROWS = 1000, 600  # long runs of equal values: value RUN0 + row // RUN_ROWS on three rows in ten
BAND31 = 0x7fffff00         # a band of 512 values across 2^31
TIE_TOP = 0x30000           # the tie block's values descend from TIE_TOP + its rows - 1 to TIE_TOP


def tie_block(n):
    """(first row, rows) of the block of byte-identical rows whose values strictly descend with the row number: 320 rows,
    more than any compiled candidate buffer (136), where the store has them."""
    return (2000, 320) if n >= 2320 else (8, 8)


def base_values(n):
    """uint32 [n].  By row number modulo ten: 0 holds 0, 1 holds 0xfffffffe, 2 nothing; 3 and 4 a band across 2^31; 5, 6
    and 7 long runs of equal values (RUN0 + row // RUN_ROWS); 8 the values 76 .. 78; 9 scattered values from 0x10000 up.
    Over them the tie block, whose values descend."""
    r = np.arange(n, dtype=np.uint64)
    v = np.empty(n, np.uint32)
    m = r % 10
    v[m == 0] = 0
    v[m == 1] = 0xfffffffe
    v[m == 2] = NONE
    band = (m == 3) | (m == 4)
    v[band] = (BAND31 + (r[band] * 73) % 512).astype(np.uint32)
    run = (m >= 5) & (m <= 7)
    v[run] = (RUN0 + r[run] // RUN_ROWS).astype(np.uint32)
    v[m == 8] = (76 + r[m == 8] % 3).astype(np.uint32)
    v[m == 9] = (0x10000 + (r[m == 9] * 2654435761) % 0x10000).astype(np.uint32)
    t0, tn = tie_block(n)
    v[t0:t0 + tn] = TIE_TOP + tn - 1 - np.arange(tn, dtype=np.uint32)
    return v


def value_mask(bvals, lo, hi):
    """bool [n]: the rows a query whose interval is (lo, hi) searches."""
    return (bvals >= np.uint32(lo)) & (bvals <= np.uint32(hi))


def value_order(bvals):
    """All row numbers ordered by (value, row): what the holder keeps."""
    return np.argsort(bvals, kind="stable")


def windows(bvals, qr):
    """int64 [nq, 2]: the window [a, b) of every query's interval in value_order(bvals); (0, 0) for lo > hi."""
    s = bvals[value_order(bvals)]
    qr = np.asarray(qr, np.uint32).reshape(-1, 2)
    a = np.searchsorted(s, qr[:, 0], "left")
    b = np.searchsorted(s, qr[:, 1], "right")
    inv = qr[:, 0] > qr[:, 1]
    a[inv] = b[inv] = 0
    return np.stack([a, b], 1).astype(np.int64)


def apply_sets(n, calls, start=None):
    """The value array after set_base_values calls [(rows, values), ...] on a store of n rows (start: the array before them,
    None = no row holds a value): rows >= n match nothing, the value NONE un-values."""
    v = np.full(n, NONE, np.uint32) if start is None else np.array(start, np.uint32)
    for rows, vals in calls:
        rows, vals = np.asarray(rows, np.int64), np.asarray(vals, np.uint32)
        v[rows[rows < n]] = vals[rows < n]
    return v


# ---- the stores and queries of the tests ---------------------------------------------------------------------------------------
def make_base(n, d):
    """exact_tags_ref's store with the tie block: its rows are byte for byte the block's first."""
    b = tr.make_base(n, d)
    t0, tn = tie_block(n)
    b[t0:t0 + tn] = b[t0]
    return b


TIE_QUERY = 3  # the query that equals the tie block's rows, where there are that many queries


def make_queries(nq, d, base):
    q = tr.make_queries(nq, d, base)
    if nq > TIE_QUERY:
        q[TIE_QUERY] = base[tie_block(base.shape[0])[0]]
    return q


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def _distinct(qr):
    qr = np.asarray(qr, np.uint32).reshape(-1, 2)
    key = qr[:, 0].astype(np.uint64) << np.uint64(32) | qr[:, 1].astype(np.uint64)
    return [(int(k) >> 32, int(k) & 0xffffffff, np.flatnonzero(key == k)) for k in np.unique(key)]


def search(base_u8, queries_u8, k, bvals, qr):
    """(distances f32 [nq, k], labels i64 [nq, k]) in the caller's query order, each query under its own mask."""
    qr = np.asarray(qr, np.uint32).reshape(-1, 2)
    nq = queries_u8.shape[0]
    out_d = np.full((nq, k), FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        out_d[q], out_l[q] = (a[0] for a in fr.search(base_u8, queries_u8[q:q + 1], k, value_mask(bvals, *qr[q])))
    return out_d, out_l


def range_search(base_u8, queries_u8, radius, bvals, qr):
    """(lims u64 [nq + 1], distances f32 [total], labels i64 [total]): per query, in the caller's order, the rows under the
    query's own mask with float32(dist) < float32(radius), ascending label."""
    qr = np.asarray(qr, np.uint32).reshape(-1, 2)
    nq = queries_u8.shape[0]
    lims = np.zeros(nq + 1, np.uint64)
    ds, ls = [np.zeros(0, np.float32)], [np.zeros(0, np.int64)]
    for q in range(nq):
        _, d, l = fr.range_search(base_u8, queries_u8[q:q + 1], radius, value_mask(bvals, *qr[q]))
        lims[q + 1] = lims[q] + np.uint64(d.size)
        ds.append(d)
        ls.append(l)
    return lims, np.concatenate(ds), np.concatenate(ls)


def search_blocked(base_u8, queries_u8, k, bvals, qr):
    """search() for hundreds of queries: the same values, one call of exact_filter_ref per distinct interval."""
    nq = queries_u8.shape[0]
    out_d = np.full((nq, k), FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    for lo, hi, idx in _distinct(qr):
        out_d[idx], out_l[idx] = fr.search(base_u8, queries_u8[idx], k, value_mask(bvals, lo, hi))
    return out_d, out_l


def range_blocked(base_u8, queries_u8, radius, bvals, qr):
    """range_search() for hundreds of queries: the same values from one call per distinct interval."""
    nq = queries_u8.shape[0]
    per_q = [None] * nq
    for lo, hi, idx in _distinct(qr):
        lims, d, l = fr.range_search(base_u8, queries_u8[idx], radius, value_mask(bvals, lo, hi))
        for j, q in enumerate(idx):
            per_q[q] = (d[int(lims[j]):int(lims[j + 1])], l[int(lims[j]):int(lims[j + 1])])
    lims = np.zeros(nq + 1, np.uint64)
    lims[1:] = np.cumsum([p[0].size for p in per_q], dtype=np.uint64)
    return lims, np.concatenate([p[0] for p in per_q]), np.concatenate([p[1] for p in per_q])


# ---- query-to-interval assignments: name -> uint32 [nq, 2] ---------------------------------------------------------------------
ASSIGNMENTS = ("full", "one", "sizes", "g129", "each", "wide", "gap", "single", "absent", "interleaved")
MIN_NQ = {"full": 1, "one": 1, "sizes": 96, "g129": 129, "each": 1, "wide": 32, "gap": 2, "single": 1, "absent": 1, "interleaved": 1}


def fits(name, n, nq):
    return nq >= MIN_NQ[name]


def pool(n):
    """Intervals of every kind over base_values(n): runs and spans of runs (edges between runs), the bands, points, the
    boundary pairs, the tie block and parts of it, FULL, VALUED, ABSENT and INVERTED."""
    t0, tn = tie_block(n)
    nruns = (n - 1) // RUN_ROWS + 1
    p = [FULL, VALUED, (0, 0), (RUN0, RUN0), (RUN0, RUN0 + nruns), (RUN0 + 1, RUN0 + 3), (76, 78), (77, 77), (78, 0xffff),
         (BAND31, BAND31 + 511), (0x7fffffff, 0x80000000), (0x80000000, 0x800000ff), (BAND31 + 17, 0x7fffffff),
         (0xfffffffe, 0xfffffffe), (0xfffffffe, NONE), (NONE, NONE), (0x10000, 0x10fff), (1, 0xffff), (1, 0xfffffffd),
         (TIE_TOP, TIE_TOP + tn - 1), (TIE_TOP + 3, TIE_TOP + tn // 2), (TIE_TOP + tn - 1, TIE_TOP + tn - 1),
         ABSENT, INVERTED, (77, 0x80000000), (0x10000, 0xfffffffe)]
    return np.array(p, np.uint32)


def assignment(name, n, nq, seed=0):
    rng = np.random.default_rng(seed + 31 * nq)
    P = pool(n)
    t0, tn = tie_block(n)
    out = np.empty((nq, 2), np.uint32)
    if name == "full":                        # every query the whole store
        out[:] = FULL
    elif name == "one":                       # every query the same interval, which holds the tie block (query 3 equals it)
        out[:] = (1, 0xfffffffd)
    elif name == "sizes":                     # groups of 31 / 32 / 33 identical intervals side by side, the rest FULL
        out[:] = FULL
        out[:31], out[31:63], out[63:96] = (RUN0 + 1, RUN0 + 3), (BAND31, BAND31 + 511), (TIE_TOP, TIE_TOP + tn - 1)
    elif name == "g129":                      # a group of 129 identical intervals among the others, in random order
        out[:] = P[np.arange(nq) % len(P)]
        out[:129] = (0x7fffffff, 0x80000000)
        out = rng.permutation(out)
    elif name == "each":                      # one interval per query, all distinct: [u[i], u[i + 1 + i % 7]] over the values in use
        u = np.unique(base_values(n))
        i = (np.arange(nq) * 37) % (u.size - 8)
        out[:, 0], out[:, 1] = u[i], u[i + 1 + np.arange(nq) % 7]
    elif name == "wide":                      # per 32 queries one near-full window among 31 narrow ones
        u = np.unique(base_values(n))
        out[:, 0] = out[:, 1] = u[(np.arange(nq) * 11) % u.size]
        out[5::32] = VALUED
    elif name == "gap":                       # windows at the two ends of the value order, in one strip: the gap between them
        out[0::2] = (0, 0)
        out[1::2] = (0xfffffffe, 0xfffffffe)
        if nq > 4:
            out[4] = (NONE, NONE)
    elif name == "single":                    # single-row windows: the tie block's values are one row each
        out[:, 0] = out[:, 1] = TIE_TOP + (np.arange(nq) * 7) % tn
    elif name == "absent":                    # half the queries on absent and inverted intervals
        out[:] = P[rng.integers(0, len(P), nq)]
        out[::2] = np.array([ABSENT, INVERTED], np.uint32)[(np.arange(nq)[::2] // 2) % 2]
    elif name == "interleaved":               # full, empty and windowed queries in random order
        out[:] = P[rng.integers(0, len(P), nq)]
    else:
        raise KeyError(name)
    if nq > TIE_QUERY and name in ("each", "wide", "single", "interleaved"):
        out[TIE_QUERY] = (TIE_TOP, TIE_TOP + tn - 1)  # the query that equals the tie block searches exactly the block
    return out


def strips(bvals, qr):
    """(dense strips, windowed strips as lists of query numbers): the plan of a chunk restated -- whole-store windows in
    Dense strips of 32, the other non-empty ones stably by their start in strips of 32."""
    w = windows(bvals, qr)
    n = bvals.size
    full = (w[:, 0] == 0) & (w[:, 1] == n)
    win = np.flatnonzero(~full & (w[:, 1] > w[:, 0]))
    order = win[np.argsort(w[win, 0], kind="stable")]
    return (int(full.sum()) + 31) // 32, [order[i:i + 32] for i in range(0, order.size, 32)]


# ---- the grid of tests/test_gpu_exact_values.py --------------------------------------------------------------------------------
NS, DS, KS, NQS = tr.NS, tr.DS, tr.KS, tr.NQS
SPLITS, MAPS = tr.SPLITS, tr.MAPS
BIG_N = 6001


def grid():
    """(n, d, k, nq, assignment, exact_splits, exact_range_map): every (n, d, k) once with the other axes cycling, then every
    assignment at every nq it fits on the 6001-row store, k cycling; plus the corners named below."""
    cases = []
    for i, (n, d, k) in enumerate(itertools.product(NS, DS, KS)):
        a = ASSIGNMENTS[i % len(ASSIGNMENTS)]
        nqs = [q for q in NQS if fits(a, n, q)]
        cases.append((n, d, k, nqs[i % len(nqs)], a, SPLITS[i % 3], MAPS[i % 2]))
    i = 0
    for a in ASSIGNMENTS:
        for nq in NQS:
            if fits(a, BIG_N, nq):
                cases.append((BIG_N, DS[i % 4], KS[i % 3], nq, a, SPLITS[(i // 3) % 3], MAPS[(i // 2) % 2]))
                i += 1
    cases += [(BIG_N, 48, 10, 300, "single", 64, 1),   # one-row windows under 64 splits: most splits empty
              (BIG_N, 16, 100, 300, "one", 3, 0),      # k = 100 over the tie block on a split cut
              (BIG_N, 128, 100, 300, "g129", 64, 1), (BIG_N, 16, 1, 33, "gap", 1, 0), (BIG_N, 256, 100, 129, "wide", 3, 1),
              (33, 16, 10, 33, "each", 3, 1)]
    return sorted(set(cases))
