"""numpy restatement of the exact calls with a base tag per query (ivfhnsw_gpu_exact_search_tags /
ivfhnsw_gpu_exact_range_search_tags), the expected values of their tests, and the base tag assignment, the
query-to-tag assignments and the grid those tests share.  Every query is answered under ITS OWN mask -- btags == t for a
query whose tag is t, all-true for NONE -- from the restatements of tests/exact_filter_ref.py, which stays as it is.
tests/test_exact_tags_cpu.py pins this file to exact_filter_ref run per tag on the tag's queries, and asserts what the
fixture has to hold for the GPU tests to mean something."""
import itertools

import numpy as np

import exact_filter_ref as fr
import exact_ref

FLT_MAX = exact_ref.FLT_MAX
NONE = 0xffff

# ---- the base tag assignment: a uint16 per row of a store of n rows -----------------------------------------------------------
BIG, FEW, SOME, ONE, MID = 3, 255, 256, 0xfffe, 9  # >= half the rows; < 10 rows; < 100 rows; exactly one row; a quarter of the odd rows
MANY0 = 1000                                        # the first of the tags of about 4 rows each
ABSENT = (7, 0x1234)                                # tags no row carries
TIED = (0, 1, 7)                                    # rows the stores of the GPU tests make equal (exact_filter_ref's deny0 / only7)


def many_tags(n):
    """How many tags of about 4 rows each base_tags(n) holds: MANY0 .. MANY0 + many_tags(n) - 1."""
    return max(1, ((n // 2) * 2 // 5) // 4)


def base_tags(n):
    """uint16 [n].  Even rows carry BIG.  The odd rows, in order: 4 * many_tags(n) rows dealt round-robin over the MANY tags
    (a tag's rows lie 2 * many_tags(n) apart), then FEW, SOME, ONE and MID, the rest untagged.  The tied rows carry BIG."""
    t = np.full(n, NONE, np.uint16)
    t[0::2] = BIG
    odd = np.arange(1, n, 2)
    m = odd.size
    nm = many_tags(n)
    a = 4 * nm
    t[odd[:a]] = MANY0 + np.arange(min(a, m)) % nm
    for tag, cnt in ((FEW, min(5, max(1, m // 8))), (SOME, min(60, max(1, m // 5))), (ONE, 1), (MID, m // 4)):
        t[odd[a:a + cnt]] = tag
        a += cnt
    if n > max(TIED):
        t[list(TIED)] = BIG
    return t


def tags_in_use(btags):
    u = np.unique(btags)
    return u[u != NONE]


def tag_mask(btags, tag):
    """bool [n]: the rows a query whose tag is `tag` searches."""
    return np.ones(btags.size, bool) if int(tag) == NONE else btags == np.uint16(tag)


def apply_sets(n, calls, start=None):
    """The tag array after set_base_tags calls [(rows, tags), ...] on a store of n rows (start: the array before them, None =
    untagged): rows >= n match nothing, the tag NONE untags."""
    t = np.full(n, NONE, np.uint16) if start is None else np.array(start, np.uint16)
    for rows, tags in calls:
        rows, tags = np.asarray(rows, np.int64), np.asarray(tags, np.uint16)
        t[rows[rows < n]] = tags[rows < n]
    return t


# ---- the stores and queries of the tests (the ties of tests/test_gpu_exact_filter.py's _base) -------------------------------
def make_base(n, d):
    rng = np.random.default_rng(1000 * d + n)
    b = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    if n > 7:
        b[1] = b[0]
        b[7] = b[0]
        b[n - 1] = b[3]
        b[4] = 0
        b[5] = 255
    return b


def make_queries(nq, d, base):
    rng = np.random.default_rng(d * 7919 + base.shape[0] * 31 + nq * 7)
    q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
    q[0] = base[0]  # at distance 0 from every tied row
    if nq > 2:
        q[1] = 0
        q[2] = 255
    return q


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def search(base_u8, queries_u8, k, btags, qtags):
    """(distances f32 [nq, k], labels i64 [nq, k]) in the caller's query order, each query under its own mask."""
    nq = queries_u8.shape[0]
    out_d = np.full((nq, k), FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        out_d[q], out_l[q] = (a[0] for a in fr.search(base_u8, queries_u8[q:q + 1], k, tag_mask(btags, qtags[q])))
    return out_d, out_l


def range_search(base_u8, queries_u8, radius, btags, qtags):
    """(lims u64 [nq + 1], distances f32 [total], labels i64 [total]): per query, in the caller's order, the rows under the
    query's own mask with float32(dist) < float32(radius), ascending label."""
    nq = queries_u8.shape[0]
    lims = np.zeros(nq + 1, np.uint64)
    ds, ls = [np.zeros(0, np.float32)], [np.zeros(0, np.int64)]
    for q in range(nq):
        _, d, l = fr.range_search(base_u8, queries_u8[q:q + 1], radius, tag_mask(btags, qtags[q]))
        lims[q + 1] = lims[q] + np.uint64(d.size)
        ds.append(d)
        ls.append(l)
    return lims, np.concatenate(ds), np.concatenate(ls)


def search_blocked(base_u8, queries_u8, k, btags, qtags):
    """search() for hundreds of queries: the same values, one distance matrix and one sort per tag present."""
    nq = queries_u8.shape[0]
    out_d = np.full((nq, k), FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    for t in np.unique(qtags):
        idx = np.flatnonzero(qtags == t)
        out_d[idx], out_l[idx] = fr.search(base_u8, queries_u8[idx], k, tag_mask(btags, t))
    return out_d, out_l


def range_blocked(base_u8, queries_u8, radius, btags, qtags):
    """range_search() for hundreds of queries: the same values from one call per tag present."""
    nq = queries_u8.shape[0]
    per_q = [None] * nq
    for t in np.unique(qtags):
        idx = np.flatnonzero(qtags == t)
        lims, d, l = fr.range_search(base_u8, queries_u8[idx], radius, tag_mask(btags, t))
        for j, q in enumerate(idx):
            per_q[q] = (d[int(lims[j]):int(lims[j + 1])], l[int(lims[j]):int(lims[j + 1])])
    lims = np.zeros(nq + 1, np.uint64)
    lims[1:] = np.cumsum([p[0].size for p in per_q], dtype=np.uint64)
    return lims, np.concatenate([p[0] for p in per_q]), np.concatenate([p[1] for p in per_q])


# ---- query-to-tag assignments: name -> uint16 [nq] -------------------------------------------------------------------------------
ASSIGNMENTS = ("none", "one", "each", "sizes", "g129", "interleaved", "absent", "many")
MIN_NQ = {"none": 1, "one": 1, "each": 1, "sizes": 96, "g129": 129, "interleaved": 1, "absent": 1, "many": 300}
MANY_N = 6001  # "many" is for the store that holds 300 tags of about 4 rows


def fits(name, n, nq):
    return nq >= MIN_NQ[name] and (name != "many" or n == MANY_N)


def assignment(name, n, nq, seed=0):
    rng = np.random.default_rng(seed + 17 * nq)
    used = tags_in_use(base_tags(n))
    named = [BIG, FEW, SOME, ONE, MID, NONE]
    every = np.array(named + [t for t in used if t not in named], np.uint16)
    if name == "none":                       # every query untagged: the whole store
        return np.full(nq, NONE, np.uint16)
    if name == "one":                        # every query the same tag (the big one; query 0 meets the tied rows)
        return np.full(nq, BIG, np.uint16)
    if name == "each":                       # the tags in turn: one query per tag while they last, every strip padded 31 of 32
        return every[np.arange(nq) % every.size]
    if name == "sizes":                      # groups of 31 / 32 / 33 side by side, the rest untagged
        out = np.full(nq, NONE, np.uint16)
        out[:31], out[31:63], out[63:96] = BIG, SOME, MID
        return out
    if name == "g129":                       # a group of 129: more than a workgroup's rows at both strip widths (128, 64)
        out = every[np.arange(nq) % every.size]
        out[:129] = SOME
        return rng.permutation(out)
    if name == "interleaved":                # the tags in use and NONE in random order
        return rng.choice(every, nq).astype(np.uint16)
    if name == "absent":                     # half the queries on tags no row carries
        out = rng.choice(every, nq).astype(np.uint16)
        out[::2] = np.array(ABSENT, np.uint16)[(np.arange(nq)[::2] // 2) % 2]
        return out
    if name == "many":                       # every query its own tag of about 4 rows
        assert n == MANY_N and nq <= many_tags(n)
        return (MANY0 + np.arange(nq)).astype(np.uint16)
    raise KeyError(name)


def strips(qtags, btags):
    """The strips of 32 a chunk with these query tags takes: ceil(count / 32) per tag that has rows, and for NONE."""
    t, c = np.unique(qtags, return_counts=True)
    has = np.array([int(x) == NONE or bool((btags == x).any()) for x in t])
    return int(((c[has] + 31) // 32).sum())


# ---- the grid of tests/test_gpu_exact_tags.py ----------------------------------------------------------------------------------
NS, DS, KS, NQS = (33, 6001), (16, 48, 128, 256), (1, 10, 100), (1, 33, 129, 300)
SPLITS, MAPS = (1, 3, 64), (0, 1)


def grid():
    """(n, d, k, nq, assignment, exact_splits, exact_range_map): every (n, d, k) once with the other axes cycling, then every
    assignment at every nq it fits on the 6001-row store, k cycling; plus the corners named below."""
    cases = []
    for i, (n, d, k) in enumerate(itertools.product(NS, DS, KS)):
        names = [a for a in ASSIGNMENTS if a != "many"]
        a = names[i % len(names)]
        nqs = [q for q in NQS if fits(a, n, q)]
        cases.append((n, d, k, nqs[i % len(nqs)], a, SPLITS[i % 3], MAPS[i % 2]))
    i = 0
    for a in ASSIGNMENTS:
        for nq in NQS:
            if fits(a, MANY_N, nq):
                cases.append((MANY_N, DS[i % 4], KS[i % 3], nq, a, SPLITS[(i // 3) % 3], MAPS[(i // 2) % 2]))
                i += 1
    cases += [(MANY_N, 48, 10, 300, "many", 64, 1),   # a 4-row tag under 64 splits: most splits empty
              (MANY_N, 16, 1, 300, "many", 1, 0), (MANY_N, 128, 100, 300, "g129", 64, 1), (MANY_N, 16, 100, 129, "g129", 1, 0),
              (33, 16, 10, 33, "each", 3, 1)]
    return sorted(set(cases))
