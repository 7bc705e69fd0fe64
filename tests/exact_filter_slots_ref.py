"""numpy restatement of the exact calls with a base filter slot per query (ivfhnsw_gpu_exact_search_slots /
ivfhnsw_gpu_exact_range_search_slots), the expected values of their tests, and the slot sets, the
query-to-slot assignments and the grid those tests share.  Every query is answered under ITS OWN mask -- the mask of the
slot its byte names, all-false for a slot that is not set, all-true for NONE -- from the restatements of
tests/exact_filter_ref.py, which stays as it is.  tests/test_exact_filter_slots_cpu.py pins this file to exact_filter_ref
run per slot on the slot's queries."""
import itertools

import numpy as np

import exact_filter_ref as fr
import exact_ref

FLT_MAX = exact_ref.FLT_MAX
NONE = 0xff
SLOTS = 32


def slot_masks(n, sets):
    """{slot: bool [n]} of sets = {slot: (labels, deny)}."""
    return {s: fr.pass_mask(n, lab, deny) for s, (lab, deny) in sets.items()}


def query_mask(n, masks, byte):
    """bool [n]: the rows that pass for a query whose slot byte is `byte`."""
    if byte == NONE:
        return np.ones(n, bool)
    return masks.get(int(byte), np.zeros(n, bool))


def search(base_u8, queries_u8, k, masks, qslots):
    """(distances f32 [nq, k], labels i64 [nq, k]) in the caller's query order, each query under its own mask."""
    n, nq = base_u8.shape[0], queries_u8.shape[0]
    out_d = np.full((nq, k), FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        out_d[q], out_l[q] = (a[0] for a in fr.search(base_u8, queries_u8[q:q + 1], k, query_mask(n, masks, qslots[q])))
    return out_d, out_l


def range_search(base_u8, queries_u8, radius, masks, qslots):
    """(lims u64 [nq + 1], distances f32 [total], labels i64 [total]): per query, in the caller's order, the rows passing the
    query's own mask with float32(dist) < float32(radius), ascending label."""
    n, nq = base_u8.shape[0], queries_u8.shape[0]
    lims = np.zeros(nq + 1, np.uint64)
    ds, ls = [], []
    for q in range(nq):
        _, d, l = fr.range_search(base_u8, queries_u8[q:q + 1], radius, query_mask(n, masks, qslots[q]))
        lims[q + 1] = lims[q] + np.uint64(d.size)
        ds.append(d)
        ls.append(l)
    return lims, np.concatenate(ds) if ds else np.zeros(0, np.float32), np.concatenate(ls) if ls else np.zeros(0, np.int64)


def search_blocked(base_u8, queries_u8, k, masks, qslots):
    """search() for thousands of queries: the same values, one distance matrix and one sort per slot byte present."""
    n, nq = base_u8.shape[0], queries_u8.shape[0]
    out_d = np.full((nq, k), FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    for b in np.unique(qslots):
        idx = np.flatnonzero(qslots == b)
        out_d[idx], out_l[idx] = fr.search(base_u8, queries_u8[idx], k, query_mask(n, masks, b))
    return out_d, out_l


def range_blocked(base_u8, queries_u8, radius, masks, qslots):
    """range_search() for thousands of queries: the same values from one call per slot byte present."""
    n, nq = base_u8.shape[0], queries_u8.shape[0]
    per_q = [None] * nq
    for b in np.unique(qslots):
        idx = np.flatnonzero(qslots == b)
        lims, d, l = fr.range_search(base_u8, queries_u8[idx], radius, query_mask(n, masks, b))
        for j, q in enumerate(idx):
            per_q[q] = (d[int(lims[j]):int(lims[j + 1])], l[int(lims[j]):int(lims[j + 1])])
    lims = np.zeros(nq + 1, np.uint64)
    lims[1:] = np.cumsum([p[0].size for p in per_q], dtype=np.uint64)
    return lims, np.concatenate([p[0] for p in per_q]), np.concatenate([p[1] for p in per_q])


# ---- the slot sets the tests share: one pattern of exact_filter_ref per slot ------------------------------------------------
# masked (rand50, alt_*, gap, deny0, all), list-form (rand03, rand64, last, first, only7), empty (none) and full (all) sets;
# deny0 / only7 sit on the tied rows; rand64 pads k = 100.  Slots 8 and 30 are never set.
SLOT_PATTERNS = {0: "rand50", 1: "rand03", 2: "none", 3: "all", 4: "deny0", 5: "only7", 6: "rand64", 7: "alt_first_empty",
                 9: "gap", 12: "last", 20: "alt_last_empty", 31: "first"}
UNSET = (8, 30)
SET = tuple(sorted(SLOT_PATTERNS))


def slot_sets(n):
    return {s: fr.pattern(name, n) for s, name in SLOT_PATTERNS.items()}


# ---- query-to-slot assignments: name -> bytes [nq] ---------------------------------------------------------------------------
ASSIGNMENTS = ("none", "one", "each", "sizes", "g129", "interleaved", "unset")
MIN_NQ = {"none": 1, "one": 1, "each": 1, "sizes": 96, "g129": 129, "interleaved": 1, "unset": 1}


def assignment(name, nq, seed=0):
    rng = np.random.default_rng(seed + 17 * nq)
    every = np.array(SET + (NONE,), np.uint8)
    if name == "none":                       # every query unfiltered
        return np.full(nq, NONE, np.uint8)
    if name == "one":                        # every query the same slot (a masked one)
        return np.full(nq, 0, np.uint8)
    if name == "each":                       # the slots in turn: nq <= 13 is one query per slot, every strip padded to 31 of 32
        return every[np.arange(nq) % every.size]
    if name == "sizes":                      # groups of 31 / 32 / 33 side by side, the rest unfiltered
        out = np.full(nq, NONE, np.uint8)
        out[:31], out[31:63], out[63:96] = 0, 1, 7
        return out
    if name == "g129":                       # a group of 129: more than a workgroup's rows at both strip widths (128, 64)
        out = every[np.arange(nq) % every.size]
        out[:129] = 6
        return rng.permutation(out)
    if name == "interleaved":                # every set slot and NONE in random order
        return rng.choice(every, nq).astype(np.uint8)
    if name == "unset":                      # half the queries on slots that are not set
        out = rng.choice(every, nq).astype(np.uint8)
        out[::2] = np.array(UNSET, np.uint8)[(np.arange(nq)[::2] // 2) % 2]
        return out
    raise KeyError(name)


# ---- the grid of tests/test_gpu_exact_filter_slots.py ------------------------------------------------------------------------
NS, DS, KS, NQS = (33, 6001), (16, 48, 128, 256), (1, 10, 100), (1, 33, 129, 300)
SPLITS, MAPS = (1, 3, 64), (0, 1)


def grid():
    """(n, d, k, nq, assignment, exact_splits, exact_range_map): every (n, d, k) once with the other axes cycling, then every
    assignment at every nq it fits on the 6001-row store, k cycling; plus one query per slot exactly (nq = 13)."""
    cases = []
    for i, (n, d, k) in enumerate(itertools.product(NS, DS, KS)):
        a = ASSIGNMENTS[i % len(ASSIGNMENTS)]
        nq = [q for q in NQS if q >= MIN_NQ[a]][i % len([q for q in NQS if q >= MIN_NQ[a]])]
        cases.append((n, d, k, nq, a, SPLITS[i % 3], MAPS[i % 2]))
    i = 0
    for a in ASSIGNMENTS:
        for nq in NQS:
            if nq >= MIN_NQ[a]:
                cases.append((6001, DS[i % 4], KS[i % 3], nq, a, SPLITS[(i // 3) % 3], MAPS[(i // 2) % 2]))
                i += 1
    cases += [(6001, 48, 100, 13, "each", 3, 1), (33, 16, 10, 13, "each", 1, 0), (6001, 128, 100, 300, "g129", 64, 1),
              (6001, 16, 100, 129, "g129", 1, 0)]
    return sorted(set(cases))
