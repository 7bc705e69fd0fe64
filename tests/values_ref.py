"""The common fixture of the row-value tests and their expected values, without new oracle code.

Every id of a corpus b (norm codes clipped, filter_ref) gets at most one uint32 value, seeded: 50 % of the ids a band that
straddles 2^31 (0x7fffff00 + id % 512: a signed compare breaks here), 10 % exactly 0, 10 % exactly 0xfffffffe, 10 % a band
that straddles 2^16 (0xff00 + id % 512: a 16-bit load left over from the tag form breaks here), 1 % exactly 77, 5 % stay
without a value (NONE), and the rest gets 1 000 000 + id % 1000 (about 4 rows each).  Query q carries PATTERN[q % 9].
Period 9 is coprime with 64, 2048 and 8192, so a query array sliced at a wrong offset gives wrong answers.

The rule is lo <= value <= hi, unsigned and inclusive, and a row without a value holds 0xffffffff: nothing is special.
What query q must return: what any search returns on filter_ref.poisoned(b, rows whose value lies in its interval); an
interval that passes every row is b itself, one that passes none is padding (FLT_MAX / -1, an empty range)."""
import numpy as np

import filter_ref
from filter_slots_ref import (FLT_MAX, IVF_PARAMS, GROUPING_PARAMS, first_mismatch, oracle_search,  # noqa: F401
                              same_bits, tiled)

NONE = 0xffffffff
FULL = (0, NONE)
VALUED = (0, 0xfffffffe)
POINT = (77, 77)
INVERTED = (5000, 4999)
FEW = (1_000_007, 1_000_007)
PATTERN = [FULL, VALUED, (0x80000000, 0x800000ff), (0x7fffff00, 0x800000ff), POINT, (0, 0), (0x10000, 0x100ff), INVERTED, FEW]
BAND31, BAND16 = 0x7fffff00, 0xff00
# (what, fraction of the ids): a band's values are base + id % 512
SHARES = [("band31", 0.50), ("zero", 0.10), ("top", 0.10), ("band16", 0.10), ("point", 0.01), ("none", 0.05)]
# The seed of a corpus' assignment, by (the corpus' own seed, its code size); 0 for any other corpus.  Chosen so that the
# fixture conditions of test_values_cpu.py hold (the interval of ~4 rows must be found by one of its queries, the 1 % point
# must leave one of its queries short of 10 results): a seed that fails them is replaced, the conditions stay.
SEEDS = {(11, 8): 0, (11, 16): 2, (11, 32): 0, (81, 12): 1, (85, 28): 6, (42, 16): 15, (43, 16): 0}


def assignment(b, seed=None):
    """(labels uint32 ascending, values uint32): the value of every id of b; NONE for the ones without."""
    if seed is None:
        seed = SEEDS.get((b.get("seed"), b.get("code_size")), 0)
    ids = np.unique(b["ids"]).astype(np.uint32)
    order = np.random.default_rng(9000 + seed).permutation(len(ids))
    values = (1_000_000 + ids % 1000).astype(np.uint32)
    fill = {"band31": (BAND31 + ids % 512).astype(np.uint32), "band16": (BAND16 + ids % 512).astype(np.uint32),
            "zero": np.zeros(len(ids), np.uint32), "top": np.full(len(ids), 0xfffffffe, np.uint32),
            "point": np.full(len(ids), 77, np.uint32), "none": np.full(len(ids), NONE, np.uint32)}
    at = 0
    for what, frac in SHARES:
        n = max(1, int(frac * len(ids)))
        sel = order[at:at + n]
        values[sel] = fill[what][sel]
        at += n
    return ids, values


def query_ranges(nq, first=0):
    """[nq, 2] uint32: the interval of queries first .. first + nq - 1."""
    return np.array([PATTERN[q % len(PATTERN)] for q in range(first, first + nq)], np.uint32).reshape(nq, 2)


def valued(asg):
    """The (labels, values) a set_values call needs: the ids that have a value."""
    m = asg[1] != NONE
    return asg[0][m], asg[1][m]


def install(g, asg, parts=1):
    """set_values of the assignment, in `parts` incremental calls."""
    labels, values = valued(asg)
    for p in range(parts):
        g.set_values(labels[p::parts], values[p::parts])
    return g


def labels_in(asg, rng):
    """The labels whose value lies in the interval (those without a value hold NONE)."""
    v = asg[1].astype(np.uint64)
    return asg[0][(v >= int(rng[0])) & (v <= int(rng[1]))]


def row_values(ids, asg):
    """uint32 per row: the value of its id, NONE where the assignment does not know the id."""
    labels, values = asg
    at = np.minimum(np.searchsorted(labels, ids), len(labels) - 1)
    return np.where(labels[at] == ids, values[at], NONE).astype(np.uint32)


def passing_rows(b, asg, rng):
    """Row mask of b for a query that carries the interval rng = (lo, hi)."""
    v = row_values(b["ids"], asg).astype(np.uint64)  # (compared as Python-sized integers: no wrap-around here)
    return (v >= int(rng[0])) & (v <= int(rng[1]))


def range_corpus(b, asg, rng):
    """The corpus an unfiltered search of which is the search of b by a query that carries rng."""
    m = passing_rows(b, asg, rng)
    return b if m.all() else filter_ref.poisoned(b, m)


def key(rng):
    return (int(rng[0]), int(rng[1]))


def per_range(search, b, asg, queries, k, ranges=None):
    """{(lo, hi): (dist [nq, k], labels [nq, k])} for every interval of PATTERN: search(corpus, queries) -> (dist, labels,
    ...) run on the interval's corpus; an interval that passes no row needs no search."""
    out = {}
    for r in sorted({key(r) for r in (PATTERN if ranges is None else ranges)}):
        if not passing_rows(b, asg, r).any():
            out[r] = (np.full((len(queries), k), FLT_MAX, np.float32), np.full((len(queries), k), -1, np.int64))
        else:
            res = search(range_corpus(b, asg, r), queries)
            out[r] = (np.asarray(res[0]).reshape(len(queries), k), np.asarray(res[1]).reshape(len(queries), k))
    return out


def compose(refs, qr, base_index=None):
    """Expected (dist, labels) of a batch: row i is the row base_index[i] (default i) of the reference of interval qr[i]."""
    qr = np.asarray(qr).reshape(-1, 2)
    nq = len(qr)
    bi = np.arange(nq) if base_index is None else np.asarray(base_index)
    k = next(iter(refs.values()))[0].shape[1]
    d = np.empty((nq, k), np.float32)
    l = np.empty((nq, k), np.int64)
    for r in {key(r) for r in qr}:
        m = (qr[:, 0] == r[0]) & (qr[:, 1] == r[1])
        d[m] = refs[r][0][bi[m]]
        l[m] = refs[r][1][bi[m]]
    return d, l


def mine(qr, rng):
    """Which queries of qr carry rng."""
    qr = np.asarray(qr).reshape(-1, 2)
    return (qr[:, 0] == int(rng[0])) & (qr[:, 1] == int(rng[1]))


def redo_case(base_of):
    """filter_slots_ref.redo_case under values: the overflowing query three times -- on (100, 200), where every id has the
    value 150 but 2.7 % of the query's first list and the query's unfiltered nearest (those have 0x80000005), on the full
    interval, and on the inverted one.  Returns (corpus, queries [3, d], query ranges [3, 2], assignment, parameters)."""
    import filter_slots_ref as fs
    b, q, _, sets, params = fs.redo_case(base_of)
    ids = np.unique(b["ids"]).astype(np.uint32)
    values = np.where(np.isin(ids, sets[31][0]), 0x80000005, 150).astype(np.uint32)
    return b, q, np.array([(100, 200), FULL, INVERTED], np.uint32), (ids, values), params
