"""The common fixture of the tag-AND-value tests and their expected values, without new oracle code.

Every id of a corpus b (norm codes clipped, filter_ref) carries the tag tags_ref.assignment gives it and the value
values_ref.assignment gives it.  The two are drawn by independent permutations, so tag sets and value bands really
intersect.  One deterministic change: every id tagged 256 whose value is exactly 0 gets the value 1 -- (256, (0, 0)) is
then a pair whose tag has rows (about 10 %) and whose interval has rows (about 9 %) while NO row carries both, the case that
tells AND from OR and from either predicate alone.  Query q carries PATTERN[q % 13]: a tag and an interval.  Period 13 is
coprime with 64, 2048 and 8192, so a query array sliced at a wrong offset gives wrong answers.

The rule is (t == NONE || tag == t) && lo <= value <= hi.  What query q must return: what any search returns on
filter_ref.poisoned(b, rows that pass its pair); a pair that passes every row is b itself, one that passes none is padding
(FLT_MAX / -1, an empty range)."""
import numpy as np

import filter_ref
import tags_ref as tr
import values_ref as vr
from filter_slots_ref import (FLT_MAX, IVF_PARAMS, GROUPING_PARAMS, first_mismatch, oracle_search,  # noqa: F401
                              same_bits, tiled)

TAG_NONE, VALUE_NONE = tr.NONE, vr.NONE
ABSENT = tr.ABSENT
FULL, VALUED, POINT, INVERTED = vr.FULL, vr.VALUED, vr.POINT, vr.INVERTED
UPPER31 = (0x80000000, 0x800000ff)
BAND31 = (0x7fffff00, 0x800000ff)
UNFILTERED = (TAG_NONE, FULL)
DISJOINT = (256, (0, 0))
FEW = (1007, FULL)
PATTERN = [UNFILTERED, (0, FULL), (TAG_NONE, UPPER31), (0, BAND31), (255, (0, 0)), (256, VALUED), (0xfffe, UPPER31),
           (0, POINT), FEW, (0, (VALUE_NONE, VALUE_NONE)), (ABSENT, FULL), (0, INVERTED), DISJOINT]
PADDING = [(ABSENT, FULL), (0, INVERTED), DISJOINT]  # the pairs no row passes
# The seeds of a corpus' two assignments, by (the corpus' own seed, its code size): those of tags_ref and values_ref unless
# named here.  Chosen so that the fixture conditions of test_tags_values_cpu.py hold: a seed that fails them is replaced,
# the conditions stay.
SEEDS = {(11, 32): (1, None), (42, 16): (1, None)}  # (the tag seed, the value seed); None: the twin fixture's own


def key(pair):
    return (int(pair[0]), (int(pair[1][0]), int(pair[1][1])))


def assignment(b, seeds=None):
    """(labels uint32 ascending, tags uint16, values uint32) of every id of b."""
    if seeds is None:
        seeds = SEEDS.get((b.get("seed"), b.get("code_size")), (None, None))
    labels, tags = tr.assignment(b, seeds[0])
    labels_v, values = vr.assignment(b, seeds[1])
    assert np.array_equal(labels, labels_v)
    values = values.copy()
    values[(tags == 256) & (values == 0)] = 1
    return labels, tags, values


def tag_asg(asg):
    return asg[0], asg[1]


def value_asg(asg):
    return asg[0], asg[2]


def query_tags(nq, first=0):
    """[nq] uint16: the tag of queries first .. first + nq - 1."""
    return np.array([PATTERN[q % len(PATTERN)][0] for q in range(first, first + nq)], np.uint16)


def query_ranges(nq, first=0):
    """[nq, 2] uint32: the interval of queries first .. first + nq - 1."""
    return np.array([PATTERN[q % len(PATTERN)][1] for q in range(first, first + nq)], np.uint32).reshape(nq, 2)


def install(g, asg, parts=1, tags=True, values=True):
    """set_tags and set_values of the assignment (either may be left out), in `parts` incremental calls each."""
    if tags:
        tr.install(g, tag_asg(asg), parts)
    if values:
        vr.install(g, value_asg(asg), parts)
    return g


def without(asg, tags=True, values=True):
    """The assignment as a handle sees it that holds no tag table (tags=False) or no value table: NONE for every id."""
    labels, t, v = asg
    return (labels, t if tags else np.full(len(labels), TAG_NONE, np.uint16),
            v if values else np.full(len(labels), VALUE_NONE, np.uint32))


def _pass(t, v, pair):
    tag, (lo, hi) = key(pair)
    v = v.astype(np.uint64)  # (compared as Python-sized integers: no wrap-around here)
    return ((t == tag) | (tag == TAG_NONE)) & (v >= lo) & (v <= hi)


def labels_in(asg, pair):
    """The labels that pass the pair (those without a tag / a value hold NONE)."""
    return asg[0][_pass(asg[1], asg[2], pair)]


def passing_rows(b, asg, pair):
    """Row mask of b for a query that carries the pair (tag, (lo, hi))."""
    return _pass(tr.row_tags(b["ids"], tag_asg(asg)), vr.row_values(b["ids"], value_asg(asg)), pair)


def pair_corpus(b, asg, pair):
    """The corpus an unfiltered search of which is the search of b by a query that carries the pair."""
    m = passing_rows(b, asg, pair)
    return b if m.all() else filter_ref.poisoned(b, m)


def per_pair(search, b, asg, queries, k, pairs=None):
    """{pair: (dist [nq, k], labels [nq, k])} for every pair of PATTERN: search(corpus, queries) -> (dist, labels, ...) run on
    the pair's corpus; a pair that passes no row needs no search."""
    out = {}
    for p in sorted({key(p) for p in (PATTERN if pairs is None else pairs)}):
        if not passing_rows(b, asg, p).any():
            out[p] = (np.full((len(queries), k), FLT_MAX, np.float32), np.full((len(queries), k), -1, np.int64))
        else:
            res = search(pair_corpus(b, asg, p), queries)
            out[p] = (np.asarray(res[0]).reshape(len(queries), k), np.asarray(res[1]).reshape(len(queries), k))
    return out


def mine(qt, qr, pair):
    """Which queries of (qt, qr) carry the pair."""
    tag, (lo, hi) = key(pair)
    qr = np.asarray(qr).reshape(-1, 2)
    return (np.asarray(qt) == tag) & (qr[:, 0] == lo) & (qr[:, 1] == hi)


def compose(refs, qt, qr, base_index=None):
    """Expected (dist, labels) of a batch: row i is the row base_index[i] (default i) of the reference of query i's pair."""
    qr = np.asarray(qr).reshape(-1, 2)
    nq = len(qr)
    bi = np.arange(nq) if base_index is None else np.asarray(base_index)
    k = next(iter(refs.values()))[0].shape[1]
    d = np.empty((nq, k), np.float32)
    l = np.empty((nq, k), np.int64)
    done = np.zeros(nq, bool)
    for p in {(int(t), (int(r[0]), int(r[1]))) for t, r in zip(qt, qr)}:
        m = mine(qt, qr, p)
        d[m] = refs[p][0][bi[m]]
        l[m] = refs[p][1][bi[m]]
        done |= m
    assert done.all()
    return d, l
