"""The common fixture of the row-tag tests and their expected values, without new oracle code.

Every id of a corpus b (norm codes clipped, filter_ref) gets at most one 16-bit tag, seeded and disjoint: tag 0 -> 50 % of
the ids, 1 -> 1 %, 255 -> 10 %, 256 -> 10 %, 0xfffe -> 10 %, 5 % stay untagged (NONE), and the rest is spread over the tags
1000..1999 by id % 1000.  Query q names PATTERN[q % 9]; no label carries 4242.  255 is the filter slots' "none" byte and
an ordinary tag here, and 255 / 256 straddle the byte boundary of the 16-bit load.  Period 9 is coprime with 64, 2048 and
8192, so query tags sliced at a wrong offset give wrong answers.

What query q must return: on tag t, what any search returns on filter_ref.poisoned(b, rows whose id is tagged t); on NONE,
what it returns on b; on a tag no label carries, padding (FLT_MAX / -1, an empty range)."""
import numpy as np

import filter_ref
from filter_slots_ref import (FLT_MAX, IVF_PARAMS, GROUPING_PARAMS, compose, first_mismatch, oracle_search,  # noqa: F401
                              same_bits, tiled)

NONE = 0xffff
ABSENT = 4242
PATTERN = [0, 0xfffe, NONE, 1, 255, 256, ABSENT, 1007, 0xfffe]
SHARES = [(0, 0.50), (1, 0.01), (255, 0.10), (256, 0.10), (0xfffe, 0.10)]  # tag: fraction of the ids
UNTAGGED = 0.05
# The seed of a corpus' assignment, by (the corpus' own seed, its code size); 0 for any other corpus.  Chosen so that the
# fixture conditions of test_tags_cpu.py hold (a tag of ~4 rows must be found by one of its queries, the 1 % tag must leave
# one of its queries short of 10 results): a seed that fails them is replaced, the conditions stay.
SEEDS = {(11, 8): 1, (11, 16): 5, (11, 32): 0, (81, 12): 0, (85, 28): 7, (42, 16): 37, (43, 16): 10}


def assignment(b, seed=None):
    """(labels uint32 ascending, tags uint16): the tag of every id of b; NONE for the untagged ones."""
    if seed is None:
        seed = SEEDS.get((b.get("seed"), b.get("code_size")), 0)
    ids = np.unique(b["ids"]).astype(np.uint32)
    order = np.random.default_rng(7000 + seed).permutation(len(ids))
    tags = (1000 + ids % 1000).astype(np.uint16)
    at = 0
    for t, frac in SHARES + [(NONE, UNTAGGED)]:
        n = max(1, int(frac * len(ids)))
        tags[order[at:at + n]] = t
        at += n
    return ids, tags


def query_tags(nq, first=0):
    """The tag of queries first .. first + nq - 1."""
    return np.array([PATTERN[q % len(PATTERN)] for q in range(first, first + nq)], np.uint16)


def tagged(asg):
    """The (labels, tags) a set_tags call needs: the ids that carry a tag."""
    m = asg[1] != NONE
    return asg[0][m], asg[1][m]


def install(g, asg, parts=1):
    """set_tags of the assignment, in `parts` incremental calls."""
    labels, tags = tagged(asg)
    for p in range(parts):
        g.set_tags(labels[p::parts], tags[p::parts])
    return g


def labels_of(asg, tag):
    return asg[0][asg[1] == tag]


def row_tags(ids, asg):
    """uint16 per row: the tag of its id, NONE where the assignment does not know the id."""
    labels, tags = asg
    at = np.minimum(np.searchsorted(labels, ids), len(labels) - 1)
    return np.where(labels[at] == ids, tags[at], NONE).astype(np.uint16)


def passing_rows(b, asg, tag):
    """Row mask of b for a query tagged `tag`: everything for NONE."""
    if tag == NONE:
        return np.ones(len(b["ids"]), bool)
    return row_tags(b["ids"], asg) == tag


def tag_corpus(b, asg, tag):
    """The corpus an unfiltered search of which is the search of b by a query tagged `tag` (NONE: b itself)."""
    return b if tag == NONE else filter_ref.poisoned(b, passing_rows(b, asg, tag))


def per_tag(search, b, asg, queries, k, tags=None):
    """{tag: (dist [nq, k], labels [nq, k])} for every tag of PATTERN: search(corpus, queries) -> (dist, labels, ...) run on
    the tag's corpus; a tag that no row carries needs no search."""
    out = {}
    for t in sorted({int(t) for t in (PATTERN if tags is None else tags)}):
        if t != NONE and not passing_rows(b, asg, t).any():
            out[t] = (np.full((len(queries), k), FLT_MAX, np.float32), np.full((len(queries), k), -1, np.int64))
        else:
            r = search(tag_corpus(b, asg, t), queries)
            out[t] = (np.asarray(r[0]).reshape(len(queries), k), np.asarray(r[1]).reshape(len(queries), k))
    return out


def redo_case(base_of):
    """filter_slots_ref.redo_case under tags: the overflowing query three times -- tagged 0xfffe, which every id carries but
    2.7 % of the query's first list and the query's unfiltered nearest (those carry 255), under NONE, and tagged 4242.
    Returns (corpus, queries [3, d], query tags, assignment, parameters)."""
    import filter_slots_ref as fs
    b, q, _, sets, params = fs.redo_case(base_of)
    ids = np.unique(b["ids"]).astype(np.uint32)
    tags = np.where(np.isin(ids, sets[31][0]), 255, 0xfffe).astype(np.uint16)
    return b, q, np.array([0xfffe, NONE, ABSENT], np.uint16), (ids, tags), params
