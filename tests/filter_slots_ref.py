"""The common fixture of the filter-slot tests and their expected values, without new oracle code.

Slot sets over a corpus b (norm codes clipped, filter_ref): slot 0 allows 50 %, slot 1 allows 1 %, slot 7 denies 10 %,
slot 31 -- the last plane -- allows 10 %, slot 5 is never set.  Query q names PATTERN[q % 7]: neighbouring queries, hence
neighbouring workgroups, read different planes, and period 7 is coprime with 64, 2048 and 8192, so slot bytes sliced at a
wrong offset give wrong answers.

What query q must return: on slot s, what any search returns on filter_ref.poisoned(b, passing rows of s); on NONE, what it
returns on b; on a slot that is not set, padding (FLT_MAX / -1, an empty range)."""
import numpy as np

import filter_ref

NONE = 0xff
UNSET = 5
PATTERN = [0, 31, NONE, 1, 7, UNSET, 31]
SPECS = {0: (0.50, False), 1: (0.01, False), 7: (0.10, True), 31: (0.10, False)}  # slot: (fraction of the ids, deny)
FLT_MAX = np.finfo(np.float32).max


def slot_sets(b, seed=0):
    """{slot: (labels uint32, deny)} over the ids of b."""
    ids = np.unique(b["ids"])
    sets = {}
    for s, (frac, deny) in SPECS.items():
        rng = np.random.default_rng(1000 * seed + s)
        sets[s] = (rng.choice(ids, max(1, int(frac * len(ids))), replace=False).astype(np.uint32), deny)
    return sets


def query_slots(nq, first=0):
    """The slot byte of queries first .. first + nq - 1."""
    return np.array([PATTERN[q % 7] for q in range(first, first + nq)], np.uint8)


def install(g, sets):
    for s, (labels, deny) in sets.items():
        g.set_filter_slot(s, labels, deny=deny)
    return g


def passing_rows(b, sets, slot):
    """Row mask of b under `slot`: everything for NONE, nothing for a slot that is not set."""
    if slot == NONE:
        return np.ones(len(b["ids"]), bool)
    if slot not in sets:
        return np.zeros(len(b["ids"]), bool)
    return filter_ref.passing(b["ids"], sets[slot][0], sets[slot][1])


def slot_corpus(b, sets, slot):
    """The corpus an unfiltered search of which is the filtered search of b under `slot` (NONE: b itself)."""
    return b if slot == NONE else filter_ref.poisoned(b, passing_rows(b, sets, slot))


def per_slot(search, b, sets, queries, k, slots=None):
    """{slot: (dist [nq, k], labels [nq, k])} for every slot of PATTERN: search(corpus, queries) -> (dist, labels, ...) run on
    the slot's corpus; a slot that is not set needs no search."""
    out = {}
    for s in sorted({int(s) for s in (PATTERN if slots is None else slots)}):
        if s != NONE and s not in sets:
            out[s] = (np.full((len(queries), k), FLT_MAX, np.float32), np.full((len(queries), k), -1, np.int64))
        else:
            r = search(slot_corpus(b, sets, s), queries)
            out[s] = (np.asarray(r[0]).reshape(len(queries), k), np.asarray(r[1]).reshape(len(queries), k))
    return out


def compose(refs, qslots, base_index=None):
    """Expected (dist, labels) of a batch: row i is the row base_index[i] (default i) of the reference of slot qslots[i]."""
    nq = len(qslots)
    bi = np.arange(nq) if base_index is None else np.asarray(base_index)
    k = next(iter(refs.values()))[0].shape[1]
    d = np.empty((nq, k), np.float32)
    l = np.empty((nq, k), np.int64)
    for s in np.unique(qslots):
        m = qslots == s
        d[m] = refs[int(s)][0][bi[m]]
        l[m] = refs[int(s)][1][bi[m]]
    return d, l


def same_bits(got, want):
    return np.array_equal(got[1], want[1].reshape(got[1].shape)) and \
        np.array_equal(got[0].view(np.uint32), want[0].reshape(got[0].shape).view(np.uint32))


def first_mismatch(got, want):
    bad = np.nonzero((got[1] != want[1]).any(1) | (got[0].view(np.uint32) != want[0].view(np.uint32)).any(1))[0]
    return None if len(bad) == 0 else (int(bad[0]), got[1][bad[0]][:4], want[1][bad[0]][:4])


# ---- the corpora of the GPU tests and the parameters they are searched with ---------------------------------------------
IVF_PARAMS = (16, 2000, 40)       # nprobe, max_codes, efSearch
GROUPING_PARAMS = (16, 2000, 64)


def tiled(q, n):
    return np.ascontiguousarray(np.tile(q, ((n + len(q) - 1) // len(q), 1))[:n])


def oracle_search(params, k, pruning=False):
    """search(corpus, queries) for per_slot: the oracle with these parameters."""
    import synth

    def search(c, q):
        ox = synth.oracle_index(c)
        ox.set_params(params[0], params[1], params[2], do_pruning=pruning)
        return ox.search_batch(q, k=k)
    return search


def redo_case(base_of):
    """The overflowing query of test_gpu_filter.test_heap_redo_path, three times: on slot 31 (a deny set: 2.7 % of the
    query's first list and the query's unfiltered nearest), under NONE and on slot 5, which is not set.  base_of(**kw) ->
    clipped corpus.  Returns (corpus with that list in descending order, queries [3, d], slot bytes, sets, parameters)."""
    import synth
    from test_gpu_heap_unbounded import OVERFLOW, CAP, _descending
    nprobe, max_codes, ef, k = 8, 20000, 16, 10
    c = base_of(**OVERFLOW[1][0])
    ox = synth.oracle_index(c)
    ox.set_params(nprobe, 10 ** 9, ef)
    cid = ox.search_batch(c["queries"], k=1)[2]
    sizes = np.diff(c["offsets"].astype(np.int64))
    qi = int(np.argmax(sizes[cid[:, 0]]))
    lst = int(cid[qi, 0])
    lo, hi = int(c["offsets"][lst]), int(c["offsets"][lst + 1])
    b = _descending(c, c["queries"][qi], lst)
    ox = synth.oracle_index(b)
    ox.set_params(nprobe, max_codes, ef)
    nearest = ox.search_batch(b["queries"][[qi]], k=1)[1][0, 0]
    assert nearest >= 0
    deny = np.unique(np.concatenate([c["ids"][lo:hi][::37], [nearest]])).astype(np.uint32)
    assert (hi - lo) - len(deny) > CAP + 200, "fixture: the passing rows of the first probed list must outgrow the stream"
    q = np.ascontiguousarray(np.repeat(b["queries"][[qi]], 3, axis=0))
    return b, q, np.array([31, NONE, UNSET], np.uint8), {31: (deny, True)}, (nprobe, max_codes, ef, k)
