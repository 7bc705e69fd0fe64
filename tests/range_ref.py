"""Expected values of range search (ivfhnsw_gpu_range_search) from the oracle as it stands.

The oracle has no range entry point.  Its k-search with k >= the codes it scores (OrcStats.ncode) admits every scored code
with a finite distance, so the heap array it returns IS the scored set: labels with their distance bits.  The expected
range result of a query is the part of that set below the radius.  Scan order for IVFADC is restated in numpy (ivf_order:
the ids of the probed lists in probe order, empty lists skipped, stopping behind the list that brings the count to
max_codes, IndexIVF_HNSW.cpp:267-292); Grouping has no such restatement and is pinned by the tests in other ways."""
import numpy as np

import synth

_CACHE = {}


def scored_batch(c, queries, nprobe, max_codes, ef, pruning=False, key=None):
    """For every query: what the oracle's search scores.  Returns a dict with cid / cd [nq, nprobe] (the oracle's coarse
    stage), ncode [nq], and per query labels[i] (int64, sorted ascending) with dists[i] (float32, same order).
    key (hashable): cache the result for the session under it."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    ox = synth.oracle_index(c)
    ox.set_params(nprobe, max_codes, ef, do_pruning=pruning)
    queries = np.ascontiguousarray(queries, np.float32)
    _, _, cid, cd, _ = ox.search_batch(queries, k=1)
    ncode, labels, dists = [], [], []
    for i in range(len(queries)):
        st = ox.search_coarse(queries[i], cid[i], cd[i], k=1)[2]
        n = int(st.ncode)
        d, l, st2 = ox.search_coarse(queries[i], cid[i], cd[i], k=max(n, 1))
        assert int(st2.ncode) == n
        keep = l >= 0
        order = np.argsort(l[keep], kind="stable")
        labels.append(l[keep][order])
        dists.append(d[keep][order])
        ncode.append(n)
    out = dict(cid=cid, cd=cd, ncode=np.array(ncode, np.int64), labels=labels, dists=dists)
    if key is not None:
        _CACHE[key] = out
    return out


def pooled_quantile(sc, q):
    """The q-quantile of the scored distances of the whole batch, as float32."""
    return np.float32(np.quantile(np.concatenate(sc["dists"]).astype(np.float64), q))


def expected_set(sc, i, radius):
    """Query i's expected results as a sorted array of (label, distance bits) pairs."""
    keep = sc["dists"][i] < np.float32(radius)
    return np.stack([sc["labels"][i][keep], sc["dists"][i][keep].view(np.uint32).astype(np.int64)], axis=1)


def result_set(lims, dist, lab, i):
    """Query i's part of a range result in the form expected_set returns."""
    a, b = int(lims[i]), int(lims[i + 1])
    order = np.argsort(lab[a:b], kind="stable")
    return np.stack([lab[a:b][order], dist[a:b][order].view(np.uint32).astype(np.int64)], axis=1)


def ivf_order(c, cid_row, max_codes):
    """The ids an IVFADC search scores for one query, in scan order (slots >= nc are padding)."""
    off = np.asarray(c["offsets"]).astype(np.int64)
    out, n = [], 0
    for lst in cid_row:
        lst = int(lst)
        if lst >= len(off) - 1 or off[lst + 1] == off[lst]:
            continue
        out.append(np.asarray(c["ids"][off[lst]:off[lst + 1]]).astype(np.int64))
        n += len(out[-1])
        if n >= max_codes:
            break
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def expected_ivf(c, sc, max_codes, radius, cid=None, subset=False):
    """(lims u64 [nq + 1], distances f32, labels i64) of an IVFADC range search: the scored set below the radius, in scan
    order.  Needs unique labels (the distance of a scan position is looked up by its label).  cid: coarse results other
    than the ones sc was scored with; subset: they probe only some of those lists (the distance of a code depends on
    its own list alone)."""
    cid = sc["cid"] if cid is None else cid
    lims, dd, ll = [0], [], []
    for i in range(len(cid)):
        order = ivf_order(c, cid[i], max_codes)
        lab, dist = sc["labels"][i], sc["dists"][i]
        assert len(np.unique(lab)) == len(lab) and np.isin(order, lab).all(), "labels must be unique and scored"
        assert subset or len(lab) == len(order), "every scored code must be admitted"
        d = dist[np.searchsorted(lab, order)]
        keep = d < np.float32(radius)
        dd.append(d[keep])
        ll.append(order[keep])
        lims.append(lims[-1] + int(keep.sum()))
    return np.array(lims, np.uint64), np.concatenate(dd).astype(np.float32), np.concatenate(ll).astype(np.int64)


def same_range(got, want):
    """lims, distance bits and labels of two range results are equal."""
    return (np.array_equal(np.asarray(got[0], np.uint64), np.asarray(want[0], np.uint64)) and
            np.array_equal(got[2], want[2]) and
            np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32)))


def filtered(res, passing):
    """A range result with the entries whose label is not in `passing` deleted and lims rebuilt."""
    lims, dist, lab = res
    keep = np.isin(lab, passing)
    cum = np.concatenate([[0], np.cumsum(keep)])
    return cum[np.asarray(lims, np.int64)].astype(np.uint64), dist[keep], lab[keep]
