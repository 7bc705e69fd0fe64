#!/usr/bin/env python3
"""Recall of the FILTERED IVF search against the filtered truth.

On the small SIFT-like uint8 corpus of tests/rerank_ref.uint8_recall_corpus (ids = row numbers of the base), for pass
fractions 1, 1/2, 1/8 and 1/32: the same random allow set is installed as the index's label filter
(ivfhnsw_gpu_set_filter: the IVF search returns only allowed ids) and as the base filter (ivfhnsw_gpu_set_base_filter:
the exact search returns the true nearest allowed rows).  Reported per fraction and per (nprobe, max_codes, efSearch)
setting: Recall@1 = share of queries whose true nearest allowed row is the IVF search's first result, and Recall@10 =
share of the true 10 nearest allowed rows among the IVF search's 10 results.
With --slots: 32 seeded random allow sets, pass fractions cycling 1/2, 1/8 and 1/32, are installed as
filter slots and as base filter slots; the queries are spread over the 32 slots and NONE; ONE search_slots call is scored
against ONE exact_search_slots call, Recall@1 and Recall@10 per pass fraction.
With --tags: every row gets one of 1 024 tags -- tag t < 4 holds 1/8 of the rows each, the other half is
spread evenly over the tags 4..1023 -- and the queries are dealt over a sample of tags and NONE; ONE search_tags call is
scored against the truth of a tagged search, the per-tag loop of set_base_filter + exact_search.
With --base-tags: the same corpus and tags, installed on the store as well (ivfhnsw_gpu_set_base_tags); the
queries are dealt over ALL 1 024 tags and NONE, and ONE search_tags call is scored against ONE exact_search_tags call.
With --values: every row gets a distinct value (a seeded permutation of 0..n-1: a timestamp), and the
queries are dealt over a handful of sample intervals -- four of pass fraction 1/8 that overlap one another, five of about
1/2000, and (0, 0xffffffff); ONE search_values call is scored against the per-interval loop of set_base_filter + exact_search.
With --base-values: the same corpus and values, installed on the store as well
(ivfhnsw_gpu_set_base_values); every query names an interval of its own, and ONE search_values call is scored against ONE
exact_search_values call.
usage: python tools/filter_recall.py [--seed 77] [--slots | --tags | --base-tags | --values | --base-values] [--out result.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRACTIONS = (1, 2, 8, 32)
SETTINGS = ((16, 10000, 64), (32, 20000, 80))  # (nprobe, max_codes, efSearch), as tools/range_bench.py --recall


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def recall_pair(lab, truth):
    """(Recall@1, Recall@10) of search labels [m, 10] against true labels [m, 10] (-1 = no such row)."""
    r1 = float((lab[:, 0] == truth[:, 0]).mean())
    hits = sum(np.intersect1d(lab[i][lab[i] >= 0], truth[i][truth[i] >= 0]).size for i in range(len(lab)))
    return r1, hits / max(1, int((truth >= 0).sum()))


def upload(pkg, c):
    g = pkg.GpuIndex(0)
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"])
    g.upload_quantizer(c["counts"], c["links"], c["centroids"], c.get("enterpoint", 0))
    g.upload_base(c["base"])
    return g


def filtered_recall(pkg, seed=77, corpus=None, allow_sets=None, query_idx=None, settings=SETTINGS):
    """corpus: a dict as rerank_ref.uint8_recall_corpus returns it (default: that corpus); allow_sets: [(name, row numbers)]
    in place of the random sets of FRACTIONS; query_idx: only these queries."""
    if corpus is None:
        import rerank_ref
        corpus = rerank_ref.uint8_recall_corpus(pkg, seed=seed)
    c = corpus
    g = upload(pkg, c)
    qf = c["queries"] if query_idx is None else c["queries"][query_idx]
    q8 = qf.astype(np.uint8)  # integer-valued, 0..255
    nq, n = len(q8), len(c["base"])
    rng = np.random.default_rng(seed + 1)
    if allow_sets is None:
        allow_sets = [("1/%d" % den, np.arange(n, dtype=np.uint32) if den == 1 else
                       np.sort(rng.choice(n, n // den, replace=False)).astype(np.uint32)) for den in FRACTIONS]
    rows = []
    for name, allow in allow_sets:
        g.set_filter(allow)
        g.set_base_filter(allow)
        assert g.filter_info()[1] == g.base_filter_info()[1] == allow.size
        _, truth = g.exact_search(q8, 10)
        for nprobe, max_codes, ef in settings:
            _, lab = g.search(qf, 10, nprobe, max_codes, efSearch=ef)
            r1, r10 = recall_pair(lab, truth)
            row = {"pass_fraction": name, "rows_passing": int(allow.size), "nprobe": nprobe, "max_codes": max_codes,
                   "efSearch": ef, "recall_at_1": r1, "recall_at_10": r10}
            rows.append(row)
            log("[filter_recall] %s of %d rows, nprobe %d max_codes %d: Recall@1 %.4f, Recall@10 %.4f"
                % (name, n, nprobe, max_codes, r1, r10))
    g.close()
    return {"corpus": "uint8_recall_corpus(seed=%d)" % seed, "rows": n, "nq": nq, "filtered_recall": rows}


SLOT_FRACTIONS = (2, 8, 32)
SLOT_NONE = 0xff


def slot_allow_sets(n, seed):
    """The 32 allow sets of the --slots run: slot s holds a random n / SLOT_FRACTIONS[s % 3] of the row numbers."""
    rng = np.random.default_rng(seed + 2)
    return [np.sort(rng.choice(n, n // SLOT_FRACTIONS[s % 3], replace=False)).astype(np.uint32) for s in range(32)]


def slots_recall(pkg, seed=77, corpus=None, settings=SETTINGS):
    """Recall of one search_slots call against one exact_search_slots call, per pass fraction.  corpus: a dict as
    rerank_ref.uint8_recall_corpus returns it (ids = row numbers of the base); default: that corpus itself.  Returns the
    report; its "truth" / "query_slots" / "sets" entries are the arrays themselves, for a test to compare."""
    if corpus is None:
        import rerank_ref
        corpus = rerank_ref.uint8_recall_corpus(pkg, seed=seed)
    c = corpus
    g = upload(pkg, c)
    qf = c["queries"]
    q8 = qf.astype(np.uint8)
    nq, n = len(q8), len(c["base"])
    sets = slot_allow_sets(n, seed)
    for s, allow in enumerate(sets):
        g.set_filter_slot(s, allow)
        g.set_base_filter_slot(s, allow)
        assert g.filter_slot_info(s)[1] == g.base_filter_slot_info(s)[1] == allow.size
    qs = (np.arange(nq) % 33).astype(np.uint8)  # the 32 slots and NONE in turn
    qs[qs == 32] = SLOT_NONE
    _, truth = g.exact_search_slots(q8, 10, qs)
    rows = []
    den_of = np.array([1 if b == SLOT_NONE else SLOT_FRACTIONS[b % 3] for b in qs])
    per_slot = []
    for nprobe, max_codes, ef in settings:
        _, lab = g.search_slots(qf, 10, qs, nprobe, max_codes, efSearch=ef)
        per_slot.append([recall_pair(lab[qs == b], truth[qs == b]) for b in range(32)])
        for den in (1,) + SLOT_FRACTIONS:
            idx = np.flatnonzero(den_of == den)
            r1, r10 = recall_pair(lab[idx], truth[idx])
            rows.append({"pass_fraction": "1/%d" % den, "queries": int(idx.size), "nprobe": nprobe, "max_codes": max_codes,
                         "efSearch": ef, "recall_at_1": r1, "recall_at_10": r10})
            log("[filter_recall] slots, 1/%d (%d queries), nprobe %d max_codes %d: Recall@1 %.4f, Recall@10 %.4f"
                % (den, idx.size, nprobe, max_codes, r1, r10))
    g.close()
    return {"rows": n, "nq": nq, "slots": 32, "slots_recall": rows, "truth": truth, "query_slots": qs, "sets": sets,
            "per_slot": per_slot}


TAG_NONE = 0xffff
TAG_SAMPLE = (0, 1, 2, 3, 4, 5, 100, 511, 1023, TAG_NONE)  # four large tags, five small ones, no tag


def tag_assignment(n, seed):
    """uint16 [n]: the tag of row (= id) i.  Tags 0..3 hold n / 8 rows each, tags 4..1023 share the other half."""
    rng = np.random.default_rng(seed + 3)
    tags = np.empty(n, np.uint16)
    order = rng.permutation(n)
    big = n // 8
    for t in range(4):
        tags[order[t * big:(t + 1) * big]] = t
    rest = order[4 * big:]
    tags[rest] = 4 + np.arange(len(rest)) % 1020
    return tags


def tags_recall(pkg, seed=77, corpus=None, settings=SETTINGS):
    """Recall of one search_tags call against the per-tag loop of set_base_filter + exact_search, per tag of TAG_SAMPLE."""
    if corpus is None:
        import rerank_ref
        corpus = rerank_ref.uint8_recall_corpus(pkg, seed=seed)
    c = corpus
    g = upload(pkg, c)
    qf = c["queries"]
    q8 = qf.astype(np.uint8)
    nq, n = len(q8), len(c["base"])
    tags = tag_assignment(n, seed)
    g.set_tags(np.arange(n, dtype=np.uint32), tags)
    assert g.tags_info() == (n, n, n)
    qt = np.array([TAG_SAMPLE[i % len(TAG_SAMPLE)] for i in range(nq)], np.uint16)
    truth = np.empty((nq, 10), np.int64)
    for t in TAG_SAMPLE:
        mine = np.flatnonzero(qt == t)
        if t == TAG_NONE:
            g.clear_base_filter()
        else:
            rows = np.flatnonzero(tags == t).astype(np.uint32)
            assert g.tag_rows(t) == rows.size
            g.set_base_filter(rows)
        truth[mine] = g.exact_search(q8[mine], 10)[1]
    g.clear_base_filter()
    rows_out = []
    for nprobe, max_codes, ef in settings:
        _, lab = g.search_tags(qf, 10, qt, nprobe, max_codes, efSearch=ef)
        assert g.last_scan_kernel().endswith("+tags")
        for name, sel in (("1/8 (tags 0..3)", qt < 4), ("~1/2040 (small tags)", (qt >= 4) & (qt != TAG_NONE)),
                          ("1 (no tag)", qt == TAG_NONE)):
            idx = np.flatnonzero(sel)
            r1, r10 = recall_pair(lab[idx], truth[idx])
            rows_out.append({"pass_fraction": name, "queries": int(idx.size), "nprobe": nprobe, "max_codes": max_codes,
                             "efSearch": ef, "recall_at_1": r1, "recall_at_10": r10})
            log("[filter_recall] tags, %s (%d queries), nprobe %d max_codes %d: Recall@1 %.4f, Recall@10 %.4f"
                % (name, idx.size, nprobe, max_codes, r1, r10))
    g.close()
    return {"rows": n, "nq": nq, "tags": 1024, "tags_recall": rows_out}


def base_tags_recall(pkg, seed=77, corpus=None, settings=SETTINGS):
    """Recall of one search_tags call against ONE exact_search_tags call, the queries dealt over ALL 1 024 tags and NONE
    (the --tags corpus and tag assignment).  Returns the report; its "truth" / "query_tags" / "tags" entries are the arrays
    themselves, for a test to compare."""
    if corpus is None:
        import rerank_ref
        corpus = rerank_ref.uint8_recall_corpus(pkg, seed=seed)
    c = corpus
    g = upload(pkg, c)
    qf = c["queries"]
    q8 = qf.astype(np.uint8)
    nq, n = len(q8), len(c["base"])
    tags = tag_assignment(n, seed)
    rows = np.arange(n, dtype=np.uint32)
    g.set_tags(rows, tags)      # ids = row numbers of the base: the index and the store carry the same tags
    g.set_base_tags(rows, tags)
    assert g.tags_info() == (n, n, n) and g.base_tags_info() == (n, n, np.unique(tags).size)
    # the tags of TAG_SAMPLE first (what --tags scores), then every other tag in a seeded order, dealt in turn
    others = np.setdiff1d(np.arange(1024), TAG_SAMPLE)
    every = np.concatenate([TAG_SAMPLE, np.random.default_rng(seed + 4).permutation(others)]).astype(np.uint16)
    qt = every[np.arange(nq) % every.size]
    _, truth = g.exact_search_tags(q8, 10, qt)
    rows_out = []
    for nprobe, max_codes, ef in settings:
        _, lab = g.search_tags(qf, 10, qt, nprobe, max_codes, efSearch=ef)
        assert g.last_scan_kernel().endswith("+tags")
        for name, sel in (("1/8 (tags 0..3)", qt < 4), ("~1/2040 (small tags)", (qt >= 4) & (qt != TAG_NONE)),
                          ("1 (no tag)", qt == TAG_NONE)):
            idx = np.flatnonzero(sel)
            r1, r10 = recall_pair(lab[idx], truth[idx]) if idx.size else (float("nan"), float("nan"))
            rows_out.append({"pass_fraction": name, "queries": int(idx.size), "tags_named": int(np.unique(qt[idx]).size),
                             "nprobe": nprobe, "max_codes": max_codes, "efSearch": ef, "recall_at_1": r1, "recall_at_10": r10})
            log("[filter_recall] base tags, %s (%d queries on %d tags), nprobe %d max_codes %d: Recall@1 %.4f, Recall@10 %.4f"
                % (name, idx.size, np.unique(qt[idx]).size, nprobe, max_codes, r1, r10))
    g.close()
    return {"rows": n, "nq": nq, "tags": 1024, "base_tags_recall": rows_out, "truth": truth, "query_tags": qt, "tags_of_rows": tags}


VALUE_NONE = 0xffffffff


def value_intervals(n):
    """The sample intervals over values 0..n-1: (name of the pass fraction, lo, hi)."""
    w8, w2k = n // 8, max(1, n // 2000)
    out = [("1/8", a, a + w8 - 1) for a in (0, w8 // 2, n // 2 - w8 // 3, n - w8)]  # neighbours overlap: no tag partition
    out += [("~1/2000", a, a + w2k - 1) for a in (0, n // 7, n // 3, n // 2, n - w2k)]
    out.append(("1 (0, 0xffffffff)", 0, VALUE_NONE))
    return out


def values_recall(pkg, seed=77, corpus=None, settings=SETTINGS):
    """Recall of one search_values call against the per-interval loop of set_base_filter + exact_search."""
    if corpus is None:
        import rerank_ref
        corpus = rerank_ref.uint8_recall_corpus(pkg, seed=seed)
    c = corpus
    g = upload(pkg, c)
    qf = c["queries"]
    q8 = qf.astype(np.uint8)
    nq, n = len(q8), len(c["base"])
    values = np.random.default_rng(seed + 5).permutation(n).astype(np.uint32)  # the value of row (= id) i
    g.set_values(np.arange(n, dtype=np.uint32), values)
    assert g.values_info() == (n, n, n)
    sample = value_intervals(n)
    pick = np.arange(nq) % len(sample)
    qr = np.array([(sample[i][1], sample[i][2]) for i in pick], np.uint32)
    truth = np.empty((nq, 10), np.int64)
    for i, (_, lo, hi) in enumerate(sample):
        mine = np.flatnonzero(pick == i)
        if hi == VALUE_NONE:
            g.clear_base_filter()
        else:
            rows = np.flatnonzero((values >= lo) & (values <= hi)).astype(np.uint32)
            assert g.value_rows(lo, hi) == rows.size
            g.set_base_filter(rows)
        truth[mine] = g.exact_search(q8[mine], 10)[1]
    g.clear_base_filter()
    rows_out = []
    names = np.array([s_[0] for s_ in sample])
    for nprobe, max_codes, ef in settings:
        _, lab = g.search_values(qf, 10, qr, nprobe, max_codes, efSearch=ef)
        assert g.last_scan_kernel().endswith("+values")
        for name in ("1/8", "~1/2000", "1 (0, 0xffffffff)"):
            idx = np.flatnonzero(names[pick] == name)
            r1, r10 = recall_pair(lab[idx], truth[idx])
            rows_out.append({"pass_fraction": name, "queries": int(idx.size), "nprobe": nprobe, "max_codes": max_codes,
                             "efSearch": ef, "recall_at_1": r1, "recall_at_10": r10})
            log("[filter_recall] values, %s (%d queries), nprobe %d max_codes %d: Recall@1 %.4f, Recall@10 %.4f"
                % (name, idx.size, nprobe, max_codes, r1, r10))
    g.close()
    return {"rows": n, "nq": nq, "intervals": len(sample), "values_recall": rows_out}


def base_values_recall(pkg, seed=77, corpus=None, settings=SETTINGS, sample_only=False):
    """Recall of one search_values call against ONE exact_search_values call (the --values corpus and value assignment,
    installed on the store as well).  The queries name a whole batch of distinct intervals: query q takes, in turn, a width
    of 1/8 of the values, of about 1/2000, or (0, 0xffffffff), at a seeded start of its own.  sample_only: the queries are
    dealt over the ten sample intervals of --values instead, and the figures are the ones --values prints.  Returns the
    report; its "truth" / "query_ranges" / "values_of_rows" entries are the arrays themselves, for a test to compare."""
    if corpus is None:
        import rerank_ref
        corpus = rerank_ref.uint8_recall_corpus(pkg, seed=seed)
    c = corpus
    g = upload(pkg, c)
    qf = c["queries"]
    q8 = qf.astype(np.uint8)
    nq, n = len(q8), len(c["base"])
    values = np.random.default_rng(seed + 5).permutation(n).astype(np.uint32)  # the value of row (= id) i
    rows = np.arange(n, dtype=np.uint32)
    g.set_values(rows, values)       # ids = row numbers of the base: the index and the store hold the same values
    g.set_base_values(rows, values)
    assert g.values_info() == (n, n, n) and g.base_values_info() == (n, n)
    if sample_only:
        sample = value_intervals(n)
        pick = np.arange(nq) % len(sample)
        qr = np.array([(sample[i][1], sample[i][2]) for i in pick], np.uint32)
        names = np.array([s_[0] for s_ in sample])[pick]
    else:
        w8, w2k = n // 8, max(1, n // 2000)
        start = np.random.default_rng(seed + 6).integers(0, n, nq)
        kind = np.arange(nq) % 3
        names = np.array(["1/8", "~1/2000", "1 (0, 0xffffffff)"])[kind]
        width = np.where(kind == 0, w8, w2k)
        lo = np.minimum(start, n - width)
        qr = np.stack([np.where(kind == 2, 0, lo), np.where(kind == 2, VALUE_NONE, lo + width - 1)], 1).astype(np.uint32)
    distinct = int(np.unique(qr, axis=0).shape[0])
    _, truth = g.exact_search_values(q8, 10, qr)
    rows_out = []
    for nprobe, max_codes, ef in settings:
        _, lab = g.search_values(qf, 10, qr, nprobe, max_codes, efSearch=ef)
        assert g.last_scan_kernel().endswith("+values")
        for name in ("1/8", "~1/2000", "1 (0, 0xffffffff)"):
            idx = np.flatnonzero(names == name)
            r1, r10 = recall_pair(lab[idx], truth[idx]) if idx.size else (float("nan"), float("nan"))
            rows_out.append({"pass_fraction": name, "queries": int(idx.size), "nprobe": nprobe, "max_codes": max_codes,
                             "efSearch": ef, "recall_at_1": r1, "recall_at_10": r10})
            log("[filter_recall] base values, %s (%d queries), nprobe %d max_codes %d: Recall@1 %.4f, Recall@10 %.4f"
                % (name, idx.size, nprobe, max_codes, r1, r10))
    g.close()
    return {"rows": n, "nq": nq, "intervals": distinct, "base_values_recall": rows_out, "truth": truth, "query_ranges": qr,
            "values_of_rows": values}


def tag_value_pairs(n):
    """The sample pairs: (name of the pass fraction, tag, lo, hi)."""
    iv = value_intervals(n)
    eighths = [x for x in iv if x[0] == "1/8"]
    small = [x for x in iv if x[0] == "~1/2000"]
    out = [("1/64 (1/8 x 1/8)", t, lo, hi) for t in range(4) for _, lo, hi in eighths]
    out += [("1/8 (tag, FULL)", t, 0, VALUE_NONE) for t in range(4)]
    out += [("1/8 (NONE, interval)", TAG_NONE, lo, hi) for _, lo, hi in eighths]
    out += [("~1/2040 (small tag, FULL)", t, 0, VALUE_NONE) for t in (4, 5, 100, 511, 1023)]
    out += [("~1/2000 (NONE, small interval)", TAG_NONE, lo, hi) for _, lo, hi in small]
    out.append(("1 (NONE, FULL)", TAG_NONE, 0, VALUE_NONE))
    return out


def tags_values_recall(pkg, seed=77, corpus=None, settings=SETTINGS):
    """Recall of one search_tags_values call against the per-pair loop of set_base_filter + exact_search."""
    if corpus is None:
        import rerank_ref
        corpus = rerank_ref.uint8_recall_corpus(pkg, seed=seed)
    c = corpus
    g = upload(pkg, c)
    qf = c["queries"]
    q8 = qf.astype(np.uint8)
    nq, n = len(q8), len(c["base"])
    tags = tag_assignment(n, seed)
    values = np.random.default_rng(seed + 5).permutation(n).astype(np.uint32)  # the value of row (= id) i
    g.set_tags(np.arange(n, dtype=np.uint32), tags)
    g.set_values(np.arange(n, dtype=np.uint32), values)
    sample = tag_value_pairs(n)
    pick = np.arange(nq) % len(sample)
    qt = np.array([sample[i][1] for i in pick], np.uint16)
    qr = np.array([(sample[i][2], sample[i][3]) for i in pick], np.uint32)
    truth = np.empty((nq, 10), np.int64)
    passing = {}
    for i, (name, t, lo, hi) in enumerate(sample):
        mine = np.flatnonzero(pick == i)
        if t == TAG_NONE and hi == VALUE_NONE:
            g.clear_base_filter()
            passing.setdefault(name, []).append(n)
        else:
            rows = np.flatnonzero(((tags == t) | (t == TAG_NONE)) & (values >= lo) & (values <= hi)).astype(np.uint32)
            assert g.tag_value_rows(t, lo, hi) == rows.size
            passing.setdefault(name, []).append(int(rows.size))
            g.set_base_filter(rows)
        truth[mine] = g.exact_search(q8[mine], 10)[1]
    g.clear_base_filter()
    rows_out = []
    names = np.array([s_[0] for s_ in sample])
    for nprobe, max_codes, ef in settings:
        _, lab = g.search_tags_values(qf, 10, qt, qr, nprobe, max_codes, efSearch=ef)
        assert g.last_scan_kernel().endswith("+tags+values")
        for name in dict.fromkeys(names.tolist()):
            idx = np.flatnonzero(names[pick] == name)
            r1, r10 = recall_pair(lab[idx], truth[idx])
            rows_out.append({"pass_fraction": name, "rows_passing_mean": float(np.mean(passing[name])), "queries": int(idx.size),
                             "nprobe": nprobe, "max_codes": max_codes, "efSearch": ef, "recall_at_1": r1, "recall_at_10": r10})
            log("[filter_recall] tags+values, %s (%d queries, %.0f rows pass), nprobe %d max_codes %d: Recall@1 %.4f, Recall@10 %.4f"
                % (name, idx.size, np.mean(passing[name]), nprobe, max_codes, r1, r10))
    g.close()
    return {"rows": n, "nq": nq, "pairs": len(sample), "tags_values_recall": rows_out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--tags", action="store_true", help="one search_tags call against the per-tag base-filter loop")
    ap.add_argument("--base-tags", action="store_true", help="one search_tags call against one exact_search_tags call, "
                                                              "the queries over all 1 024 tags")
    ap.add_argument("--slots", action="store_true", help="one search_slots call against one exact_search_slots call")
    ap.add_argument("--values", action="store_true", help="one search_values call against the per-interval base-filter loop")
    ap.add_argument("--base-values", action="store_true", help="one search_values call against one exact_search_values call, "
                                                                "every query an interval of its own")
    ap.add_argument("--tags-values", action="store_true", help="one search_tags_values call against the per-pair base-filter loop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    if args.base_tags:
        out = base_tags_recall(pkg, args.seed)
        out = {k: v for k, v in out.items() if k not in ("truth", "query_tags", "tags_of_rows")}
        out["corpus"] = "uint8_recall_corpus(seed=%d)" % args.seed
    elif args.base_values:
        out = base_values_recall(pkg, args.seed)
        out = {k: v for k, v in out.items() if k not in ("truth", "query_ranges", "values_of_rows")}
        out["corpus"] = "uint8_recall_corpus(seed=%d)" % args.seed
    elif args.tags_values:
        out = tags_values_recall(pkg, args.seed)
        out["corpus"] = "uint8_recall_corpus(seed=%d)" % args.seed
    elif args.values:
        out = values_recall(pkg, args.seed)
        out["corpus"] = "uint8_recall_corpus(seed=%d)" % args.seed
    elif args.tags:
        out = tags_recall(pkg, args.seed)
        out["corpus"] = "uint8_recall_corpus(seed=%d)" % args.seed
    elif args.slots:
        out = slots_recall(pkg, args.seed)
        out = {k: v for k, v in out.items() if k not in ("truth", "query_slots", "sets", "per_slot")}
        out["corpus"] = "uint8_recall_corpus(seed=%d)" % args.seed
    else:
        out = filtered_recall(pkg, args.seed)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
