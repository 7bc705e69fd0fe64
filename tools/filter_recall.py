#!/usr/bin/env python3
"""Recall of the FILTERED IVF search against the filtered truth.

On the small SIFT-like uint8 corpus of tests/rerank_ref.uint8_recall_corpus (ids = row numbers of the base), for pass
fractions 1, 1/2, 1/8 and 1/32: the same random allow set is installed as the index's label filter
(ivfhnsw_gpu_set_filter: the IVF search returns only allowed ids) and as the base filter (ivfhnsw_gpu_set_base_filter:
the exact search returns the true nearest allowed rows).  Reported per fraction and per (nprobe, max_codes, efSearch)
setting: Recall@1 = share of queries whose true nearest allowed row is the IVF search's first result, and Recall@10 =
share of the true 10 nearest allowed rows among the IVF search's 10 results.
usage: python tools/filter_recall.py [--seed 77] [--out result.json]"""
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


def filtered_recall(pkg, seed=77):
    import rerank_ref
    c = rerank_ref.uint8_recall_corpus(pkg, seed=seed)
    g = pkg.GpuIndex(0)
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"])
    g.upload_quantizer(c["counts"], c["links"], c["centroids"], 0)
    g.upload_base(c["base"])
    qf = c["queries"]
    q8 = qf.astype(np.uint8)  # integer-valued, 0..255
    nq, n = len(q8), len(c["base"])
    rng = np.random.default_rng(seed + 1)
    rows = []
    for den in FRACTIONS:
        allow = np.arange(n, dtype=np.uint32) if den == 1 else \
            np.sort(rng.choice(n, n // den, replace=False)).astype(np.uint32)
        g.set_filter(allow)
        g.set_base_filter(allow)
        assert g.filter_info()[1] == g.base_filter_info()[1] == allow.size
        _, truth = g.exact_search(q8, 10)
        for nprobe, max_codes, ef in SETTINGS:
            _, lab = g.search(qf, 10, nprobe, max_codes, efSearch=ef)
            r1 = float((lab[:, 0] == truth[:, 0]).mean())
            hits = sum(np.intersect1d(lab[i][lab[i] >= 0], truth[i][truth[i] >= 0]).size for i in range(nq))
            r10 = hits / max(1, int((truth >= 0).sum()))
            row = {"pass_fraction": "1/%d" % den, "rows_passing": int(allow.size), "nprobe": nprobe, "max_codes": max_codes,
                   "efSearch": ef, "recall_at_1": r1, "recall_at_10": r10}
            rows.append(row)
            log("[filter_recall] 1/%d of %d rows, nprobe %d max_codes %d: Recall@1 %.4f, Recall@10 %.4f"
                % (den, n, nprobe, max_codes, r1, r10))
    g.close()
    return {"corpus": "uint8_recall_corpus(seed=%d)" % seed, "rows": n, "nq": nq, "filtered_recall": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    out = filtered_recall(pkg, args.seed)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
