#!/usr/bin/env python3
"""Range search (ivfhnsw_gpu_range_search_dev) at the metric's shape, on one handle in one run.

  bench.py's synthetic-1B-pq16-nc993127-nprobe32 corpus, 10 k queries, (nprobe, max_codes, efSearch) = (32, 10000, 80).
  Baseline: the k = 1 search_dev step (the path bench.py times; range search does not touch it).
  Measured: range_search_dev at radii taken from the scored distances of a 64-query sample so that about 0, 1e-4, 1e-2
  and all of the scored codes are returned.  Per radius: wall milliseconds per call (the call returns when the results
  are complete), in a second loop with set_profiling the time of the count pass (accounted as the scan stage) and of
  the fill pass (the select stage), results per second, and the bytes the handle holds.
  --recall instead: on the small SIFT-like uint8 corpus of tests/rerank_ref.uint8_recall_corpus, the IVF range search
  against the exact one (ivfhnsw_gpu_exact_range_search) at radii taken as quantiles of the exact 10th
  neighbour's distance: recall |IVF range & exact range| / |exact range| and precision |IVF range & exact range| /
  |IVF range| of the label sets (the ADC distance is an approximation: neither is 1), and the mean results per query.
  --recall --allow-fraction F: the same under a filter -- a random allow set of F * n rows is installed as the index's
  label filter and as the base filter (ids are row numbers on this corpus), so the filtered IVF range
  search is scored against the filtered exact one.
usage: python tools/range_bench.py [--workload NAME] [--nq 10000] [--reps 10] [--recall [--allow-fraction F]]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def recall(pkg, quantiles=(0.1, 0.5, 0.9), allow_fraction=None):
    import rerank_ref
    c = rerank_ref.uint8_recall_corpus(pkg, seed=77)
    g = pkg.GpuIndex(0)
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"])
    g.upload_quantizer(c["counts"], c["links"], c["centroids"], 0)
    g.upload_base(c["base"])
    qf = c["queries"]
    q8 = qf.astype(np.uint8)  # integer-valued, 0..255
    nq, n = len(q8), len(c["base"])
    npass = n
    if allow_fraction is not None:  # the same rows pass the IVF search and the exact one
        npass = max(1, int(allow_fraction * n))
        allow = np.sort(np.random.default_rng(78).choice(n, npass, replace=False)).astype(np.uint32)
        g.set_filter(allow)
        g.set_base_filter(allow)
        assert g.filter_info()[1] == g.base_filter_info()[1] == npass
    kd, _ = g.exact_search(q8, 10)
    rows = []
    for x in quantiles:
        r = float(np.quantile(kd[:, 9], x, method="lower"))
        el, _, elab = g.exact_range_search(q8, r)
        ekeys = np.repeat(np.arange(nq, dtype=np.int64), np.diff(el.astype(np.int64))) * n + elab
        for nprobe, max_codes, ef in ((16, 10000, 64), (32, 20000, 80)):
            il, _, ilab = g.range_search(qf, r, nprobe, max_codes, efSearch=ef)
            ikeys = np.unique(np.repeat(np.arange(nq, dtype=np.int64), np.diff(il.astype(np.int64))) * n + ilab)
            both = np.intersect1d(ikeys, ekeys, assume_unique=True).size
            row = {"quantile_of_10th_neighbour": x, "radius": r, "nprobe": nprobe, "max_codes": max_codes, "efSearch": ef,
                   "exact_per_query": ekeys.size / nq, "ivf_per_query": ikeys.size / nq,
                   "recall": both / max(1, ekeys.size), "precision": both / max(1, ikeys.size)}
            rows.append(row)
            log("[range_bench] radius %.0f (q%.2f) nprobe %d: exact %.2f / query, ivf %.2f / query, recall %.4f, precision %.4f"
                % (r, x, nprobe, row["exact_per_query"], row["ivf_per_query"], row["recall"], row["precision"]))
    g.close()
    return {"corpus": "uint8_recall_corpus(seed=77)", "rows": n, "rows_passing": npass, "allow_fraction": allow_fraction, "nq": nq,
            "range_recall": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synthetic-1B-pq16-nc993127-nprobe32")
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--recall", action="store_true", help="recall and precision against the exact range search instead")
    ap.add_argument("--allow-fraction", type=float, default=None,
                    help="with --recall: score under a random allow set of this fraction of the rows")
    args = ap.parse_args()
    if args.allow_fraction is not None and (not args.recall or not 0 < args.allow_fraction <= 1):
        ap.error("--allow-fraction F goes with --recall, 0 < F <= 1")
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    if args.recall:
        print(json.dumps(recall(pkg, allow_fraction=args.allow_fraction)))
        return
    import bench
    import synth
    dev = torch.device("cuda", 0)
    c = bench.Corpus(pkg, synth, args.workload, 1234, dev, 0)
    g = c.g
    nq, reps = args.nq, args.reps
    out = {"workload": args.workload, "nc": c.nc, "code_size": c.M, "codes": c.n_total, "nq": nq,
           "params": [c.nprobe, c.max_codes, c.ef]}
    q = torch.from_numpy(c.queries(nq, 4321)).to(dev)
    dd = torch.empty((nq, 1), dtype=torch.float32, device=dev)
    ll = torch.empty((nq, 1), dtype=torch.int64, device=dev)
    lims = torch.empty((nq + 1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # torch's stream is not the handle's

    def k1_step_ms():
        for _ in range(5):
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        g.sync()
        t = time.perf_counter()
        for _ in range(reps):
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        g.sync()
        return (time.perf_counter() - t) * 1e3 / reps

    out["k1_step_ms"] = k1_step_ms()
    out["k1_scan_kernel"] = g.last_scan_kernel()
    out["codes_scored_per_batch"] = g.last_scan_counts()[0]
    log("[range_bench] k = 1 step: %.3f ms (%s)" % (out["k1_step_ms"], out["k1_scan_kernel"]))

    def rsd(r, n=nq):
        return g.range_search_dev(n, q, float(r), lims, c.nprobe, c.max_codes, efSearch=c.ef)

    # radii: quantiles of what a sample of the batch scores
    total = rsd(np.inf, 64)
    sample = np.sort(g.range_results(0, total)[0])
    radii = [("none", float(sample[0])), ("1e-4", float(sample[int(1e-4 * len(sample))])),
             ("1e-2", float(sample[int(1e-2 * len(sample))])), ("all", float("inf"))]
    mem0 = g.memory_bytes()
    rows = []
    for name, r in radii:
        for _ in range(3):
            total = rsd(r)
        t = time.perf_counter()
        for _ in range(reps):
            rsd(r)
        ms = (time.perf_counter() - t) * 1e3 / reps
        g.set_profiling(True)
        g.reset_stage_ms()
        for _ in range(reps):
            rsd(r)
        st = g.stage_ms()
        g.set_profiling(False)
        row = {"radius": name, "radius_value": r, "results": total, "step_ms": ms,
               "count_pass_ms": st["scan"][0] / reps, "fill_pass_ms": st["select"][0] / reps,
               "coarse_ms": st["coarse"][0] / reps, "plan_table_ms": (st["lut"][0] + st["plan"][0]) / reps,
               "results_per_s": total / (ms * 1e-3), "result_bytes": 12 * total,
               "memory_bytes_over_start": g.memory_bytes() - mem0, "kernel": g.last_scan_kernel()}
        rows.append(row)
        log("[range_bench] %-5s %12d results: step %.3f ms, count %.3f ms, fill %.3f ms" %
            (name, total, ms, row["count_pass_ms"], row["fill_pass_ms"]))
    out["range"] = rows
    out["k1_step_ms_after"] = k1_step_ms()
    out["memory_GB"] = g.memory_bytes() / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
