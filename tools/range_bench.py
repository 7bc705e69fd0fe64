#!/usr/bin/env python3
"""Range search (ivfhnsw_gpu_range_search_dev) at the metric's shape, on one handle in one run.

  bench.py's synthetic-1B-pq16-nc993127-nprobe32 corpus, 10 k queries, (nprobe, max_codes, efSearch) = (32, 10000, 80).
  Baseline: the k = 1 search_dev step (the path bench.py times; range search does not touch it).
  Measured: range_search_dev at radii taken from the scored distances of a 64-query sample so that about 0, 1e-4, 1e-2
  and all of the scored codes are returned.  Per radius: wall milliseconds per call (the call returns when the results
  are complete), in a second loop with set_profiling the time of the count pass (accounted as the scan stage) and of
  the fill pass (the select stage), results per second, and the bytes the handle holds.
usage: python tools/range_bench.py [--workload NAME] [--nq 10000] [--reps 10]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synthetic-1B-pq16-nc993127-nprobe32")
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    import bench
    import synth
    pkg = ge.load_pkg()
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
