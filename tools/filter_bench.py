#!/usr/bin/env python3
"""The label filter of a handle (ivfhnsw_gpu_set_filter) at the metric's shape.

On bench.py's synthetic-1B-pq16-nc993127-nprobe32 corpus (lists generated on the device, 10^9 codes, ids = the running
index):
  1. set_filter_dev of 1 k, 10 M and 500 M distinct random labels below n_total: wall milliseconds per call (the call
     returns when the mask is installed) and the rows that pass (checked against the number of labels).  The first call
     allocates the bitmap and the mask, and is reported apart.
  2. search_dev queries/s (10 k queries, k = 1) of ONE handle in one run, in this order: unfiltered; deny nothing (every
     row passes: the cost of the filtered kernels alone); allow 50 %; allow 10 %; allow 1 %; unfiltered again.  The
     reference point of every filtered figure is the unfiltered pair of the same run.
usage: python tools/filter_bench.py [--workload NAME] [--sizes 1000,10000000,500000000] [--fractions 0.5,0.1,0.01]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synthetic-1B-pq16-nc993127-nprobe32")
    ap.add_argument("--sizes", default="1000,10000000,500000000")
    ap.add_argument("--fractions", default="0.5,0.1,0.01")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    import bench
    import synth
    pkg = ge.load_pkg()
    dev = torch.device("cuda", 0)
    c = bench.Corpus(pkg, synth, args.workload, 1234, dev, 0)
    g = c.g
    out = {"workload": args.workload, "nc": c.nc, "code_size": c.M, "codes": c.n_total}
    nq = 10000
    q = torch.from_numpy(c.queries(nq, 4321)).to(dev)
    dd = torch.empty((nq, 1), dtype=torch.float32, device=dev)
    ll = torch.empty((nq, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # torch's stream is not the handle's

    def qps(reps=10):
        for _ in range(5):
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        g.sync()
        t = time.perf_counter()
        for _ in range(reps):
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        g.sync()
        return nq * reps / (time.perf_counter() - t), g.last_scan_kernel()

    def labels_of(n, seed):
        """n distinct labels below n_total: every K-th id from a random phase, K = n_total // n (ids are the running index)"""
        K = max(1, c.n_total // n)
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        phase = int(torch.randint(0, K, (1,), device=dev, generator=gen).item())
        lab = torch.arange(n, device=dev, dtype=torch.int64) * K + phase
        lab = lab[torch.randperm(n, device=dev, generator=gen)] if n <= 10 ** 7 else lab
        t = lab.to(torch.int32)  # the same bits as uint32
        torch.cuda.synchronize(dev)
        return t

    def timed_set(n, deny, seed):
        lab = labels_of(n, seed) if n else None
        t = time.perf_counter()
        g.set_filter_dev(n, lab, deny=deny)
        ms = (time.perf_counter() - t) * 1e3
        mode, passing, total = g.filter_info()
        assert total == c.n_total and passing == (total - n if deny else n), (mode, passing, total, n)
        return ms, passing

    # 1. installing
    ms, _ = timed_set(1, False, 1)
    out["first_call_ms"] = ms
    rows = []
    for i, n in enumerate(int(x) for x in args.sizes.split(",")):
        ms, passing = timed_set(n, False, 10 + i)
        ms2, _ = timed_set(n, True, 20 + i)
        rows.append({"labels": n, "allow_ms": ms, "deny_ms": ms2, "rows_passing_allow": passing})
        log("[filter_bench] set_filter_dev %d labels: allow %.2f ms, deny %.2f ms" % (n, ms, ms2))
    out["set_filter_dev"] = rows
    out["memory_GB_with_filter"] = g.memory_bytes() / 1e9
    g.clear_filter()

    # 2. searching, one handle, one run
    runs = []

    def record(name):
        v, kernel = qps()
        runs.append({"filter": name, "qps": v, "kernel": kernel, "rows_passing": g.filter_info()[1]})
        log("[filter_bench] %-18s %.0f queries/s  (%s)" % (name, v, kernel))

    record("none")
    timed_set(0, True, 0)
    record("deny nothing")
    for f in (float(x) for x in args.fractions.split(",")):
        timed_set(int(c.n_total * f), False, 30)
        record("allow %g %%" % (100 * f))
    g.clear_filter()
    record("none (again)")
    out["search"] = runs
    base = [r["qps"] for r in runs if r["filter"].startswith("none")]
    out["unfiltered_spread"] = abs(base[0] - base[1]) / max(base)
    for r in runs:
        r["of_unfiltered"] = r["qps"] / (sum(base) / len(base))
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
