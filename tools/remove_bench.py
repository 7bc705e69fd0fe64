#!/usr/bin/env python3
"""Removals by label from a device-resident index (ivfhnsw_gpu_remove_ids) at the metric's shape.

  1. bench.py's synthetic-1B-pq16-nc993127-nprobe32 corpus (lists generated on the device, 10^9 codes, ids = the
     running index).  Removals of 1 k, 1 M and 10 M distinct random labels below n_total through remove_ids_dev: wall
     milliseconds per call (the call returns when the new arrays are in place), and the bytes it moves -- the ids the
     mark reads, the old arrays the compaction reads, the new arrays it writes (M + 5 bytes per code each) -- against the
     6.29 TB/s copy rate of the guide.  n_removed must equal the number of labels (checked).
  2. search_dev queries/s (10 k queries, k = 1) before and after the removals: the layout is the same CSR.
  3. The path a removal replaces: the class filters every list on the host and uploads the whole index again.  At a
     shape the host holds (--reupload-codes, 10^8 by default) that is a boolean filter of the flat CSR arrays (the
     lower bound of the per-list filtering), then upload_ivf.
usage: python tools/remove_bench.py [--workload NAME] [--sizes 1000,1000000,10000000] [--reupload-codes N (0: skip)]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_TBS = 6.29


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synthetic-1B-pq16-nc993127-nprobe32")
    ap.add_argument("--sizes", default="1000,1000000,10000000")
    ap.add_argument("--reupload-codes", type=int, default=100_000_000)
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

    def qps(reps=10):
        for _ in range(5):
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        g.sync()
        t = time.perf_counter()
        for _ in range(reps):
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        g.sync()
        return nq * reps / (time.perf_counter() - t)

    out["qps_before"] = qps()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    n_local = c.n_total
    rows = []
    # Label set i (of K - 1) takes residues i mod K, so the sets are disjoint and every label is present once: ids are
    # the running index.  Label 0 (residue 0) goes first: that call allocates the bitmap, mask and count buffers the
    # handle keeps, and is reported apart.
    sizes = [int(x) for x in args.sizes.split(",")]
    K = len(sizes) + 1
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)  # torch's stream is not the handle's
    t = time.perf_counter()
    n_rm = g.remove_ids_dev(1, zero)
    out["first_call_ms"] = (time.perf_counter() - t) * 1e3
    assert n_rm == 1, n_rm
    n_local -= 1
    for i, n in enumerate(sizes, 1):
        lab = torch.unique(torch.randint(0, c.n_total // K, (n,), device=dev, generator=gen, dtype=torch.int64)) * K + i
        labels = lab.to(torch.int32)   # labels below 2^31: the same bits as uint32
        m = labels.numel()
        torch.cuda.synchronize(dev)
        before = n_local
        t = time.perf_counter()
        n_rm = g.remove_ids_dev(m, labels)
        ms = (time.perf_counter() - t) * 1e3
        assert n_rm == m, (n_rm, m)
        n_local -= n_rm
        # ids read by the mark, old rows read and new rows written by the compaction (codes + norm code + id)
        moved = before * 4 + before * (c.M + 5) + n_local * (c.M + 5)
        rows.append({"labels": m, "removed": n_rm, "codes_before": before, "ms": ms, "GB_moved": moved / 1e9,
                     "TBps": moved / ms / 1e9, "of_copy_rate": moved / ms / 1e9 / COPY_TBS})
        log("[remove_bench] remove %d labels from %d codes: %.2f ms, %.2f TB/s" % (m, before, ms, rows[-1]["TBps"]))
        del lab, labels
    out["removals"] = rows
    out["qps_after"] = qps()
    out["memory_GB_after"] = g.memory_bytes() / 1e9
    g.close()
    torch.cuda.empty_cache()

    # the re-upload path at a host-sized shape
    n = args.reupload_codes
    if n <= 0:
        print(json.dumps(out))
        return
    rng = np.random.default_rng(3)
    sizes = np.bincount(rng.integers(0, c.nc, n), minlength=c.nc).astype(np.uint64)
    codes = np.frombuffer(rng.bytes(n * c.M), np.uint8).reshape(n, c.M)
    ncodes = np.frombuffer(rng.bytes(n), np.uint8)
    ids = rng.permutation(n).astype(np.uint32)
    labels = rng.choice(n, 10 ** 6, replace=False).astype(np.uint32)
    lid = np.repeat(np.arange(c.nc), sizes.astype(np.int64))
    t = time.perf_counter()
    drop = np.isin(ids, labels)
    keep = ~drop
    fi, fc, fn = ids[keep], codes[keep], ncodes[keep]
    off = np.concatenate([[0], np.cumsum(sizes - np.bincount(lid[drop], minlength=c.nc))]).astype(np.uint64)
    t_filter = time.perf_counter() - t
    h = pkg.GpuIndex(0)
    t = time.perf_counter()
    h.upload_ivf(c.d, c.M, off, fi, fc, fn, np.zeros(c.nc, np.float32), np.zeros(256 * c.d, np.float32),
                 np.zeros(256, np.float32))
    t_up = time.perf_counter() - t
    h.close()
    out["reupload"] = {"codes": n, "labels": len(labels), "filter_s": t_filter, "upload_s": t_up,
                       "total_s": t_filter + t_up, "per_1B_s": (t_filter + t_up) * 1e9 / n}
    log("[remove_bench] host filter + re-upload of %d codes: filter %.2fs + upload %.2fs" % (n, t_filter, t_up))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
