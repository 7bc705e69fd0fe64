#!/usr/bin/env python3
"""Appends to a device-resident index (ivfhnsw_gpu_append_ivf) at the metric's shape.

  1. bench.py's synthetic-1B-pq16-nc993127-nprobe32 corpus (lists generated on the device, 10^9 codes).  Appends of
     1 M and 10 M codes with uniformly random list ids through append_ivf_dev: wall milliseconds per call (the call
     returns when the new arrays are in place), and the bytes the merge moves (old arrays read + new arrays written)
     against the 6.29 TB/s copy rate of the guide.
  2. search_dev queries/s (10 k queries, k = 1) before and after the appends: the layout is the same CSR.
  3. The path an append replaces: the class flattens every list on the host and uploads the whole index again.  At a
     shape the host holds (--reupload-codes, 10^8 by default) the flatten is a gather of the rows into one CSR (what
     device_upload_common copies list by list), then upload_ivf.
usage: python tools/append_bench.py [--workload NAME] [--sizes 1000000,10000000] [--reps 3] [--reupload-codes N]"""
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
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=3)
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

    def qps(reps=5):
        for _ in range(2):
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
    for n in [int(x) for x in args.sizes.split(",")]:
        li = torch.randint(0, c.nc, (n,), dtype=torch.int32, device=dev, generator=gen)
        ids = torch.arange(n, dtype=torch.int32, device=dev)
        codes = torch.randint(0, 256, (n, c.M), dtype=torch.uint8, device=dev, generator=gen)
        ncodes = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=gen)
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.reps):
            t = time.perf_counter()
            g.append_ivf_dev(n, li, ids, codes, ncodes)
            ms.append((time.perf_counter() - t) * 1e3)
            # bytes: old rows read, all rows written (codes + norm code + id), plus the batch itself
            moved = (n_local + (n_local + n)) * (c.M + 5) + n * (c.M + 5)
            n_local += n
            rows.append({"n": n, "codes_before": n_local - n, "ms": ms[-1], "TBps": moved / ms[-1] / 1e9,
                         "of_copy_rate": moved / ms[-1] / 1e9 / COPY_TBS})
            log("[append_bench] append %d codes to %d: %.2f ms, %.2f TB/s" % (n, n_local - n, ms[-1], rows[-1]["TBps"]))
        del li, ids, codes, ncodes
    out["appends"] = rows
    out["qps_after"] = qps()
    out["memory_GB_after"] = g.memory_bytes() / 1e9
    g.close()
    torch.cuda.empty_cache()

    # the re-upload path at a host-sized shape
    n = args.reupload_codes
    rng = np.random.default_rng(3)
    sizes = np.bincount(rng.integers(0, c.nc, n), minlength=c.nc).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    codes = np.frombuffer(rng.bytes(n * c.M), np.uint8).reshape(n, c.M)
    ncodes = np.frombuffer(rng.bytes(n), np.uint8)
    ids = np.arange(n, dtype=np.uint32)
    perm = rng.permutation(n)           # the rows as the host lists hold them: scattered
    t = time.perf_counter()
    fc, fn, fi = codes[perm], ncodes[perm], ids[perm]
    t_flat = time.perf_counter() - t
    h = pkg.GpuIndex(0)
    t = time.perf_counter()
    h.upload_ivf(c.d, c.M, off, fi, fc, fn, np.zeros(c.nc, np.float32), np.zeros(256 * c.d, np.float32),
                 np.zeros(256, np.float32))
    t_up = time.perf_counter() - t
    h.close()
    out["reupload"] = {"codes": n, "flatten_s": t_flat, "upload_s": t_up, "total_s": t_flat + t_up,
                       "per_1B_s": (t_flat + t_up) * 1e9 / n}
    log("[append_bench] re-upload of %d codes: flatten %.2fs + upload %.2fs" % (n, t_flat, t_up))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
