#!/usr/bin/env python3
"""Additions to a device-resident Grouping index (ivfhnsw_gpu_append_grouping) at the metric's shape.

  1. bench.py's grouping-1B-pq16-nc993127-nsubc64-opq-pruning corpus (lists generated on the device, 10^9 codes).
     append_grouping_dev of 1 M and 10 M codes at uniformly random (list, sub-group): wall milliseconds per call (host
     clock around a call that returns when the new arrays are in place) and the bytes it moves -- old arrays read + new
     arrays written (M + 5 bytes per code each) + the batch + the sub-group sizes table read and written -- against the
     6.29 TB/s copy rate of the guide.
  2. In the same run, alternating with 1: append_ivf_dev of the same n on an IVFADC handle over the same offsets and
     code books (two handles of about 26 GB each plus one append's new arrays at a time).  This is the yardstick: the
     same box, the same minute, the merge the grouping append was modelled on.  The ratio of the two is reported with
     the spread of the repeats.
     Beside them: the wall time of one hipMalloc + hipFree of an array the size of the codes, which every append of
     either kind pays three times over and which differs between boxes by two orders of magnitude.
  3. search_dev queries/s (10 k queries, k = 1, pruning) on the Grouping handle before, after (every list is longer:
     more codes per query), and after the added codes were removed again (the original lists: the same CSR layout).
  4. The path replaced: the class flattens every list on the host and uploads the whole index and its four tables
     again.  At a shape the host holds (--reupload-codes, 10^8 by default): a gather of the rows into one CSR, then
     upload_ivf + upload_grouping.
usage: python tools/add_groups_bench.py [--workload NAME] [--sizes 1000000,10000000] [--reps 3] [--reupload-codes N]"""
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
NSUBC = 64


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="grouping-1B-pq16-nc993127-nsubc64-opq-pruning")
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
    tb = c.tb
    # the IVFADC corpus of the same size: the same offsets and code books, no grouping tables
    f = pkg.GpuIndex(0)
    f.upload_ivf_synthetic(c.d, c.M, tb["offsets"], c.centroid_norms, tb["pq_centroids"], tb["norm_table"], c.code_seed,
                           opq_A=c.opq_A)
    out = {"workload": args.workload, "nc": c.nc, "code_size": c.M, "nsubc": NSUBC, "codes": c.n_total}
    nq = 10000
    q = torch.from_numpy(c.queries(nq, 4321)).to(dev)
    dd = torch.empty((nq, 1), dtype=torch.float32, device=dev)
    ll = torch.empty((nq, 1), dtype=torch.int64, device=dev)

    def qps(reps=10):
        for _ in range(5):
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef, do_pruning=True)
        g.sync()
        t = time.perf_counter()
        for _ in range(reps):
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef, do_pruning=True)
        g.sync()
        return nq * reps / (time.perf_counter() - t)

    out["qps_before"] = [qps() for _ in range(3)]

    def alloc_probe():
        """hipMalloc + hipFree of one array the size of the codes (what every append does three times over), in ms:
        boxes differ in this by two orders of magnitude, and it is no part of the merge."""
        torch.cuda.empty_cache()
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        buf = torch.empty(c.n_total * c.M, dtype=torch.uint8, device=dev)
        del buf
        torch.cuda.empty_cache()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) * 1e3

    out["alloc_free_16GB_ms"] = [alloc_probe() for _ in range(3)]
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    n_g = n_f = c.n_total
    next_id = c.n_total
    table_bytes = c.nc * NSUBC * 4
    rows = []
    first = True
    for n in [int(x) for x in args.sizes.split(",")]:
        grp_ms, ivf_ms, grp_b, ivf_b = [], [], [], []
        for rep in range(args.reps + (1 if first else 0)):
            li = torch.randint(0, c.nc, (n,), device=dev, generator=gen, dtype=torch.int32)
            si = torch.randint(0, NSUBC, (n,), device=dev, generator=gen, dtype=torch.int32)
            ids = torch.arange(next_id, next_id + n, device=dev, dtype=torch.int64).to(torch.int32)
            codes = torch.randint(0, 256, (n, c.M), device=dev, generator=gen, dtype=torch.uint8)
            ncodes = torch.randint(0, 256, (n,), device=dev, generator=gen, dtype=torch.uint8)
            torch.cuda.synchronize(dev)  # torch's stream is not the handle's
            t = time.perf_counter()
            g.append_grouping_dev(n, li, si, ids, codes, ncodes)
            ms_g = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            f.append_ivf_dev(n, li, ids, codes, ncodes)
            ms_f = (time.perf_counter() - t) * 1e3
            row = c.M + 5
            bytes_f = n_f * row + (n_f + n) * row + n * (row + 4)
            bytes_g = n_g * row + (n_g + n) * row + n * (row + 8) + 2 * table_bytes
            n_g += n
            n_f += n
            next_id += n
            del li, si, ids, codes, ncodes
            if first and rep == 0:
                # the first call of each handle allocates the work buffers it keeps: reported apart
                out["first_call_ms"] = {"append_grouping": ms_g, "append_ivf": ms_f}
                continue
            grp_ms.append(ms_g)
            ivf_ms.append(ms_f)
            grp_b.append(bytes_g)
            ivf_b.append(bytes_f)
            log("[add_groups_bench] n %d rep %d: append_grouping %.2f ms, append_ivf %.2f ms" % (n, rep, ms_g, ms_f))
        first = False
        gm, fm = float(np.median(grp_ms)), float(np.median(ivf_ms))
        rows.append({"n": n, "append_grouping_ms": grp_ms, "append_ivf_ms": ivf_ms,
                     "append_grouping_GB": grp_b[0] / 1e9, "append_ivf_GB": ivf_b[0] / 1e9,
                     "append_grouping_TBps": float(np.median(np.array(grp_b) / np.array(grp_ms))) / 1e9,
                     "append_ivf_TBps": float(np.median(np.array(ivf_b) / np.array(ivf_ms))) / 1e9,
                     "ratio_median": gm / fm, "ratios": [a / b for a, b in zip(grp_ms, ivf_ms)],
                     "bytes_ratio": grp_b[0] / ivf_b[0]})
        rows[-1]["append_grouping_of_copy_rate"] = rows[-1]["append_grouping_TBps"] / COPY_TBS
        rows[-1]["append_ivf_of_copy_rate"] = rows[-1]["append_ivf_TBps"] / COPY_TBS
    out["appends"] = rows
    f.close()
    out["qps_after"] = [qps() for _ in range(3)]
    # the added codes make every list longer, so a search scores more codes than before; taken out again (remove_ids_dev,
    # DESIGN.md 3.11) the lists are the original ones, and so must the rate be
    added = torch.arange(c.n_total, next_id, device=dev, dtype=torch.int64).to(torch.int32)
    torch.cuda.synchronize(dev)
    assert g.remove_ids_dev(added.numel(), added) == next_id - c.n_total
    del added
    out["qps_after_removing_them"] = [qps() for _ in range(3)]
    out["memory_GB_after"] = g.memory_bytes() / 1e9
    g.close()
    torch.cuda.empty_cache()

    # the re-upload path at a host-sized shape
    n = args.reupload_codes
    if n <= 0:
        print(json.dumps(out))
        return
    rng = np.random.default_rng(3)
    nc = c.nc
    flat = rng.integers(0, nc * NSUBC, n)
    sg = np.bincount(flat, minlength=nc * NSUBC).reshape(nc, NSUBC).astype(np.uint32)
    codes = np.frombuffer(rng.bytes(n * c.M), np.uint8).reshape(n, c.M)
    ncodes = np.frombuffer(rng.bytes(n), np.uint8)
    ids = rng.permutation(n).astype(np.uint32)
    order = np.argsort(flat, kind="stable")
    t = time.perf_counter()
    fi, fc, fn = ids[order], codes[order], ncodes[order]    # the gather device_upload_common does list by list
    off = np.concatenate([[0], np.cumsum(sg.sum(1, dtype=np.int64))]).astype(np.uint64)
    t_flat = time.perf_counter() - t
    h = pkg.GpuIndex(0)
    t = time.perf_counter()
    h.upload_ivf(c.d, c.M, off, fi, fc, fn, np.zeros(nc, np.float32), np.zeros(256 * c.d, np.float32),
                 np.zeros(256, np.float32))
    h.upload_grouping(NSUBC, c.gt["alphas"], c.gt["nn_centroid_idxs"], sg, c.gt["inter_centroid_dists"])
    t_up = time.perf_counter() - t
    h.close()
    out["reupload"] = {"codes": n, "flatten_s": t_flat, "upload_s": t_up, "total_s": t_flat + t_up,
                       "per_1B_s": (t_flat + t_up) * 1e9 / n}
    log("[add_groups_bench] host flatten + re-upload of %d codes: flatten %.2fs + upload %.2fs" % (n, t_flat, t_up))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
