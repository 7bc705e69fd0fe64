#!/usr/bin/env python3
"""searchDisk's exact re-rank on the device (kernels_rerank.hip): what it costs at the metric's shape and what it buys.

  1. The bench corpus (bench.py's synthetic-1B-pq16-nc993127-nprobe32 tables and graph, lists generated on the device)
     plus a 10^9 x 128 uint8 base store filled on the device in ~1 GB torch chunks through upload_base_dev.  For 10 k
     queries at k = 10 and kc in {10, 20, 100, 1000}: search_dev (kc) and rerank_dev milliseconds from HIP events on
     one stream, rows/s and TB/s of gathered row bytes, and the whole step against search_dev at k = 1 and k = 10.
  2. A small SIFT-like uint8 corpus (tests/rerank_ref.uint8_recall_corpus): Recall@1 / Recall@10 with and without the
     re-rank.
usage: python tools/rerank_bench.py [--workload NAME] [--reps 10] [--kcs 10,20,100,1000] [--no-recall] [--no-speed]"""
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


def speed(args, pkg, torch):
    import bench
    import synth
    dev = torch.device("cuda", 0)
    c = bench.Corpus(pkg, synth, args.workload, 1234, dev, 0)
    g = c.g
    n, d, nq, k = c.n_total, c.d, 10000, 10
    stream = torch.cuda.current_stream(dev)
    g.set_stream(stream.cuda_stream)  # one stream: torch's events time the library's kernels
    t0 = time.time()
    chunk_rows = (1 << 30) // d
    buf = torch.empty(chunk_rows * d, dtype=torch.uint8, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    for first in range(0, n, chunk_rows):
        m = min(chunk_rows, n - first)
        buf.random_(0, 256, generator=gen)
        torch.cuda.synchronize(dev)
        g.upload_base_dev(n, d, first, m, buf)
    del buf
    log("[rerank_bench] %d x %d base store on the device: %.1fs, %.1f GB held" % (n, d, time.time() - t0,
                                                                                g.memory_bytes() / 1e9))
    q = torch.from_numpy(c.queries(nq, 4321)).to(dev)
    out = {"workload": args.workload, "nq": nq, "k": k, "base_rows": n, "d": d}

    def search_ms(kk):
        dd = torch.empty((nq, kk), dtype=torch.float32, device=dev)
        ll = torch.empty((nq, kk), dtype=torch.int64, device=dev)
        for _ in range(2):
            g.search_dev(nq, kk, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record(stream)
        for _ in range(args.reps):
            g.search_dev(nq, kk, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        e[1].record(stream)
        g.sync()
        return e[0].elapsed_time(e[1]) / args.reps, dd, ll

    out["search_k1_ms"], _, _ = search_ms(1)
    out["search_k10_ms"], _, _ = search_ms(10)
    rows = []
    for kc in [int(x) for x in args.kcs.split(",")]:
        s_ms, _, cl = search_ms(kc)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        ol = torch.empty((nq, k), dtype=torch.int64, device=dev)
        for _ in range(2):
            g.rerank_dev(nq, kc, q, cl, k, od, ol)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record(stream)
        for _ in range(args.reps):
            g.rerank_dev(nq, kc, q, cl, k, od, ol)
        e[1].record(stream)
        g.sync()
        r_ms = e[0].elapsed_time(e[1]) / args.reps
        valid = int((cl >= 0).sum().item())
        r = {"kc": kc, "search_kc_ms": round(s_ms, 4), "rerank_dev_ms": round(r_ms, 4), "valid_candidates": valid,
             "rows_per_s": valid / (r_ms * 1e-3), "row_TBps": valid * d / (r_ms * 1e-3) / 1e12,
             "step_ms": round(s_ms + r_ms, 4), "step_vs_search_k1": round((s_ms + r_ms) / out["search_k1_ms"], 3),
             "step_vs_search_k10": round((s_ms + r_ms) / out["search_k10_ms"], 3),
             "rerank_share_of_k1_step": round(r_ms / out["search_k1_ms"], 4)}
        rows.append(r)
        print(json.dumps(r), flush=True)
    out["rows"] = rows
    g.close()
    return out


def recall(pkg):
    import rerank_ref
    c = rerank_ref.uint8_recall_corpus(pkg, seed=77)
    g = pkg.GpuIndex(0)
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"])
    g.upload_quantizer(c["counts"], c["links"], c["centroids"], 0)
    g.upload_base(c["base"])
    q, gt = c["queries"], c["gt"][:, 0]
    res = []
    for nprobe, max_codes, ef in ((16, 10000, 64), (32, 20000, 80)):
        _, la = g.search(q, 10, nprobe, max_codes, efSearch=ef)
        r = {"nprobe": nprobe, "max_codes": max_codes, "efSearch": ef,
             "adc": {"R@1": float((la[:, 0] == gt).mean()), "R@10": float((la == gt[:, None]).any(1).mean())}}
        for kc in (10, 100, 1000):
            _, lr = g.search_rerank(q, 10, kc, nprobe, max_codes, efSearch=ef)
            r["rerank_kc%d" % kc] = {"R@1": float((lr[:, 0] == gt).mean()), "R@10": float((lr == gt[:, None]).any(1).mean())}
        res.append(r)
        print(json.dumps(r), flush=True)
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synthetic-1B-pq16-nc993127-nprobe32")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kcs", default="10,20,100,1000")
    ap.add_argument("--no-recall", action="store_true")
    ap.add_argument("--no-speed", action="store_true")
    ap.add_argument("--out", default=None, help="write the whole result as JSON here")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    result = {}
    if not args.no_recall:
        result["recall"] = recall(pkg)
    if not args.no_speed:
        result["speed"] = speed(args, pkg, torch)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
