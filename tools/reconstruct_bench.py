#!/usr/bin/env python3
"""Reconstruction of stored vectors on the device (ivfhnsw_gpu_reconstruct*) at the metric's shapes.

Per workload (bench.py's synthetic 1B corpus and the 100M one, lists generated on the device, ids = the running index):
  (a) reconstruct_rows_dev of 2^20 contiguous rows and of 2^20 uniformly random rows, ROTATED space on the plain index
      and ORIGINAL space on a second upload of the same lists with an OPQ matrix: rows/s and bytes/s.  Bytes counted per
      row: 4 d written, 4 d of anchor read (one centroid row; 8 d with Grouping), M code bytes and the 8-byte row index;
      with OPQ the staged chunk is written and read once more (8 d).  Beside them the guide's HBM figures for these
      shapes: 6.29 TB/s streaming copy, 5.5-5.8 TB/s for random whole rows.
  (b) locate_dev of 10^4 and 10^6 labels against remove_ids_dev of labels that match nothing on the same handle (the same
      read of ids against a bitmap): milliseconds and the ratio.
  (c) search_reconstruct_dev against search_dev at the workload's parameters, 10 k queries, k = 1 and 10: the added
      milliseconds per step.
Medians over alternating repeats behind a warm-up.  One JSON line per workload on stdout.
usage: python tools/reconstruct_bench.py [--workloads A,B] [--rows N] [--reps R]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_TBS, GATHER_TBS = 6.29, 5.6


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def alternate(fns, sync, reps, warm=3):
    """Median milliseconds of every fn, the fns taking turns; each call ends in a synchronise."""
    for _ in range(warm):
        for f in fns:
            f()
    sync()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            t = time.perf_counter()
            f()
            sync()
            ms[i].append((time.perf_counter() - t) * 1e3)
    return [statistics.median(m) for m in ms]


def run(pkg, synth, bench, torch, name, n_rows, reps):
    dev = torch.device("cuda", 0)
    c = bench.Corpus(pkg, synth, name, 1234, dev, 0)
    g = c.g
    d, M, n_total = c.d, c.M, c.n_total
    out = {"workload": name, "nc": c.nc, "d": d, "code_size": M, "codes": n_total, "rows": n_rows}
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    start = int(torch.randint(0, n_total - n_rows, (1,), generator=gen, device=dev).item())
    contig = torch.arange(start, start + n_rows, dtype=torch.int64, device=dev)
    rand = torch.randint(0, n_total, (n_rows,), generator=gen, device=dev, dtype=torch.int64)
    buf = torch.empty((n_rows, d), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    # (a) reconstruction rate, without and with OPQ
    def rate(h, space, opq):
        per_row = 4 * d + 4 * d + M + 8 + (8 * d if opq else 0)
        ms = alternate([lambda: h.reconstruct_rows_dev(n_rows, contig, buf, space),
                        lambda: h.reconstruct_rows_dev(n_rows, rand, buf, space)], h.sync, reps)
        res = {}
        for key, t, peak in (("contiguous", ms[0], COPY_TBS), ("random", ms[1], GATHER_TBS)):
            res[key] = {"ms": t, "Mrows_per_s": n_rows / t / 1e3, "bytes_per_row": per_row, "TBps": n_rows * per_row / t / 1e9,
                        "guide_TBps": peak, "of_guide": n_rows * per_row / t / 1e9 / peak}
            log("[reconstruct_bench] %s %s rows, %s: %.3f ms, %.1f M rows/s, %.2f TB/s (guide %.2f)"
                % (name, key, "OPQ/ORIGINAL" if opq else "ROTATED", t, res[key]["Mrows_per_s"], res[key]["TBps"], peak))
        return res

    out["rows_rotated"] = rate(g, pkg.RECON_ROTATED, False)

    # (b) locate against the mark pass of a removal that matches nothing (ids are 0 .. n_total - 1)
    loc = {}
    for n in (10 ** 4, 10 ** 6):
        labels = torch.randint(0, n_total, (n,), generator=gen, device=dev, dtype=torch.int64).to(torch.int32)
        # absent labels just above the ids, so that both calls size (and clear) about the same label bitmap
        absent = (torch.randint(0, n_total // 8, (n,), generator=gen, device=dev, dtype=torch.int64) + n_total).to(torch.int32)
        rows = torch.empty(n, dtype=torch.int64, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        removed = []
        ms = alternate([lambda: g.locate_dev(n, labels, rows, cnt), lambda: removed.append(g.remove_ids_dev(n, absent))],
                       lambda: None, reps)   # both calls return with the stream drained
        assert not any(removed), "the removal was to match nothing"
        assert int((rows < 0).sum().item()) == 0 and bool((rows == labels.to(torch.int64)).all().item())
        loc[str(n)] = {"locate_ms": ms[0], "remove_nothing_ms": ms[1], "ratio": ms[0] / ms[1],
                       "ids_TBps": 4 * n_total / ms[0] / 1e9}
        log("[reconstruct_bench] %s locate %d labels: %.2f ms; remove_ids of %d absent labels: %.2f ms; ratio %.2f"
            % (name, n, ms[0], n, ms[1], ms[0] / ms[1]))
        del labels, absent, rows, cnt
    out["locate"] = loc

    # (c) search and reconstruct against search
    nq = 10000
    q = torch.from_numpy(c.queries(nq, 4321)).to(dev)
    sr = {}
    for k in (1, 10):
        dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
        ll = torch.empty((nq, k), dtype=torch.int64, device=dev)
        rr = torch.empty((nq, k), dtype=torch.int64, device=dev)
        rec = torch.empty((nq, k, d), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        ms = alternate([lambda: g.search_dev(nq, k, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef),
                        lambda: g.search_reconstruct_dev(nq, k, q, dd, ll, rec, c.nprobe, c.max_codes, d_rows=rr, efSearch=c.ef)],
                       g.sync, reps)
        sr[str(k)] = {"search_ms": ms[0], "search_reconstruct_ms": ms[1], "added_ms": ms[1] - ms[0]}
        log("[reconstruct_bench] %s k = %d, %d queries: search %.3f ms, search + reconstruct %.3f ms" % (name, k, nq, ms[0], ms[1]))
        del dd, ll, rr, rec
    out["search_reconstruct"] = sr

    # (a) again on an upload of the same lists with an OPQ matrix: ORIGINAL space goes through the staged rotation
    g.close()
    c.opq_A = synth.random_rotation(np.random.default_rng(5), d)
    h = c.upload(0, 1)
    out["rows_original_opq"] = rate(h, pkg.RECON_ORIGINAL, True)
    out["memory_GB"] = h.memory_bytes() / 1e9
    h.close()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="synthetic-100M-pq16-nc131072-nprobe32,synthetic-1B-pq16-nc993127-nprobe32")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    import bench
    import synth
    pkg = ge.load_pkg()
    for name in args.workloads.split(","):
        print(json.dumps(run(pkg, synth, bench, torch, name, args.rows, args.reps)), flush=True)


if __name__ == "__main__":
    main()
