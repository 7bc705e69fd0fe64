#!/usr/bin/env python3
"""Lloyd k-means of the coarse centroids on one MI355X (ivfhnsw_gpu_kmeans_dev).

SIFT-like rows: uint8-valued floats around 65 536 clustered centres, generated on the device; seeds = nc distinct rows.
For every (d, nc): `--iters` single iterations in sequence (an iteration depends only on the centroids it starts from,
so niter = 1 calls fed back are the niter = K run), each timed by HIP events on the handle's stream (torch's); the
assignment alone (ivfhnsw_gpu_knn_dev, k = 1, the same shapes) once, timed the same way; update + split = iteration -
assignment.  Empty clusters per iteration = clusters the iteration's assignment left empty (the splits it made).
usage: python tools/kmeans_bench.py [--n 10000000] [--ncs 65536,262144,993127] [--ds 128,96] [--iters 2]
Prints one JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--ncs", default="65536,262144,993127")
    ap.add_argument("--ds", default="128,96")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    g = pkg.GpuIndex(0)
    g.set_stream(stream.cuda_stream)  # one stream: torch's events time the library's kernels
    n = a.n
    for d in [int(v) for v in a.ds.split(",")]:
        gen = torch.Generator(device=dev)
        gen.manual_seed(a.seed + d)
        centres = torch.randint(0, 160, (65536, d), generator=gen, device=dev, dtype=torch.int32).float()
        x = torch.empty((n, d), dtype=torch.float32, device=dev)
        for i0 in range(0, n, 1 << 20):
            i1 = min(n, i0 + (1 << 20))
            comp = torch.randint(0, 65536, (i1 - i0,), generator=gen, device=dev)
            noise = torch.randn((i1 - i0, d), generator=gen, device=dev) * 12
            x[i0:i1] = (centres[comp] + noise).round().clamp(0, 255)
        del centres
        for nc in [int(v) for v in a.ncs.split(",")]:
            pick = torch.randperm(n, generator=gen, device=dev)[:nc]
            c = x[pick].contiguous()
            assign = torch.empty(n, dtype=torch.int32, device=dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            iters = []
            for it in range(a.iters):
                ev[0].record(stream)
                obj = g.kmeans_dev(n, d, nc, x, 1, c, assign)
                ev[1].record(stream)
                ev[1].synchronize()
                ms = ev[0].elapsed_time(ev[1])
                empty = int((torch.bincount(assign.long(), minlength=nc) == 0).sum().item())
                iters.append(dict(ms=round(ms, 2), obj=float(obj[0]), empty=empty))
                log("[kmeans] d %d nc %d iteration %d: %.1f ms, %d empty clusters split" % (d, nc, it, ms, empty))
            ids = torch.empty(n, dtype=torch.int32, device=dev)
            ev[0].record(stream)
            g.knn_dev(n, nc, d, x, c, 1, ids)
            ev[1].record(stream)
            ev[1].synchronize()
            knn_ms = ev[0].elapsed_time(ev[1])
            it_ms = float(np.median([r["ms"] for r in iters]))
            upd_ms = it_ms - knn_ms
            print(json.dumps(dict(
                n=n, d=d, nc=nc, iters=iters, s_per_iter=round(it_ms / 1e3, 3), assign_ms=round(knn_ms, 2),
                assign_tflops=round(2.0 * n * nc * d / (knn_ms * 1e-3) / 1e12, 1),
                update_split_ms=round(upd_ms, 2), update_split_share=round(upd_ms / it_ms, 4))), flush=True)
            del c, assign, ids, pick
        del x
        torch.cuda.empty_cache()
    g.close()


if __name__ == "__main__":
    t0 = time.time()
    main()
    log("[kmeans] total %.1f s" % (time.time() - t0))
