#!/usr/bin/env python3
"""Learn IVF coarse centroids from a .bvecs / .fvecs learn file on the device and write them as a .fvecs file: the file
the reference's drivers take as -path_centroids and hand to IndexIVF_HNSW::build_quantizer (IndexIVF_HNSW.cpp:34-66).

The learn file is memory-mapped: only the rows of the training sample are read (at most nc * 256 of the first n-train
rows, faiss's rule; learn_centroids in the package).  Exact Lloyd iterations, ivfhnsw_gpu_kmeans.

usage: python tools/learn_centroids.py --learn learn.bvecs --nc 993127 [--n-train N] [--niter 10] [--seed 1234]
                                       --out centroids.fvecs
Prints one JSON line: rows used, objective per iteration, seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--learn", required=True, help=".bvecs or .fvecs learn file")
    ap.add_argument("--nc", type=int, required=True, help="number of centroids")
    ap.add_argument("--n-train", type=int, default=0, help="use the first N rows of the file (default: all)")
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--max-points-per-centroid", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", required=True, help="output .fvecs file")
    a = ap.parse_args(argv)
    if not a.learn.endswith((".bvecs", ".fvecs")):
        ap.error("--learn must be a .bvecs or .fvecs file")

    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    t0 = time.time()
    mm = pkg.open_xvecs(a.learn)
    n = len(mm) if a.n_train <= 0 else min(a.n_train, len(mm))
    d = mm.dtype["v"].shape[0]
    for r in {0, n - 1}:  # the size check covers the rest of the records' layout
        if int(mm["dim"][r]) != d:
            raise SystemExit("%s: record %d has dimension %d, expected %d" % (a.learn, r, int(mm["dim"][r]), d))
    cents, obj = pkg.learn_centroids(mm["v"][:n], a.nc, niter=a.niter, seed=a.seed,
                                     max_points_per_centroid=a.max_points_per_centroid, device=a.device)
    pkg.write_fvecs(a.out, cents)
    print(json.dumps(dict(learn=os.path.basename(a.learn), n_file=len(mm), n_used=min(n, a.nc * a.max_points_per_centroid),
                          d=d, nc=a.nc, niter=a.niter, seed=a.seed, obj=[float(v) for v in obj],
                          seconds=round(time.time() - t0, 3), out=a.out)))


if __name__ == "__main__":
    main()
