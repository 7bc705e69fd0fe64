"""Times ivfhnsw_gpu_build_graph at the reference's 993 127 centroids (iid and clustered tables): the host-pointer form,
the _dev form on device-resident vectors, and ivfhnsw_gpu_knn_dev alone with the same (n, d, ncand) -- the sweep; the
remainder is phases A-C (kernels_graph.hip and the sort between them).  With --walk also what the walk finds on the
result, against a plain k-NN graph.  usage: python tools/graph_bench.py [n] [--reps R] [--walk]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge
import synth

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=993127)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--walk", action="store_true")
args = ap.parse_args()

import torch

pkg = ge.load_pkg()
n, d, M, maxM, ncand = args.n, 128, 16, 32, 64
dev = torch.device("cuda", 0)
for kind in ("iid", "clustered"):
    rng = np.random.default_rng(1)
    x = synth.sift_like(rng, n, d) if kind == "iid" else synth.clustered_centroids(rng, n, d)
    g = pkg.GpuIndex(0)
    host = []
    for _ in range(args.reps):  # (the first call also allocates the workspace)
        t0 = time.time()
        counts, links = g.build_graph(x, M, maxM, ncand)
        host.append(time.time() - t0)
    tx = torch.from_numpy(x).to(dev)
    tc = torch.empty(n, dtype=torch.uint8, device=dev)
    tl = torch.empty((n, maxM), dtype=torch.int32, device=dev)
    ti = torch.empty((n, ncand), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    total, sweep = [], []
    for _ in range(args.reps):
        t0 = time.time()
        g.build_graph_dev(n, d, tx, M, maxM, ncand, tc, tl)
        g.sync()
        total.append(time.time() - t0)
        t0 = time.time()
        g.knn_dev(n, n, d, tx, tx, ncand, ti, mode=g.KNN_EARLIER)
        g.sync()
        sweep.append(time.time() - t0)
    assert np.array_equal(tc.cpu().numpy(), counts) and np.array_equal(tl.cpu().numpy().view(np.uint32), links)
    print("%s n=%d: build_graph (host pointers) %s s; build_graph_dev %.2f s = sweep %.2f s + phases A-C %.2f s (best of "
          "%d); longest reverse list %d; mean degree %.1f, max %d"
          % (kind, n, " / ".join("%.2f" % t for t in host), min(total), min(sweep), min(total) - min(sweep), args.reps,
             g.last_graph_longest_reverse(), counts.mean(), counts.max()), flush=True)
    if args.walk:
        q = (x[rng.integers(0, n, 10000)] + rng.normal(0, 8.0, (10000, d))).astype(np.float32)
        gt, _ = g.knn(x, 1, q)
        g.upload_quantizer(counts, links, x, 0)
        ids, _ = g.coarse(q, 1, 80)
        t2 = time.time()
        kc, kl = synth.knn_graph(x, M, maxM)
        t3 = time.time()
        g2 = pkg.GpuIndex(0)
        g2.upload_quantizer(kc, kl, x, 0)
        ids2, _ = g2.coarse(q, 1, 80)
        print("%s n=%d: walk ef 80 finds the true nearest for %.4f; plain k-NN graph: %.1f s, degree %.1f, walk %.4f"
              % (kind, n, (ids[:, 0] == gt[:, 0]).mean(), t3 - t2, kc.mean(), (ids2[:, 0] == gt[:, 0]).mean()), flush=True)
        g2.close()
    g.close()
