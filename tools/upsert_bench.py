#!/usr/bin/env python3
"""Upserts on a device-resident index (ivfhnsw_gpu_upsert_ivf) at the metric's shape, against the pair of
calls an upsert replaces.

  bench.py's synthetic-1B-pq16-nc993127-nprobe32 corpus (lists generated on the device, 10^9 codes, ids = the running
  index).  One batch of --n codes (10 M) with uniformly random list ids whose labels are half resident (distinct random
  labels below n_total) and half new (n_total and up).  In ONE process, on the same starting state (each side has a
  handle of its own, and the corpus is uploaded to it again before every measurement), --rounds alternating rounds of
    A  upsert_ivf_dev(batch)
    B  remove_ids_dev(labels) followed by append_ivf_dev(batch)        (the yardstick: unchanged code)
  wall milliseconds per measurement (each call returns when the new arrays are in place), medians over the rounds, the
  bytes moved (ids read by the mark, old rows read, new rows written, M + 5 bytes per code) against the 6.29 TB/s copy
  rate of the guide, and the peak of the device memory in use during the measurement (first round only, polled from a
  second thread through hipMemGetInfo: the new arrays live beside the handle's own until they are installed, so the
  handle's ivfhnsw_gpu_memory_bytes, reported before and after the call, does not see the peak; the other side's handle
  is resident too, hence "above the start").  A whole warm-up measurement of each side comes first: the first call
  allocates the workspace the handle keeps.  At a shape the host holds (--workload of at most 2^26 codes) the two sides
  must leave the same ids.
usage: python tools/upsert_bench.py [--workload NAME] [--n 10000000] [--rounds 5]"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_TBS = 6.29


def log(*a):
    print(*a, file=sys.stderr, flush=True)


class PeakMemory:
    """The most device memory in use while the block runs, polled every millisecond."""

    def __init__(self, torch, dev):
        self.torch, self.dev, self.peak, self.stop = torch, dev, 0, False

    def poll(self):
        while not self.stop:
            free, total = self.torch.cuda.mem_get_info(self.dev)
            self.peak = max(self.peak, total - free)
            time.sleep(0.001)

    def __enter__(self):
        self.thread = threading.Thread(target=self.poll)
        self.thread.start()
        return self

    def __exit__(self, *a):
        self.stop = True
        self.thread.join()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synthetic-1B-pq16-nc993127-nprobe32")
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    import bench
    import synth
    pkg = ge.load_pkg()
    dev = torch.device("cuda", 0)
    c = bench.Corpus(pkg, synth, args.workload, 1234, dev, 0)
    c.g.close()
    n, n_total = args.n, c.n_total
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    resident = torch.unique(torch.randint(0, n_total, (n // 2,), device=dev, generator=gen, dtype=torch.int64))
    n_res = resident.numel()
    new = torch.arange(n_total, n_total + (n - n_res), device=dev, dtype=torch.int64)
    lab64 = torch.cat([resident, new])[torch.randperm(n, device=dev, generator=gen)]
    labels = (lab64 & 0xffffffff).to(torch.int32) if n_total + n < 2 ** 31 else \
        torch.where(lab64 >= 2 ** 31, lab64 - 2 ** 32, lab64).to(torch.int32)   # the same bits as uint32
    li = torch.randint(0, c.nc, (n,), dtype=torch.int32, device=dev, generator=gen)
    codes = torch.randint(0, 256, (n, c.M), dtype=torch.uint8, device=dev, generator=gen)
    ncodes = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=gen)
    del resident, new, lab64
    torch.cuda.synchronize(dev)
    row = c.M + 5
    after = n_total - n_res + n

    def side_a(g):
        t = time.perf_counter()
        n_rm = g.upsert_ivf_dev(n, li, labels, codes, ncodes)
        ms = (time.perf_counter() - t) * 1e3
        assert n_rm == n_res, (n_rm, n_res)
        return {"ms": ms}

    def side_b(g):
        t = time.perf_counter()
        n_rm = g.remove_ids_dev(n, labels)
        t1 = time.perf_counter()
        g.append_ivf_dev(n, li, labels, codes, ncodes)
        t2 = time.perf_counter()
        assert n_rm == n_res, (n_rm, n_res)
        return {"ms": (t2 - t) * 1e3, "remove_ms": (t1 - t) * 1e3, "append_ms": (t2 - t1) * 1e3}

    def upload(g):   # the starting state again, on the same handle: its update workspace stays
        tb = c.tb
        g.upload_ivf_synthetic(c.d, c.M, tb["offsets"], c.centroid_norms, tb["pq_centroids"], tb["norm_table"], c.code_seed,
                               opq_A=c.opq_A)
        g.sync()

    def measure(g, side, poll=False):
        upload(g)
        held = g.memory_bytes()
        free, total = torch.cuda.mem_get_info(dev)
        if poll:
            with PeakMemory(torch, dev) as pm:
                r = side(g)
            r.update(device_GB_before=(total - free) / 1e9, peak_device_GB=pm.peak / 1e9)
        else:
            r = side(g)
        r.update(handle_GB_before=held / 1e9, handle_GB_after=g.memory_bytes() / 1e9)
        return r, (g.download_ivf()[1] if args.check else None)

    args.check = n_total <= 2 ** 26   # the ids of both sides compared where the host holds them
    sides = (("upsert", side_a), ("pair", side_b))
    handles = {name: pkg.GpuIndex(0) for name, _ in sides}
    for name, side in sides:   # warm-up: one whole measurement each, which allocates the workspace the handle keeps
        r, _ = measure(handles[name], side)
        log("[upsert_bench] warm-up %s: %s" % (name, json.dumps(r)))
    res = {"upsert": [], "pair": []}
    ids = {}
    for rnd in range(args.rounds):
        for name, side in sides if rnd % 2 == 0 else sides[::-1]:
            r, got = measure(handles[name], side, poll=rnd == 0)
            res[name].append(r)
            ids[name] = got
            log("[upsert_bench] round %d %s: %s" % (rnd, name, json.dumps(r)))
        if args.check:
            assert np.array_equal(ids["upsert"], ids["pair"]), "the two sides leave different ids"
    for g in handles.values():
        g.close()
    # bytes: the mark reads the ids, every old row is read and every new row written -- once (upsert) or twice (the pair:
    # the removal writes n_total - n_res rows, the append reads them and writes `after` rows)
    moved_a = n_total * 4 + n_total * row + after * row
    moved_b = n_total * 4 + n_total * row + 2 * (n_total - n_res) * row + after * row
    out = {"workload": args.workload, "nc": c.nc, "code_size": c.M, "codes": n_total, "batch": n, "resident_labels": n_res,
           "rounds": args.rounds, "same_ids_checked": bool(args.check)}
    for name, moved in (("upsert", moved_a), ("pair", moved_b)):
        ms = float(np.median([r["ms"] for r in res[name]]))
        out[name] = {"median_ms": ms, "all_ms": [r["ms"] for r in res[name]], "GB_moved": moved / 1e9, "TBps": moved / ms / 1e9,
                     "of_copy_rate": moved / ms / 1e9 / COPY_TBS,
                     "peak_device_GB": res[name][0]["peak_device_GB"],
                     "peak_above_start_GB": res[name][0]["peak_device_GB"] - res[name][0]["device_GB_before"],
                     "handle_GB_after": res[name][-1]["handle_GB_after"]}
    out["pair"]["median_remove_ms"] = float(np.median([r["remove_ms"] for r in res["pair"]]))
    out["pair"]["median_append_ms"] = float(np.median([r["append_ms"] for r in res["pair"]]))
    # (a call that allocates 21 GB right after another handle freed as much can wait seconds for the allocator: the pair,
    # with two such allocations, meets that more often, and its stage medians are the steadier figure)
    out["pair"]["sum_of_stage_medians_ms"] = out["pair"]["median_remove_ms"] + out["pair"]["median_append_ms"]
    out["upsert_over_pair"] = out["upsert"]["median_ms"] / out["pair"]["median_ms"]
    out["upsert_over_pair_stage_medians"] = out["upsert"]["median_ms"] / out["pair"]["sum_of_stage_medians_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
