#!/usr/bin/env python3
"""Ground truth for a uint8 base: the file the drivers read as -path_gt (tests/test_ivfhnsw_sift1b.cpp:28-32,173-215).

Streams a .bvecs base into the device's base store (upload_base_bvecs), runs the exact brute-force search
(ivfhnsw_gpu_exact_search, kernels_exact.hip) for every query of a .bvecs query file and writes the labels as .ivecs:
per query one int32 k followed by k labels, nearest first, ties to the lower label.  Labels are the reference's idx_t
(uint32): a label >= 2^31 is stored as its 32-bit pattern; a slot beyond the base's rows (k > rows) holds 0xffffffff.

With --radius R the exact RANGE search runs instead (ivfhnsw_gpu_exact_range_search): --out is then an .npz holding lims
(uint64 [nq + 1]), labels (int64) and distances (float32) -- query q owns entries [lims[q], lims[q + 1]), every base row
with distance < R in ascending label -- and radius; --k is ignored.  read_range reads it back.

usage: python tools/ground_truth.py --base x.bvecs --queries q.bvecs --k 100 --out gt.ivecs [--rows N]
       python tools/ground_truth.py --base x.bvecs --queries q.bvecs --radius R --out gt.npz [--rows N]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))


def write_ivecs(path, labels):
    """labels [nq, k] (any integer type; -1 or values up to 2^32 - 1) as .ivecs records of an int32 k and k 32-bit labels."""
    lab = np.asarray(labels)
    assert lab.ndim == 2 and lab.shape[1] >= 1, "labels: [nq, k]"
    lab = lab.astype(np.int64)
    assert ((lab >= -1) & (lab < 1 << 32)).all(), "labels must fit the reference's uint32 idx_t"
    nq, k = lab.shape
    rec = np.empty((nq, k + 1), np.uint32)
    rec[:, 0] = k
    rec[:, 1:] = (lab & 0xffffffff).astype(np.uint32)
    rec.astype("<u4").tofile(path)


def read_ivecs(path):
    """The labels of an .ivecs file as int64 [nq, k], every 32-bit value read unsigned (the reference's idx_t); every
    record's k header is checked."""
    raw = np.fromfile(path, "<u4")
    if raw.size == 0:
        raise ValueError("%s is empty" % path)
    k = int(raw[0])
    if k < 1 or raw.size % (k + 1):
        raise ValueError("%s: not an .ivecs file of %d entries per record" % (path, k))
    rec = raw.reshape(-1, k + 1)
    if (rec[:, 0] != k).any():
        bad = int(np.nonzero(rec[:, 0] != k)[0][0])
        raise ValueError("%s: record %d has %d entries, expected %d" % (path, bad, rec[bad, 0], k))
    return rec[:, 1:].astype(np.int64)


def write_range(path, lims, distances, labels, radius):
    """The result of an exact range search as an .npz (written to exactly `path`)."""
    with open(path, "wb") as f:
        np.savez(f, lims=np.asarray(lims, np.uint64), labels=np.asarray(labels, np.int64),
                 distances=np.asarray(distances, np.float32), radius=np.float32(radius))


def read_range(path):
    """(lims uint64 [nq + 1], distances float32 [total], labels int64 [total], radius) of a file --radius wrote; lims is
    checked against the arrays."""
    with np.load(path) as z:
        lims, dist, lab, radius = z["lims"], z["distances"], z["labels"], float(z["radius"])
    if lims.dtype != np.uint64 or dist.dtype != np.float32 or lab.dtype != np.int64:
        raise ValueError("%s: lims / distances / labels are not uint64 / float32 / int64" % path)
    if lims.ndim != 1 or lims.size < 1 or lims[0] != 0 or (np.diff(lims.astype(np.int64)) < 0).any() or \
            dist.shape != (int(lims[-1]),) or lab.shape != dist.shape:
        raise ValueError("%s: lims does not describe the %d distances and %d labels" % (path, dist.size, lab.size))
    return lims, dist, lab, radius


def read_bvecs_image(path):
    """(image uint8 [n, d + 4], d) of a .bvecs file, every record's dim header checked; image[:, 4:] are the rows, d + 4
    bytes apart, as exact_search and upload_base take them."""
    raw = np.fromfile(path, np.uint8)
    if raw.size < 4:
        raise ValueError("%s is empty" % path)
    d = int(raw[:4].view("<i4")[0])
    if d <= 0 or raw.size % (d + 4):
        raise ValueError("%s: not a .bvecs file of dimension %d" % (path, d))
    img = raw.reshape(-1, d + 4)
    dims = np.ascontiguousarray(img[:, :4]).view("<i4")[:, 0]
    if (dims != d).any():
        bad = int(np.nonzero(dims != d)[0][0])
        raise ValueError("%s: record %d has dimension %d, expected %d" % (path, bad, dims[bad], d))
    return img, d


def ground_truth(pkg, base_path, query_path, k, rows=None, device=0, chunk_rows=1 << 20):
    """labels int64 [nq, k] (-1 beyond the base's rows) of the exact k nearest base rows of every query."""
    img, dq = read_bvecs_image(query_path)
    g = pkg.GpuIndex(device)
    try:
        n, d = g.upload_base_bvecs(base_path, chunk_rows=chunk_rows, rows=rows)
        if d != dq:
            raise ValueError("base dimension %d, query dimension %d" % (d, dq))
        _, lab = g.exact_search(img[:, 4:], k)
    finally:
        g.close()
    return lab


def ground_truth_range(pkg, base_path, query_path, radius, rows=None, device=0, chunk_rows=1 << 20):
    """(lims, distances, labels) of every base row within the radius of every query, ascending label per query."""
    img, dq = read_bvecs_image(query_path)
    g = pkg.GpuIndex(device)
    try:
        n, d = g.upload_base_bvecs(base_path, chunk_rows=chunk_rows, rows=rows)
        if d != dq:
            raise ValueError("base dimension %d, query dimension %d" % (d, dq))
        return g.exact_range_search(img[:, 4:], radius)
    finally:
        g.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base", required=True)
    ap.add_argument("--queries", required=True)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--radius", type=float, default=None,
                    help="range mode: every row with distance < RADIUS; --out is an .npz, --k is ignored")
    ap.add_argument("--out", required=True)
    ap.add_argument("--rows", type=int, default=None, help="only the base file's first N records")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    if args.radius is not None:
        lims, dist, lab = ground_truth_range(pkg, args.base, args.queries, args.radius, rows=args.rows, device=args.device)
        write_range(args.out, lims, dist, lab, args.radius)
        print("%s: %d queries, %d rows within %g" % (args.out, lims.size - 1, lab.size, args.radius))
        return
    lab = ground_truth(pkg, args.base, args.queries, args.k, rows=args.rows, device=args.device)
    write_ivecs(args.out, lab)
    print("%s: %d queries x %d labels" % (args.out, lab.shape[0], lab.shape[1]))


if __name__ == "__main__":
    main()
