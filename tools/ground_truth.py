#!/usr/bin/env python3
"""Ground truth for a uint8 base: the file the drivers read as -path_gt (tests/test_ivfhnsw_sift1b.cpp:28-32,173-215).

Streams a .bvecs base into the device's base store (upload_base_bvecs), runs the exact brute-force search
(ivfhnsw_gpu_exact_search, kernels_exact.hip) for every query of a .bvecs query file and writes the labels as .ivecs:
per query one int32 k followed by k labels, nearest first, ties to the lower label.  Labels are the reference's idx_t
(uint32): a label >= 2^31 is stored as its 32-bit pattern; a slot beyond the base's rows (k > rows) holds 0xffffffff.

With --radius R the exact RANGE search runs instead (ivfhnsw_gpu_exact_range_search): --out is then an .npz holding lims
(uint64 [nq + 1]), labels (int64) and distances (float32) -- query q owns entries [lims[q], lims[q + 1]), every base row
with distance < R in ascending label -- and radius; --k is ignored.  read_range reads it back.

With --allow FILE or --deny FILE (one of them; an .ivecs or .npy file of labels = row numbers of the base) the truth of a
FILTERED workload is written: the base filter (ivfhnsw_gpu_set_base_filter) is installed before either
search, so only rows in the allow set (not in the deny set) are returned.  The .npz of the range form then also holds
filter_mode (0 allow, 1 deny; -1 without a filter) and rows_passing; read_range_filter reads them.

With --tags FILE --query-tags FILE (both .npy files of uint16: one tag per row of the base, one per query; 0xffff = no tag)
the truth of a TAGGED workload is written: the base tags (ivfhnsw_gpu_set_base_tags) are installed and the
_tags form of either search runs, so query q gets only rows whose tag is query_tags[q] (every row when it is 0xffff).

With --values FILE --query-ranges FILE (both .npy files of uint32: one value per row of the base, 0xffffffff = no value;
one pair (lo, hi) per query, shape [nq, 2]) the truth of a workload with a value interval per query is written: the base
values (ivfhnsw_gpu_set_base_values) are installed and the _values form of either search runs, so query q
gets only rows whose value lies in [lo, hi], inclusive ((0, 0xffffffff): every row).

usage: python tools/ground_truth.py --base x.bvecs --queries q.bvecs --k 100 --out gt.ivecs [--rows N] [--allow F | --deny F]
       python tools/ground_truth.py --base x.bvecs --queries q.bvecs --radius R --out gt.npz [--rows N] [--allow F | --deny F]
       python tools/ground_truth.py --base x.bvecs --queries q.bvecs --k 100 --out gt.ivecs --tags t.npy --query-tags qt.npy
       python tools/ground_truth.py --base x.bvecs --queries q.bvecs --k 100 --out gt.ivecs --values v.npy --query-ranges qr.npy"""
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


def write_range(path, lims, distances, labels, radius, filter_mode=-1, rows_passing=None):
    """The result of an exact range search as an .npz (written to exactly `path`); under a base filter its mode (0 allow,
    1 deny) and the rows of the base that pass."""
    extra = {} if rows_passing is None else {"rows_passing": np.uint64(rows_passing)}
    with open(path, "wb") as f:
        np.savez(f, lims=np.asarray(lims, np.uint64), labels=np.asarray(labels, np.int64),
                 distances=np.asarray(distances, np.float32), radius=np.float32(radius), filter_mode=np.int32(filter_mode),
                 **extra)


def read_range_filter(path):
    """(filter_mode, rows_passing) of a file --radius wrote: (-1, None) when it was written without a base filter."""
    with np.load(path) as z:
        mode = int(z["filter_mode"]) if "filter_mode" in z else -1
        return mode, (int(z["rows_passing"]) if "rows_passing" in z else None)


def read_labels(path):
    """The labels of an --allow / --deny file as uint32 [n]: every value of an .ivecs file (records of any length), or
    the integers of an .npy array of any shape."""
    if path.endswith(".npy"):
        lab = np.load(path)
        if lab.dtype.kind not in "iu":
            raise ValueError("%s: labels must be integers, not %s" % (path, lab.dtype))
        lab = lab.ravel().astype(np.int64)
    else:
        lab = read_ivecs(path).ravel()
    if lab.size and (lab.min() < 0 or lab.max() >= 1 << 32):
        raise ValueError("%s: labels must fit 32 bits unsigned" % path)
    return lab.astype(np.uint32)


def read_tags(path):
    """The tags of a --tags / --query-tags file as uint16 [n]: an .npy array of integers in 0..0xffff, of any shape."""
    t = np.load(path)
    if t.dtype.kind not in "iu":
        raise ValueError("%s: tags must be integers, not %s" % (path, t.dtype))
    t = t.ravel().astype(np.int64)
    if t.size and (t.min() < 0 or t.max() > 0xffff):
        raise ValueError("%s: tags must fit 16 bits unsigned" % path)
    return t.astype(np.uint16)


def read_values(path):
    """The values of a --values / --query-ranges file as uint32, flat: an .npy array of integers in 0..0xffffffff."""
    v = np.load(path)
    if v.dtype.kind not in "iu":
        raise ValueError("%s: values must be integers, not %s" % (path, v.dtype))
    v = v.ravel()
    if v.size and (int(v.min()) < 0 or int(v.max()) > 0xffffffff):
        raise ValueError("%s: values must fit 32 bits unsigned" % path)
    return v.astype(np.uint32)


def install_values(g, n, nq, values, query_ranges):
    """The base values of a workload on g's store of n rows, the two arrays checked against the store and the queries."""
    if values.size != n or query_ranges.size != 2 * nq:
        raise ValueError("%d values for %d rows, %d interval ends for %d queries" % (values.size, n, query_ranges.size, nq))
    g.set_base_values(np.arange(n, dtype=np.uint32), values)


def install_tags(g, n, nq, tags, query_tags):
    """The base tags of a tagged workload on g's store of n rows, the two arrays checked against the store and the queries."""
    if tags.size != n or query_tags.size != nq:
        raise ValueError("%d tags for %d rows, %d query tags for %d queries" % (tags.size, n, query_tags.size, nq))
    g.set_base_tags(np.arange(n, dtype=np.uint32), tags)


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


def ground_truth(pkg, base_path, query_path, k, rows=None, device=0, chunk_rows=1 << 20, labels=None, deny=False, tags=None,
                 query_tags=None, values=None, query_ranges=None):
    """labels int64 [nq, k] (-1 beyond the base's rows) of the exact k nearest base rows of every query; with `labels`
    only of the rows whose number is in them (deny: is not); with `tags` and `query_tags` only of the rows that carry the
    query's tag; with `values` and `query_ranges` only of the rows whose value lies in the query's interval."""
    img, dq = read_bvecs_image(query_path)
    g = pkg.GpuIndex(device)
    try:
        n, d = g.upload_base_bvecs(base_path, chunk_rows=chunk_rows, rows=rows)
        if d != dq:
            raise ValueError("base dimension %d, query dimension %d" % (d, dq))
        if labels is not None:
            g.set_base_filter(labels, deny=deny)
        if tags is not None:
            install_tags(g, n, img.shape[0], tags, query_tags)
            _, lab = g.exact_search_tags(img[:, 4:], k, query_tags)
        elif values is not None:
            install_values(g, n, img.shape[0], values, query_ranges)
            _, lab = g.exact_search_values(img[:, 4:], k, query_ranges)
        else:
            _, lab = g.exact_search(img[:, 4:], k)
    finally:
        g.close()
    return lab


def ground_truth_range(pkg, base_path, query_path, radius, rows=None, device=0, chunk_rows=1 << 20, labels=None, deny=False,
                       info=None, tags=None, query_tags=None, values=None, query_ranges=None):
    """(lims, distances, labels) of every base row within the radius of every query, ascending label per query; with
    `labels` only of the rows whose number is in them (deny: is not), info (a dict) then receives rows_passing."""
    img, dq = read_bvecs_image(query_path)
    g = pkg.GpuIndex(device)
    try:
        n, d = g.upload_base_bvecs(base_path, chunk_rows=chunk_rows, rows=rows)
        if d != dq:
            raise ValueError("base dimension %d, query dimension %d" % (d, dq))
        if labels is not None:
            g.set_base_filter(labels, deny=deny)
            if info is not None:
                info["rows_passing"] = g.base_filter_info()[1]
        if tags is not None:
            install_tags(g, n, img.shape[0], tags, query_tags)
            if info is not None:
                info["rows_passing"] = g.base_tags_info()[0]  # the tagged rows
            return g.exact_range_search_tags(img[:, 4:], radius, query_tags)
        if values is not None:
            install_values(g, n, img.shape[0], values, query_ranges)
            if info is not None:
                info["rows_passing"] = g.base_values_info()[0]  # the rows that hold a value
            return g.exact_range_search_values(img[:, 4:], radius, query_ranges)
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
    flt = ap.add_mutually_exclusive_group()
    flt.add_argument("--allow", default=None, help="an .ivecs or .npy file of labels: only these rows of the base are returned")
    flt.add_argument("--deny", default=None, help="an .ivecs or .npy file of labels: these rows of the base are never returned")
    ap.add_argument("--tags", default=None, help="an .npy file of uint16: the tag of every row of the base (0xffff: none)")
    ap.add_argument("--query-tags", default=None, help="an .npy file of uint16: the tag of every query (0xffff: every row)")
    ap.add_argument("--values", default=None, help="an .npy file of uint32: the value of every row of the base (0xffffffff: none)")
    ap.add_argument("--query-ranges", default=None, help="an .npy file of uint32 [nq, 2]: the interval (lo, hi) of every query, "
                                                         "inclusive ((0, 0xffffffff): every row)")
    args = ap.parse_args(argv)
    if (args.values is None) != (args.query_ranges is None) or (args.values and (args.allow or args.deny or args.tags)):
        ap.error("--values and --query-ranges go together, and not with --allow / --deny / --tags")
    values = read_values(args.values) if args.values else None
    query_ranges = read_values(args.query_ranges) if args.values else None
    if (args.tags is None) != (args.query_tags is None) or (args.tags and (args.allow or args.deny)):
        ap.error("--tags and --query-tags go together, and not with --allow / --deny")
    tags = read_tags(args.tags) if args.tags else None
    query_tags = read_tags(args.query_tags) if args.tags else None
    labels = read_labels(args.allow or args.deny) if (args.allow or args.deny) else None
    deny = args.deny is not None
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    if args.radius is not None:
        info = {}
        lims, dist, lab = ground_truth_range(pkg, args.base, args.queries, args.radius, rows=args.rows, device=args.device,
                                             labels=labels, deny=deny, info=info, tags=tags, query_tags=query_tags,
                                             values=values, query_ranges=query_ranges)
        write_range(args.out, lims, dist, lab, args.radius, filter_mode=-1 if labels is None else int(deny),
                    rows_passing=info.get("rows_passing"))
        print("%s: %d queries, %d rows within %g" % (args.out, lims.size - 1, lab.size, args.radius))
        return
    lab = ground_truth(pkg, args.base, args.queries, args.k, rows=args.rows, device=args.device, labels=labels, deny=deny,
                       tags=tags, query_tags=query_tags, values=values, query_ranges=query_ranges)
    write_ivecs(args.out, lab)
    print("%s: %d queries x %d labels" % (args.out, lab.shape[0], lab.shape[1]))


if __name__ == "__main__":
    main()
