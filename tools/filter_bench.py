#!/usr/bin/env python3
"""The label filter of a handle (ivfhnsw_gpu_set_filter) at the metric's shape.

On bench.py's synthetic-1B-pq16-nc993127-nprobe32 corpus (lists generated on the device, 10^9 codes, ids = the running
index):
  1. set_filter_dev of 1 k, 10 M and 500 M distinct random labels below n_total: wall milliseconds per call (the call
     returns when the mask is installed) and the rows that pass (checked against the number of labels).  The first call
     allocates the bitmap and the mask, and is reported apart.
  2. search_dev queries/s (10 k queries, k = 1) of ONE handle in one run, in this order: unfiltered; deny nothing (every
     row passes: the cost of the filtered kernels alone); allow 50 %; allow 10 %; allow 1 %; unfiltered again.  The
     reference point of every filtered figure is the unfiltered pair of the same run.
With --slots, filter slots (ivfhnsw_gpu_search_slots) instead, on the same corpus and ONE handle:
  3. --reps (>= 5) alternating repetitions of: (a) unfiltered; (b) set_filter allow 10 %; (c) _slots, every query on one slot
     holding that same set; (d) _slots, 32 installed 10 % sets dealt round-robin; (e) _slots, every query NONE.  Per form and
     repetition the step time (wall, 10 steps behind 5 warm-up steps) and the scan stage's time per step (profiling level 2).
     The yardstick of (c) is (b) of the same run: its min-max spread over the repetitions is reported beside the difference.
  4. set_filter_slot_dev of 10 M labels (wall ms), and a 10 M-code append_ivf_dev with no filter, with the single filter
     installed, and with 1, 8 and 32 slots installed (wall ms, each twice; what the append costs beyond the unfiltered one
     is the re-mark).
With --tags, row tags (ivfhnsw_gpu_search_tags), on the same corpus and ONE handle (row r carries tag
r % 1024, so tags and the slots' sets below partition the same rows):
  5. --reps (>= 5) alternating repetitions of: (a) unfiltered; (b) _slots, the rows dealt into 32 slots (row r in slot
     r % 32) and the queries dealt over them; (c) _tags, the same partition as 32 tags (a query of slot s names tag s of
     a second table, r % 32); (d) _tags with 1 024 tags, the queries dealt over them.  Step and scan time as in 3.
  6. the loop (d) replaces: per tag set_filter_dev(rows of the tag) + search_dev of that tag's queries, for a sample of
     --loop-tags tags, wall ms per tag, extrapolated to the 1 024 tags of one batch.
  7. set_tags_dev of 10 M labels (wall ms), and a 10 M-code append_ivf_dev without and with the tag table (wall ms, each
     twice: what the append costs beyond the untagged one is the gather).
With --values, row values (ivfhnsw_gpu_search_values), on the same corpus and ONE handle (row r carries
tag r % 1024 and value r % 1024: value = tag, so both forms pass the same rows):
  8. --reps (>= 5) alternating repetitions of: (a) unfiltered; (b) _tags with 1 024 tags, the queries dealt over them;
     (c) _values with the same 1 024 points (t, t); (d) _values with intervals of 128 consecutive values (pass fraction
     1/8, overlapping from query to query: what tags cannot express); (e) _values, every query (0, 0xffffffff).  Step and
     scan time as in 3.
  9. the loop (d) replaces: per distinct interval set_filter_dev(rows whose value lies in it) + search_dev of that
     interval's queries, for a sample of --loop-tags intervals, wall ms per interval.
 10. set_values_dev of 10 M labels (wall ms), and a 10 M-code append_ivf_dev with and without the value table (wall ms,
     each twice: what the append costs beyond the plain one is the gather).
With --tags-values, tag AND value (ivfhnsw_gpu_search_tags_values), on the same corpus and ONE handle
that holds both tables (row r carries tag r % 1024 and value r % 1024, so (t, (t, t)), (t, FULL) and (NONE, (t, t)) pass the
same rows):
 11. --reps (>= 5) alternating repetitions of: (a) unfiltered; (b) _tags with 1 024 tags; (c) _values with the 1 024
     points (t, t); the new call with (d) (t, (t, t)), (e) (t, FULL), (f) (NONE, (t, t)) -- the same rows as (b) and (c), and
     the answers must compare equal; (h) the new call, every query (NONE, FULL), which must answer as (a).  Then, with the
     columns made independent (tag r % 8, value (r // 8) % 1024): (a), _tags over the 8 tags, _values over intervals of 128
     consecutive values, and (g) the new call over the pairs of both, about 1/8 x 1/8 of the rows.  Step and scan time as
     in 3.
 12. the loop (g) replaces: per distinct pair set_filter_dev(rows tagged t whose value lies in the interval) + search_dev of
     that pair's queries, for a sample of --loop-tags pairs, wall ms per pair, extrapolated to all pairs of the batch.
usage: python tools/filter_bench.py [--workload NAME] [--sizes 1000,10000000,500000000] [--fractions 0.5,0.1,0.01]
       python tools/filter_bench.py --slots [--reps 5] [--append 10000000]
       python tools/filter_bench.py --tags [--reps 5] [--append 10000000] [--loop-tags 8]
       python tools/filter_bench.py --values [--reps 5] [--append 10000000] [--loop-tags 8]
       python tools/filter_bench.py --tags-values [--reps 5] [--loop-tags 8]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def slots_bench(args, pkg, torch, dev, c, g, q, dd, ll, nq, labels_of, out):
    n10 = c.n_total // 10
    same = labels_of(n10, 30)
    t = time.perf_counter()
    g.set_filter_slot_dev(0, n10, same)
    out["first_set_filter_slot_dev_ms"] = (time.perf_counter() - t) * 1e3
    for s in range(1, pkg.FILTER_SLOTS):
        g.set_filter_slot_dev(s, n10, labels_of(n10, 100 + s))
    assert all(g.filter_slot_info(s) == (0, n10, c.n_total) for s in range(pkg.FILTER_SLOTS))
    out["memory_GB_with_32_slots"] = g.memory_bytes() / 1e9
    one = torch.zeros(nq, dtype=torch.uint8, device=dev)
    dealt = (torch.arange(nq, device=dev) % pkg.FILTER_SLOTS).to(torch.uint8)
    none = torch.full((nq,), pkg.SLOT_NONE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    forms = [("a unfiltered", None, False), ("b set_filter 10 %", None, True), ("c slots, one slot", one, False),
             ("d slots, 32 dealt", dealt, False), ("e slots, all NONE", none, False)]

    def step(qs):
        if qs is None:
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        else:
            g.search_slots_dev(nq, 1, q, qs, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)

    def measure(qs, steps=10):
        for _ in range(5):
            step(qs)
        g.sync()
        t = time.perf_counter()
        for _ in range(steps):
            step(qs)
        g.sync()
        wall = (time.perf_counter() - t) * 1e3 / steps
        g.set_profiling(2)
        g.reset_stage_ms()
        for _ in range(steps):
            step(qs)
        g.sync()
        scan = g.stage_ms()["scan"][0] / steps
        g.set_profiling(0)
        return wall, scan, g.last_scan_kernel()

    runs = {name: {"step_ms": [], "scan_ms": []} for name, _, _ in forms}
    for _ in range(max(5, args.reps)):
        for name, qs, single in forms:
            if single:
                g.set_filter_dev(n10, same)
            wall, scan, kernel = measure(qs)
            if single:
                g.clear_filter()
            runs[name]["step_ms"].append(wall)
            runs[name]["scan_ms"].append(scan)
            runs[name]["kernel"] = kernel
    for name, r in runs.items():
        for key in ("step_ms", "scan_ms"):
            v = r[key]
            r[key + "_min_mean_max"] = [min(v), sum(v) / len(v), max(v)]
        log("[filter_bench] %-20s step %.4f ms, scan %.4f ms  (%s)" %
            (name, r["step_ms_min_mean_max"][1], r["scan_ms_min_mean_max"][1], r["kernel"]))
    out["slots_search"] = runs
    b, cc = runs["b set_filter 10 %"], runs["c slots, one slot"]
    out["c_minus_b_scan_ms"] = cc["scan_ms_min_mean_max"][1] - b["scan_ms_min_mean_max"][1]
    out["b_scan_spread_ms"] = b["scan_ms_min_mean_max"][2] - b["scan_ms_min_mean_max"][0]
    out["c_minus_b_step_ms"] = cc["step_ms_min_mean_max"][1] - b["step_ms_min_mean_max"][1]
    out["b_step_spread_ms"] = b["step_ms_min_mean_max"][2] - b["step_ms_min_mean_max"][0]

    # 4. install and re-mark
    n10m = min(10 ** 7, c.n_total)
    lab = labels_of(n10m, 31)
    t = time.perf_counter()
    g.set_filter_slot_dev(0, n10m, lab)
    out["set_filter_slot_dev_10M_ms"] = (time.perf_counter() - t) * 1e3
    n = args.append
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    li = torch.randint(0, c.nc, (n,), device=dev, generator=gen, dtype=torch.int32)
    codes = torch.randint(0, 256, (n, c.M), device=dev, generator=gen, dtype=torch.uint8)
    ncodes = torch.randint(0, 255, (n,), device=dev, generator=gen, dtype=torch.uint8)
    torch.cuda.synchronize(dev)
    appends = []
    first_id = c.n_total

    def timed_append(what):
        nonlocal first_id
        ids = (torch.arange(n, device=dev, dtype=torch.int64) + first_id).to(torch.int32)
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        g.append_ivf_dev(n, li, ids, codes, ncodes)
        g.sync()
        ms = (time.perf_counter() - t) * 1e3
        first_id += n
        appends.append({"installed": what, "append_ms": ms})
        log("[filter_bench] append_ivf_dev of %d codes, %s: %.1f ms" % (n, what, ms))

    g.clear_filter_slot()
    timed_append("nothing (warm-up: allocations)")
    timed_append("nothing")
    timed_append("nothing")
    g.set_filter_dev(n10, same)
    timed_append("the single filter")
    timed_append("the single filter")
    g.clear_filter()
    for count in (1, 8, 32):
        for s in range(count):
            if g.filter_slot_info(s)[0] < 0:
                g.set_filter_slot_dev(s, n10, labels_of(n10, 100 + s))
        timed_append("%d slots" % count)  # the first append after an install also allocates the larger planes anew
        timed_append("%d slots" % count)
    out["append"] = appends


def tags_bench(args, pkg, torch, dev, c, g, q, dd, ll, nq, out):
    n = c.n_total
    ids = torch.arange(n, device=dev, dtype=torch.int64)

    def install(modulus):
        lab = ids.to(torch.int32)
        tg = (ids % modulus).to(torch.int16)
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        g.set_tags_dev(n, lab, tg)
        ms = (time.perf_counter() - t) * 1e3
        del lab, tg
        return ms

    # the slots' partition: row r in slot r % 32
    for s in range(pkg.FILTER_SLOTS):
        lab = (torch.arange(n // 32 + (1 if s < n % 32 else 0), device=dev, dtype=torch.int64) * 32 + s).to(torch.int32)
        torch.cuda.synchronize(dev)
        g.set_filter_slot_dev(s, lab.numel(), lab)
        del lab
    out["memory_GB_with_32_slots"] = g.memory_bytes() / 1e9
    qslots = (torch.arange(nq, device=dev) % 32).to(torch.uint8)
    qtags32 = (torch.arange(nq, device=dev) % 32).to(torch.int16)
    qtags1k = (torch.arange(nq, device=dev) % 1024).to(torch.int16)
    torch.cuda.synchronize(dev)

    def step(form):
        kind, pick = form
        if kind == "plain":
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        elif kind == "slots":
            g.search_slots_dev(nq, 1, q, pick, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        else:
            g.search_tags_dev(nq, 1, q, pick, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)

    def measure(form, steps=10):
        for _ in range(5):
            step(form)
        g.sync()
        t = time.perf_counter()
        for _ in range(steps):
            step(form)
        g.sync()
        wall = (time.perf_counter() - t) * 1e3 / steps
        g.set_profiling(2)
        g.reset_stage_ms()
        for _ in range(steps):
            step(form)
        g.sync()
        scan = g.stage_ms()["scan"][0] / steps
        g.set_profiling(0)
        return wall, scan, g.last_scan_kernel()

    runs = {}

    def series(name, form):
        wall, scan, kernel = measure(form)
        r = runs.setdefault(name, {"step_ms": [], "scan_ms": []})
        r["step_ms"].append(wall)
        r["scan_ms"].append(scan)
        r["kernel"] = kernel

    # 32 tags and 1 024 tags are two tables: each is measured with its own installed, alternating with (a) and (b)
    out["set_tags_dev_all_rows_ms"] = []
    for modulus, name, qt in ((32, "c tags, 32 dealt", qtags32), (1024, "d tags, 1024 dealt", qtags1k)):
        out["set_tags_dev_all_rows_ms"].append(install(modulus))
        for _ in range(max(5, args.reps)):
            series("a unfiltered (beside %d tags)" % modulus, ("plain", None))
            series("b slots, 32 dealt (beside %d tags)" % modulus, ("slots", qslots))
            series(name, ("tags", qt))
    out["memory_GB_with_32_slots_and_tags"] = g.memory_bytes() / 1e9
    for name, r in runs.items():
        for key in ("step_ms", "scan_ms"):
            v = r[key]
            r[key + "_min_mean_max"] = [min(v), sum(v) / len(v), max(v)]
        log("[filter_bench] %-36s step %.4f ms, scan %.4f ms  (%s)" %
            (name, r["step_ms_min_mean_max"][1], r["scan_ms_min_mean_max"][1], r["kernel"]))
    out["tags_search"] = runs
    b, cc = runs["b slots, 32 dealt (beside 32 tags)"], runs["c tags, 32 dealt"]
    out["c_minus_b_scan_ms"] = cc["scan_ms_min_mean_max"][1] - b["scan_ms_min_mean_max"][1]
    out["b_scan_spread_ms"] = b["scan_ms_min_mean_max"][2] - b["scan_ms_min_mean_max"][0]
    out["c_minus_b_step_ms"] = cc["step_ms_min_mean_max"][1] - b["step_ms_min_mean_max"][1]
    out["b_step_spread_ms"] = b["step_ms_min_mean_max"][2] - b["step_ms_min_mean_max"][0]

    # 6. the loop one search_tags call with 1 024 tags replaces
    g.clear_filter_slot()
    per_tag_q = max(1, nq // 1024)
    loop = []
    for t_ in range(args.loop_tags):
        lab = (torch.arange(n // 1024 + (1 if t_ < n % 1024 else 0), device=dev, dtype=torch.int64) * 1024 + t_).to(torch.int32)
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        g.set_filter_dev(lab.numel(), lab)
        g.search_dev(per_tag_q, 1, q[t_ * per_tag_q:(t_ + 1) * per_tag_q], dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        g.sync()
        loop.append((time.perf_counter() - t) * 1e3)
        del lab
    g.clear_filter()
    out["loop_ms_per_tag"] = loop
    out["loop_ms_1024_tags_extrapolated"] = sum(loop[1:]) / max(1, len(loop) - 1) * 1024  # the first call allocates
    log("[filter_bench] set_filter_dev + search_dev per tag: %s ms; x 1024 = %.0f ms against one search_tags step of %.3f ms"
        % (", ".join("%.2f" % v for v in loop), out["loop_ms_1024_tags_extrapolated"],
           runs["d tags, 1024 dealt"]["step_ms_min_mean_max"][1]))

    # 7. install and re-derivation
    n10m = min(10 ** 7, n)
    gen = torch.Generator(device=dev)
    gen.manual_seed(31)
    lab = (torch.arange(n10m, device=dev, dtype=torch.int64) * max(1, n // n10m))[torch.randperm(n10m, device=dev, generator=gen)]
    lab = lab.to(torch.int32)  # the same bits as uint32: every K-th id, in random order
    tg = (torch.arange(n10m, device=dev) % 1024).to(torch.int16)
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    g.set_tags_dev(n10m, lab, tg)
    out["set_tags_dev_10M_ms"] = (time.perf_counter() - t) * 1e3
    log("[filter_bench] set_tags_dev of %d labels on %d rows: %.1f ms" % (n10m, n, out["set_tags_dev_10M_ms"]))
    del lab, tg
    na = args.append
    li = torch.randint(0, c.nc, (na,), device=dev, generator=gen, dtype=torch.int32)
    codes = torch.randint(0, 256, (na, c.M), device=dev, generator=gen, dtype=torch.uint8)
    ncodes = torch.randint(0, 255, (na,), device=dev, generator=gen, dtype=torch.uint8)
    torch.cuda.synchronize(dev)
    appends = []
    first_id = n

    def timed_append(what):
        nonlocal first_id
        new = (torch.arange(na, device=dev, dtype=torch.int64) + first_id).to(torch.int32)
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        g.append_ivf_dev(na, li, new, codes, ncodes)
        g.sync()
        ms = (time.perf_counter() - t) * 1e3
        first_id += na
        appends.append({"installed": what, "append_ms": ms})
        log("[filter_bench] append_ivf_dev of %d codes, %s: %.1f ms" % (na, what, ms))

    timed_append("the tag table (warm-up: allocations)")
    timed_append("the tag table")
    timed_append("the tag table")
    g.clear_tags()
    timed_append("nothing")
    timed_append("nothing")
    out["append"] = appends


def values_bench(args, pkg, torch, dev, c, g, q, dd, ll, nq, out):
    n = c.n_total
    ids = torch.arange(n, device=dev, dtype=torch.int64)
    lab = ids.to(torch.int32)
    tg = (ids % 1024).to(torch.int16)
    vl = (ids % 1024).to(torch.int32)
    del ids
    torch.cuda.synchronize(dev)
    mem0 = g.memory_bytes()
    g.set_tags_dev(n, lab, tg)
    t = time.perf_counter()
    g.set_values_dev(n, lab, vl)
    out["set_values_dev_all_rows_ms"] = (time.perf_counter() - t) * 1e3
    del lab, tg, vl
    out["memory_GB_tags_and_values"] = (g.memory_bytes() - mem0) / 1e9
    assert g.values_info() == (n, n, n) and g.value_rows(0, 127) == 128 * (n // 1024) + min(n % 1024, 128)
    qi = torch.arange(nq, device=dev) % 1024
    qtags = qi.to(torch.int16)
    points = torch.stack([qi, qi], 1).to(torch.int32).contiguous()
    lo = (qi * 7) % 897  # 897 = 1024 - 127: every interval lies inside the values, and neighbours overlap
    eighth = torch.stack([lo, lo + 127], 1).to(torch.int32).contiguous()
    full = torch.stack([torch.zeros_like(qi), torch.full_like(qi, -1)], 1).to(torch.int32).contiguous()  # (0, 0xffffffff)
    torch.cuda.synchronize(dev)

    def step(form):
        kind, pick = form
        if kind == "plain":
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        elif kind == "tags":
            g.search_tags_dev(nq, 1, q, pick, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        else:
            g.search_values_dev(nq, 1, q, pick, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)

    def measure(form, steps=10):
        for _ in range(5):
            step(form)
        g.sync()
        t = time.perf_counter()
        for _ in range(steps):
            step(form)
        g.sync()
        wall = (time.perf_counter() - t) * 1e3 / steps
        g.set_profiling(2)
        g.reset_stage_ms()
        for _ in range(steps):
            step(form)
        g.sync()
        scan = g.stage_ms()["scan"][0] / steps
        g.set_profiling(0)
        return wall, scan, g.last_scan_kernel()

    forms = [("a unfiltered", ("plain", None)), ("b tags, 1024 dealt", ("tags", qtags)),
             ("c values, 1024 points", ("values", points)), ("d values, 1/8 intervals", ("values", eighth)),
             ("e values, all (0, 0xffffffff)", ("values", full))]
    runs = {name: {"step_ms": [], "scan_ms": []} for name, _ in forms}
    for _ in range(max(5, args.reps)):
        for name, form in forms:
            wall, scan, kernel = measure(form)
            runs[name]["step_ms"].append(wall)
            runs[name]["scan_ms"].append(scan)
            runs[name]["kernel"] = kernel
    # the same rows pass (b) and (c): the same answers
    step(("tags", qtags))
    g.sync()
    want = ll.clone()
    step(("values", points))
    g.sync()
    out["points_equal_tags"] = bool(torch.equal(want, ll))
    for name, r in runs.items():
        for key in ("step_ms", "scan_ms"):
            v = r[key]
            r[key + "_min_mean_max"] = [min(v), sum(v) / len(v), max(v)]
        log("[filter_bench] %-32s step %.4f ms, scan %.4f ms  (%s)" %
            (name, r["step_ms_min_mean_max"][1], r["scan_ms_min_mean_max"][1], r["kernel"]))
    out["values_search"] = runs
    b, cc = runs["b tags, 1024 dealt"], runs["c values, 1024 points"]
    out["c_minus_b_scan_ms"] = cc["scan_ms_min_mean_max"][1] - b["scan_ms_min_mean_max"][1]
    out["b_scan_spread_ms"] = b["scan_ms_min_mean_max"][2] - b["scan_ms_min_mean_max"][0]
    out["c_minus_b_step_ms"] = cc["step_ms_min_mean_max"][1] - b["step_ms_min_mean_max"][1]
    out["b_step_spread_ms"] = b["step_ms_min_mean_max"][2] - b["step_ms_min_mean_max"][0]

    # 9. the loop one search_values call replaces: a filter per distinct interval
    distinct = torch.unique(eighth, dim=0)
    out["distinct_intervals"] = int(distinct.shape[0])
    per_q = max(1, nq // int(distinct.shape[0]))
    loop = []
    for i in range(args.loop_tags):
        a, b_ = int(distinct[i, 0]), int(distinct[i, 1])
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        r = torch.arange(n, device=dev, dtype=torch.int64)
        m = r % 1024
        lab = r[(m >= a) & (m <= b_)].to(torch.int32)  # the application's side of the loop: the labels of the interval
        del r, m
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        g.set_filter_dev(lab.numel(), lab)
        g.search_dev(per_q, 1, q[i * per_q:(i + 1) * per_q], dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        g.sync()
        t2 = time.perf_counter()
        loop.append({"labels_ms": (t1 - t) * 1e3, "set_filter_and_search_ms": (t2 - t1) * 1e3})
        del lab
    g.clear_filter()
    out["loop_per_interval"] = loop
    tail = [x["set_filter_and_search_ms"] for x in loop[1:]] or [loop[0]["set_filter_and_search_ms"]]  # the first call allocates
    out["loop_ms_all_intervals_extrapolated"] = sum(tail) / len(tail) * int(distinct.shape[0])
    log("[filter_bench] set_filter_dev + search_dev per interval: %s ms; x %d = %.0f ms against one search_values step of %.3f ms"
        % (", ".join("%.2f" % x["set_filter_and_search_ms"] for x in loop), int(distinct.shape[0]),
           out["loop_ms_all_intervals_extrapolated"], runs["d values, 1/8 intervals"]["step_ms_min_mean_max"][1]))

    # 10. install and re-derivation
    g.clear_tags()
    n10m = min(10 ** 7, n)
    gen = torch.Generator(device=dev)
    gen.manual_seed(31)
    lab = (torch.arange(n10m, device=dev, dtype=torch.int64) * max(1, n // n10m))[torch.randperm(n10m, device=dev, generator=gen)]
    lab = lab.to(torch.int32)  # the same bits as uint32: every K-th id, in random order
    vl = (torch.arange(n10m, device=dev) % 1024).to(torch.int32)
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    g.set_values_dev(n10m, lab, vl)
    out["set_values_dev_10M_ms"] = (time.perf_counter() - t) * 1e3
    log("[filter_bench] set_values_dev of %d labels on %d rows: %.1f ms" % (n10m, n, out["set_values_dev_10M_ms"]))
    del lab, vl
    na = args.append
    li = torch.randint(0, c.nc, (na,), device=dev, generator=gen, dtype=torch.int32)
    codes = torch.randint(0, 256, (na, c.M), device=dev, generator=gen, dtype=torch.uint8)
    ncodes = torch.randint(0, 255, (na,), device=dev, generator=gen, dtype=torch.uint8)
    torch.cuda.synchronize(dev)
    appends = []
    first_id = n

    def timed_append(what):
        nonlocal first_id
        new = (torch.arange(na, device=dev, dtype=torch.int64) + first_id).to(torch.int32)
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        g.append_ivf_dev(na, li, new, codes, ncodes)
        g.sync()
        ms = (time.perf_counter() - t) * 1e3
        first_id += na
        appends.append({"installed": what, "append_ms": ms})
        log("[filter_bench] append_ivf_dev of %d codes, %s: %.1f ms" % (na, what, ms))

    timed_append("the value table (warm-up: allocations)")
    timed_append("the value table")
    timed_append("the value table")
    g.clear_values()
    timed_append("nothing")
    timed_append("nothing")
    out["append"] = appends


def tags_values_bench(args, pkg, torch, dev, c, g, q, dd, ll, nq, out):
    """Two installs on one handle.  First row r carries tag r % 1024 and value r % 1024, so that the tag t, the point
    (t, t) and their conjunction pass the same rows and the five filtered forms must give the same answers.  Then the two
    columns are made independent -- tag r % 8 (eight tenants), value (r // 8) % 1024 (a clock that ticks once per eight
    rows) -- and each query carries one tenant and an interval of 128 consecutive values: about 1/8 x 1/8 of the rows."""
    n = c.n_total
    ids = torch.arange(n, device=dev, dtype=torch.int64)
    lab = ids.to(torch.int32)
    tg = (ids % 1024).to(torch.int16)
    vl = (ids % 1024).to(torch.int32)
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    mem0 = g.memory_bytes()
    g.set_tags_dev(n, lab, tg)
    g.set_values_dev(n, lab, vl)
    out["memory_GB_tags_and_values"] = (g.memory_bytes() - mem0) / 1e9
    assert g.tag_value_rows(5, 5, 5) == g.tag_rows(5) == g.value_rows(5, 5) == g.tag_value_rows(0xffff, 5, 5)
    qi = torch.arange(nq, device=dev) % 1024
    qtags = qi.to(torch.int16)
    none = torch.full_like(qi, -1).to(torch.int16)  # 0xffff
    points = torch.stack([qi, qi], 1).to(torch.int32).contiguous()
    full = torch.stack([torch.zeros_like(qi), torch.full_like(qi, -1)], 1).to(torch.int32).contiguous()  # (0, 0xffffffff)
    torch.cuda.synchronize(dev)

    def step(form):
        kind, t, r = form
        if kind == "plain":
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        elif kind == "tags":
            g.search_tags_dev(nq, 1, q, t, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        elif kind == "values":
            g.search_values_dev(nq, 1, q, r, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        else:
            g.search_tags_values_dev(nq, 1, q, t, r, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)

    def measure(form, steps=10):
        for _ in range(5):
            step(form)
        g.sync()
        t = time.perf_counter()
        for _ in range(steps):
            step(form)
        g.sync()
        wall = (time.perf_counter() - t) * 1e3 / steps
        g.set_profiling(2)
        g.reset_stage_ms()
        for _ in range(steps):
            step(form)
        g.sync()
        scan = g.stage_ms()["scan"][0] / steps
        g.set_profiling(0)
        return wall, scan, g.last_scan_kernel()

    def run(forms):
        runs = {name: {"step_ms": [], "scan_ms": []} for name, _ in forms}
        for _ in range(max(5, args.reps)):
            for name, form in forms:
                wall, scan, kernel = measure(form)
                runs[name]["step_ms"].append(wall)
                runs[name]["scan_ms"].append(scan)
                runs[name]["kernel"] = kernel
        for name, r in runs.items():
            for key in ("step_ms", "scan_ms"):
                v = r[key]
                r[key + "_min_mean_max"] = [min(v), sum(v) / len(v), max(v)]
            log("[filter_bench] %-40s step %.4f (%.4f-%.4f) ms, scan %.4f (%.4f-%.4f) ms  (%s)" %
                (name, r["step_ms_min_mean_max"][1], r["step_ms_min_mean_max"][0], r["step_ms_min_mean_max"][2],
                 r["scan_ms_min_mean_max"][1], r["scan_ms_min_mean_max"][0], r["scan_ms_min_mean_max"][2], r["kernel"]))
        return runs

    same = [("a unfiltered", ("plain", None, None)), ("b tags, 1024 dealt", ("tags", qtags, None)),
            ("c values, 1024 points", ("values", None, points)), ("d tags+values (t, (t, t))", ("both", qtags, points)),
            ("e tags+values (t, FULL)", ("both", qtags, full)), ("f tags+values (NONE, (t, t))", ("both", none, points)),
            ("h tags+values, all (NONE, FULL)", ("both", none, full))]
    out["same_rows"] = run(same)
    # the same rows pass (b) to (f): the same answers; (h) answers as (a)
    answers = {}
    for name, form in same:
        step(form)
        g.sync()
        answers[name] = ll.clone()
    out["same_rows_answers_equal"] = bool(all(torch.equal(answers["b tags, 1024 dealt"], answers[k]) for k in
                                            ("c values, 1024 points", "d tags+values (t, (t, t))", "e tags+values (t, FULL)",
                                             "f tags+values (NONE, (t, t))")))
    out["none_full_equals_unfiltered"] = bool(torch.equal(answers["a unfiltered"], answers["h tags+values, all (NONE, FULL)"]))
    assert out["same_rows_answers_equal"] and out["none_full_equals_unfiltered"], out

    # (g) distinct tag and interval pairs of about 1/8 x 1/8: the columns made independent -- tag r % 8 (8 tenants),
    # value (r // 8) % 1024 (a clock that ticks once per 8 rows), the interval 128 consecutive values
    tg = (ids % 8).to(torch.int16)
    vl = ((ids // 8) % 1024).to(torch.int32)
    del ids
    torch.cuda.synchronize(dev)
    g.set_tags_dev(n, lab, tg)
    g.set_values_dev(n, lab, vl)
    del tg, vl
    gtags = (qi % 8).to(torch.int16)
    lo = (qi * 7) % 897  # 897 = 1024 - 127: every interval lies inside the values, and neighbours overlap
    eighth = torch.stack([lo, lo + 127], 1).to(torch.int32).contiguous()
    torch.cuda.synchronize(dev)
    t0, lo0 = int(gtags[3]), int(lo[3])
    assert abs(g.tag_value_rows(t0, lo0, lo0 + 127) - n / 64) < n / 640
    out["eighth_eighth"] = run([("a unfiltered", ("plain", None, None)), ("b tags, 8 tenants", ("tags", gtags, None)),
                                ("c values, 1/8 intervals", ("values", None, eighth)),
                                ("g tags+values, 1/8 x 1/8 pairs", ("both", gtags, eighth))])

    # 12. the loop one call replaces: a filter per distinct (tag, interval) pair
    pairs = torch.unique(torch.cat([gtags.to(torch.int32).unsqueeze(1), eighth], 1), dim=0)
    npairs = int(pairs.shape[0])
    out["distinct_pairs"] = npairs
    per_q = max(1, nq // npairs)
    loop = []
    for i in range(args.loop_tags):
        t_, a, b_ = int(pairs[i, 0]), int(pairs[i, 1]), int(pairs[i, 2])
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        r = torch.arange(n, device=dev, dtype=torch.int64)
        v = (r // 8) % 1024
        labs = r[(r % 8 == t_) & (v >= a) & (v <= b_)].to(torch.int32)  # the application's side: the labels of the pair
        del r, v
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        g.set_filter_dev(labs.numel(), labs)
        g.search_dev(per_q, 1, q[i * per_q:(i + 1) * per_q], dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        g.sync()
        t2 = time.perf_counter()
        loop.append({"labels_ms": (t1 - t) * 1e3, "set_filter_and_search_ms": (t2 - t1) * 1e3})
        del labs
    g.clear_filter()
    out["loop_per_pair"] = loop
    tail = [x["set_filter_and_search_ms"] for x in loop[1:]] or [loop[0]["set_filter_and_search_ms"]]  # the first call allocates
    out["loop_ms_all_pairs_extrapolated"] = sum(tail) / len(tail) * npairs
    log("[filter_bench] set_filter_dev + search_dev per pair: %s ms; x %d = %.0f ms against one search_tags_values step of %.3f ms"
        % (", ".join("%.2f" % x["set_filter_and_search_ms"] for x in loop), npairs, out["loop_ms_all_pairs_extrapolated"],
           out["eighth_eighth"]["g tags+values, 1/8 x 1/8 pairs"]["step_ms_min_mean_max"][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synthetic-1B-pq16-nc993127-nprobe32")
    ap.add_argument("--sizes", default="1000,10000000,500000000")
    ap.add_argument("--fractions", default="0.5,0.1,0.01")
    ap.add_argument("--slots", action="store_true")
    ap.add_argument("--tags", action="store_true")
    ap.add_argument("--values", action="store_true")
    ap.add_argument("--tags-values", action="store_true")
    ap.add_argument("--loop-tags", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--append", type=int, default=10 ** 7)
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
    torch.cuda.synchronize(dev)  # torch's stream is not the handle's

    def qps(reps=10):
        for _ in range(5):
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        g.sync()
        t = time.perf_counter()
        for _ in range(reps):
            g.search_dev(nq, 1, q, dd, ll, c.nprobe, c.max_codes, efSearch=c.ef)
        g.sync()
        return nq * reps / (time.perf_counter() - t), g.last_scan_kernel()

    def labels_of(n, seed):
        """n distinct labels below n_total: every K-th id from a random phase, K = n_total // n (ids are the running index)"""
        K = max(1, c.n_total // n)
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        phase = int(torch.randint(0, K, (1,), device=dev, generator=gen).item())
        lab = torch.arange(n, device=dev, dtype=torch.int64) * K + phase
        lab = lab[torch.randperm(n, device=dev, generator=gen)] if n <= 10 ** 7 else lab
        t = lab.to(torch.int32)  # the same bits as uint32
        torch.cuda.synchronize(dev)
        return t

    def timed_set(n, deny, seed):
        lab = labels_of(n, seed) if n else None
        t = time.perf_counter()
        g.set_filter_dev(n, lab, deny=deny)
        ms = (time.perf_counter() - t) * 1e3
        mode, passing, total = g.filter_info()
        assert total == c.n_total and passing == (total - n if deny else n), (mode, passing, total, n)
        return ms, passing

    if args.tags_values:
        tags_values_bench(args, pkg, torch, dev, c, g, q, dd, ll, nq, out)
        g.close()
        print(json.dumps(out))
        return
    if args.values:
        values_bench(args, pkg, torch, dev, c, g, q, dd, ll, nq, out)
        g.close()
        print(json.dumps(out))
        return
    if args.tags:
        tags_bench(args, pkg, torch, dev, c, g, q, dd, ll, nq, out)
        g.close()
        print(json.dumps(out))
        return
    if args.slots:
        slots_bench(args, pkg, torch, dev, c, g, q, dd, ll, nq, labels_of, out)
        g.close()
        print(json.dumps(out))
        return

    # 1. installing
    ms, _ = timed_set(1, False, 1)
    out["first_call_ms"] = ms
    rows = []
    for i, n in enumerate(int(x) for x in args.sizes.split(",")):
        ms, passing = timed_set(n, False, 10 + i)
        ms2, _ = timed_set(n, True, 20 + i)
        rows.append({"labels": n, "allow_ms": ms, "deny_ms": ms2, "rows_passing_allow": passing})
        log("[filter_bench] set_filter_dev %d labels: allow %.2f ms, deny %.2f ms" % (n, ms, ms2))
    out["set_filter_dev"] = rows
    out["memory_GB_with_filter"] = g.memory_bytes() / 1e9
    g.clear_filter()

    # 2. searching, one handle, one run
    runs = []

    def record(name):
        v, kernel = qps()
        runs.append({"filter": name, "qps": v, "kernel": kernel, "rows_passing": g.filter_info()[1]})
        log("[filter_bench] %-18s %.0f queries/s  (%s)" % (name, v, kernel))

    record("none")
    timed_set(0, True, 0)
    record("deny nothing")
    for f in (float(x) for x in args.fractions.split(",")):
        timed_set(int(c.n_total * f), False, 30)
        record("allow %g %%" % (100 * f))
    g.clear_filter()
    record("none (again)")
    out["search"] = runs
    base = [r["qps"] for r in runs if r["filter"].startswith("none")]
    out["unfiltered_spread"] = abs(base[0] - base[1]) / max(base)
    for r in runs:
        r["of_unfiltered"] = r["qps"] / (sum(base) / len(base))
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
