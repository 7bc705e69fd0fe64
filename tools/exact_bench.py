#!/usr/bin/env python3
"""Times the exact brute-force search of the uint8 base store (ivfhnsw_gpu_exact_search_dev, kernels_exact.hip).

  1. n = 10 M x 128 (the shape the float path can also run): exact_search_dev against ivfhnsw_gpu_knn_dev on the same rows
     converted to float, same queries, k = 1 and k = 10; the labels must be equal (knn's fmaf chains are exact on these
     integers too, and both break ties to the lower id).
  2. The 10^9 x 128 store, filled on the device in ~1 GB torch chunks through upload_base_dev (the rows never exist on the
     host): 10 000 queries at k = 1 and k = 100.
  3. On both stores the exact RANGE search (ivfhnsw_gpu_exact_range_search_dev) beside exact_search at
     k = 1 -- one sweep of the unchanged kernel, the yardstick: radius 0 (the call itself), the median k = 10 and k = 100
     distances of the exact_search above (about 10 and 100 rows per query), the radius one such step further (about
     1 000), and on the small store the median distance with --dense-nq queries (the total stays below 2^32).  Every
     radius with the tile map and without it ("exact_range_map" 1 / 0): seconds of the whole call, of the count pass
     and of the fill pass (HIP events, set_profiling), results, and the ratios to the k = 1 sweep.
  4. With --filter, on both stores, exact_search under a base filter (ivfhnsw_gpu_set_base_filter_dev):
     an allow set of random rows at pass fractions 1, 1/2, 1/8, 1/32 and 1/1024 (on the large store 1/32 and 1/1024
     only), k = 1 and k = 100, in the form the rule picks -- at 1/8 and 1/32 in both forms ("exact_filter_form" 0 = pass
     words, 1 = list of passing rows) -- each beside the unfiltered call of the same run, and the time of
     set_base_filter_dev itself.
  5. With --filter-slots, on both stores, base filter slots (ivfhnsw_gpu_exact_search_slots_dev): 32 slots
     of a random 1/32 of the rows each, the queries spread over the 32 slots and NONE.  Timed alternating in one run:
     (a) one exact_search_slots_dev call, (b) the loop that answers the same batch without slots -- per slot
     set_base_filter_dev then exact_search_dev on that slot's queries, NONE's unfiltered -- with and without the installs,
     (c) the plain unfiltered call on the whole batch; k = 1 and k = 100; and the range form against its per-slot loop.
  6. With --tags, on both stores, base tags (ivfhnsw_gpu_exact_search_tags_dev), run twice: with 32 tags of
     1/32 of the rows each and with 1 024 tags in the distribution of tools/filter_recall.py --tags, 1/33 of the queries
     untagged.  Timed alternating in one run: (a) one exact_search_tags_dev call, (b) the loop it replaces -- per tag
     present set_base_filter_dev then exact_search_dev on that tag's queries -- with and without the installs, (c) at 32
     tags one exact_search_slots_dev call over the same partition; k = 1 and k = 100; the range form at the median k = 10
     distance; and the time of set_base_tags_dev over every row.
  7. With --values, on both stores, base values (ivfhnsw_gpu_exact_search_values_dev): every row holds a
     distinct value, and three batches -- 897 intervals of 1/8 of the rows, 1 000 intervals of about 100 rows, the latter
     with 1/33 of the queries on (0, 0xffffffff) -- are timed alternating in one run: (a) one _values call, (b) the loop it
     replaces, per distinct interval set_base_filter_dev(the interval's rows) + the plain call on its queries, with and
     without the installs; k = 1, k = 100 and the range form at the median k = 10 distance with the reorder's share of
     it; and the time of set_base_values_dev over every row.
     With --f16 --tags-values a tag AND an interval per query on the float16 store (ivfhnsw_gpu_exact_search_f16_tags_values_dev,
     DESIGN.md 3.33) at d = 128: intervals of an eighth of each tag's rows under ascending and under shuffled values beside
     exact_search_f16_tags_dev, the all-whole batch beside it and the all-(NONE, whole) batch beside the plain call.
  8. With --f16 ONLY the float16 store (ivfhnsw_gpu_exact_search_f16_dev): --small-rows x 128 and x 96 rows
     of random bytes as float32, k = 1, 10 and 100, alternating in one process with ivfhnsw_gpu_knn_dev on the same rows as
     float32 (k <= 80) and exact_search_dev on a uint8 store of the same rows; all three are exact on such rows and must
     agree.  Store bytes per second are those of each call's own rows (2, 4 and 1 bytes a value).
     With --f16 --range the float16 store's exact RANGE search (ivfhnsw_gpu_exact_range_search_f16_dev) as
     well, as 3. does for the uint8 one: at the median k = 10 and k = 100 distances and one step beyond, the call with the
     tile map and without it ALTERNATING with the k = 1 f16 sweep, the yardstick, in one process (whole call, count pass
     and fill pass, and the ratios to the sweep); and at the k = 100 radius the split count the rule picks beside one
     neighbour on each side ("exact_splits").
     With --f16 --tags base tags on the float16 store (ivfhnsw_gpu_exact_search_f16_tags_dev) at d = 128:
     with 32 and with 1 024 tags, k = 1 and 100, the tagged call under the rule's split count and under its two neighbours
     ALTERNATING with exact_search_tags_dev on the uint8 store of the same rows (the two must agree); and the all-NONE batch
     alternating with the plain exact_search_f16_dev, its plan stage (plan and gather) from the stage profiler.
     Per tag count also the range form under the tags (ivfhnsw_gpu_exact_range_search_f16_tags_dev) at the
     radius of the tagged 10th neighbour, alternating with exact_range_search_tags_dev on the uint8 store (the two must
     agree), the tagged k = 1 sweep, the call without the tile map and the call under the neighbouring split counts; and
     its all-NONE batch alternating with the plain exact_range_search_f16_dev.
     With --f16 --values base values on the float16 store (ivfhnsw_gpu_exact_search_f16_values_dev) at
     d = 128: the three workloads of 7., k = 1 and 100, ALTERNATING with exact_search_values_dev on the uint8 store of the
     same rows (the two must agree); and the all-FULL batch alternating with the plain exact_search_f16_dev, with the plan
     stage (plan and gather) from the stage profiler.  Per workload also the range form under the intervals
     (ivfhnsw_gpu_exact_range_search_f16_values_dev) at the radius of the 30th neighbour inside the interval,
     alternating with exact_range_search_values_dev on the uint8 store (equal lims, labels and distances required), the
     k = 1 search under the intervals, the call without the tile map and under the neighbouring split counts; the all-FULL
     batch alternating with the plain exact_range_search_f16_dev.
Each figure: warm-up runs, then the median of several repetitions, each timed from the call to the end of the stream's
work.  Reported: seconds, 2 nq n d / t in TOP/s, store bytes per second per pass (n d / t) and, with one pass per query
tile, the bytes per second all tiles stream together.
usage: python tools/exact_bench.py [--rows 1000000000] [--small-rows 10000000] [--nq 10000] [--reps 3] [--warmup 1]
                                   [--no-big] [--no-small] [--no-knn] [--no-range] [--filter] [--filter-slots] [--tags] [--values]
                                   [--dense-nq 512] [--f16 [--range] [--tags] [--values]]
                                   [--out result.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def fill_store(g, torch, dev, n, d, seed, keep=False):
    """n x d random bytes into the base store in chunks of ~1 GB; keep: also return them as one tensor."""
    chunk_rows = min(n, (1 << 30) // d)
    buf = torch.empty((chunk_rows, d), dtype=torch.uint8, device=dev)
    kept = torch.empty((n, d), dtype=torch.uint8, device=dev) if keep else None
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    t0 = time.time()
    for first in range(0, n, chunk_rows):
        m = min(chunk_rows, n - first)
        buf.random_(0, 256, generator=gen)
        if keep:
            kept[first:first + m] = buf[:m]
        torch.cuda.synchronize(dev)
        g.upload_base_dev(n, d, first, m, buf)
    del buf
    log("[exact_bench] %d x %d base store on the device: %.1fs, %.1f GB held" % (n, d, time.time() - t0, g.memory_bytes() / 1e9))
    return kept


def timed(torch, dev, fn, warmup, reps, what):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    ts = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t0)
        log("[exact_bench] %s rep %d: %.4f s" % (what, i, ts[-1]))
    return statistics.median(ts), ts


def figures(name, n, d, nq, k, t, ts, rows_per_tile=None):
    r = {"what": name, "rows": n, "d": d, "nq": nq, "k": k, "seconds": round(t, 5), "reps": [round(x, 5) for x in ts],
         "TOPs": round(2.0 * nq * n * d / t / 1e12, 2), "store_TB_per_s_per_pass": round(n * d / t / 1e12, 4)}
    if rows_per_tile:  # every query tile streams the whole store: what the caches deliver to the CUs
        r["query_tiles"] = -(-nq // rows_per_tile)
        r["streamed_TB_per_s"] = round(r["query_tiles"] * n * d / t / 1e12, 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--small-rows", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-big", action="store_true")
    ap.add_argument("--no-small", action="store_true")
    ap.add_argument("--no-knn", action="store_true", help="skip the float knn comparison on the small store")
    ap.add_argument("--no-range", action="store_true", help="skip the exact range search legs")
    ap.add_argument("--filter", action="store_true", help="add the base-filter legs (DESIGN.md 3.18)")
    ap.add_argument("--filter-slots", action="store_true", help="add the base-filter-slot legs (DESIGN.md 3.20)")
    ap.add_argument("--tags", action="store_true", help="add the base-tag legs (DESIGN.md 3.22)")
    ap.add_argument("--values", action="store_true", help="add the base-value legs (DESIGN.md 3.25)")
    ap.add_argument("--tags-values", action="store_true", help="with --f16: add the tag-and-interval legs (DESIGN.md 3.33)")
    ap.add_argument("--f16", action="store_true", help="only the float16 store's legs (DESIGN.md 3.27), at d = 128 and d = 96 on --small-rows rows")
    ap.add_argument("--range", action="store_true", help="with --f16: add the float16 store's exact range search legs (DESIGN.md 3.28)")
    ap.add_argument("--dense-nq", type=int, default=512, help="queries of the dense (median distance) range leg")
    ap.add_argument("--out", default=None, help="write the whole result as JSON here")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    dev = torch.device("cuda", 0)
    g = pkg.GpuIndex(0)
    g.set_stream(torch.cuda.current_stream(dev).cuda_stream)  # one stream: torch's synchronize covers the library's work
    d, nq = args.d, args.nq
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    q = torch.empty((nq, d), dtype=torch.uint8, device=dev).random_(0, 256, generator=gen)
    result = {"device": torch.cuda.get_device_name(dev), "rows": []}

    def exact(n, k, name):
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        ol = torch.empty((nq, k), dtype=torch.int64, device=dev)
        t, ts = timed(torch, dev, lambda: g.exact_search_dev(nq, q, d, k, od, ol), args.warmup, args.reps,
                      "%s exact k=%d" % (name, k))
        r = figures("exact_search_dev", n, d, nq, k, t, ts, 128 if k <= 32 else 64)  # kernels_exact.hip's strips
        result["rows"].append(r)
        print(json.dumps(r), flush=True)
        return r, ol, od

    lims = torch.empty((nq + 1,), dtype=torch.int64, device=dev)

    def range_legs(n, name, k1_seconds, d10, d100, dense_radius=None):
        """The exact range search at each radius, with and without the tile map, against the k = 1 sweep."""
        r10, r100 = float(d10.median()), float(d100.median())
        legs = [("0", 0.0, nq), ("k=10 distance", r10, nq), ("k=100 distance", r100, nq),
                ("one step beyond", 2 * r100 - r10, nq)]
        if dense_radius is not None:
            legs.append(("median distance", dense_radius, min(nq, args.dense_nq)))
        g.set_profiling(True)
        for what, radius, m in legs:
            for use_map in (1, 0):
                g.set_option("exact_range_map", use_map)
                total = [0]

                def call():
                    total[0] = g.exact_range_search_dev(m, q, d, radius, lims)
                for _ in range(args.warmup):
                    call()
                g.reset_stage_ms()
                t, ts = timed(torch, dev, call, 0, args.reps, "%s range '%s' map=%d" % (name, what, use_map))
                st = g.stage_ms()
                r = {"what": "exact_range_search_dev", "rows": n, "d": d, "nq": m, "radius": what, "radius_value": radius,
                     "tile_map": bool(use_map), "results": total[0], "results_per_query": round(total[0] / m, 2),
                     "seconds": round(t, 5), "reps": [round(x, 5) for x in ts],
                     "count_pass_s": round(st["scan"][0] / 1e3 / max(1, args.reps), 5),
                     "fill_pass_s": round(st["select"][0] / 1e3 / max(1, args.reps), 5),
                     "k1_sweep_s": round(k1_seconds * m / nq, 5)}
                for key in ("seconds", "count_pass_s", "fill_pass_s"):
                    r[key.replace("_s", "").replace("seconds", "total") + "_over_k1"] = round(r[key] / r["k1_sweep_s"], 3)
                result["rows"].append(r)
                print(json.dumps(r), flush=True)
                if radius == 0.0:
                    break  # no sweep, no map
        g.set_profiling(False)
        g.set_option("exact_range_map", -1)

    def random_rows(n, fraction, seed):
        """About fraction * n distinct random row numbers ascending, as an int32 tensor on the device (n < 2^31)."""
        if fraction >= 1:
            return torch.arange(n, dtype=torch.int32, device=dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        parts, chunk = [], 1 << 26
        for first in range(0, n, chunk):
            m = min(chunk, n - first)
            hit = torch.rand(m, device=dev, generator=gen) < fraction
            parts.append((hit.nonzero().flatten() + first).to(torch.int32))
        return torch.cat(parts)

    def filter_legs(n, name, plain_seconds, fractions):
        """exact_search under an allow set of random rows, per fraction, k and form, beside the unfiltered call."""
        for den in fractions:
            labels = random_rows(n, 1.0 / den, 1000 + den)
            torch.cuda.synchronize(dev)
            t_set, ts_set = timed(torch, dev, lambda: g.set_base_filter_dev(labels.numel(), labels), args.warmup, args.reps,
                                  "%s set_base_filter 1/%d" % (name, den))
            mode, npass, total = g.base_filter_info()
            assert npass == labels.numel() and total == n
            r = {"what": "set_base_filter_dev", "rows": n, "fraction": "1/%d" % den, "rows_passing": npass,
                 "seconds": round(t_set, 5), "reps": [round(x, 5) for x in ts_set]}
            result["rows"].append(r)
            print(json.dumps(r), flush=True)
            rule_is_list = npass <= n // 8
            forms = (0, 1) if den in (8, 32) else (-1,)
            for k in (1, 100):
                od = torch.empty((nq, k), dtype=torch.float32, device=dev)
                ol = torch.empty((nq, k), dtype=torch.int64, device=dev)
                for form in forms:
                    g.set_option("exact_filter_form", form)
                    if form == 1 and not rule_is_list:
                        g.set_base_filter_dev(labels.numel(), labels)  # the set keeps the list when the option asks for it
                    t, ts = timed(torch, dev, lambda: g.exact_search_dev(nq, q, d, k, od, ol), args.warmup, args.reps,
                                  "%s filtered 1/%d k=%d form=%d" % (name, den, k, form))
                    used = "list" if (form == 1 or (form == -1 and rule_is_list)) else "words"
                    r = {"what": "exact_search_dev filtered", "rows": n, "d": d, "nq": nq, "k": k, "fraction": "1/%d" % den,
                         "rows_passing": npass, "form": used, "forced": form != -1, "rule_picks": "list" if rule_is_list else "words",
                         "seconds": round(t, 5), "reps": [round(x, 5) for x in ts], "unfiltered_s": round(plain_seconds[k], 5),
                         "over_unfiltered": round(t / plain_seconds[k], 4)}
                    result["rows"].append(r)
                    print(json.dumps(r), flush=True)
            g.set_option("exact_filter_form", -1)
            del labels
        g.clear_base_filter()

    def slots_legs(n, name, d10):
        """One _slots call against the per-slot loop of single-filter calls and the plain call, alternating."""
        nslots, none_share = 32, 33  # queries cycle over the 32 slots and NONE: 1/33 of them unfiltered
        sets = [random_rows(n, 1.0 / 32, 5000 + s) for s in range(nslots)]
        qs = (torch.arange(nq, device=dev) % none_share).to(torch.uint8)
        qs[qs == nslots] = 0xff
        perm = torch.randperm(nq, device=dev, generator=torch.Generator(device=dev).manual_seed(9))
        qs = qs[perm].contiguous()
        groups = [(s, (qs == (0xff if s == nslots else s)).nonzero().flatten()) for s in range(nslots + 1)]
        sub = [(s, q[idx].contiguous(), idx) for s, idx in groups]
        for s in range(nslots):
            g.set_base_filter_slot_dev(s, sets[s].numel(), sets[s])
        torch.cuda.synchronize(dev)
        radius = float(d10.median())

        def loop(k, od, ol, installs):
            """the parent commit's way; installs False: only the searches are timed"""
            t = 0.0
            for s, qsub, idx in sub:
                t0 = time.perf_counter()
                if s == nslots:
                    g.clear_base_filter()
                else:
                    g.set_base_filter_dev(sets[s].numel(), sets[s])
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                if k:
                    g.exact_search_dev(qsub.shape[0], qsub, d, k, od[:qsub.shape[0]], ol[:qsub.shape[0]])
                else:
                    g.exact_range_search_dev(qsub.shape[0], qsub, d, radius, lims)
                torch.cuda.synchronize(dev)
                t += time.perf_counter() - (t0 if installs else t1)
            g.clear_base_filter()
            return t

        for k in (1, 100, 0):  # 0: the range form
            od = torch.empty((nq, max(k, 1)), dtype=torch.float32, device=dev)
            ol = torch.empty((nq, max(k, 1)), dtype=torch.int64, device=dev)
            ta, tb, tbi, tc = [], [], [], []
            for rep in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                if k:
                    g.exact_search_slots_dev(nq, q, d, k, qs, od, ol)
                else:
                    g.exact_range_search_slots_dev(nq, q, d, qs, radius, lims)
                torch.cuda.synchronize(dev)
                a = time.perf_counter() - t0
                full = loop(k, od, ol, True)
                only = loop(k, od, ol, False)
                t0 = time.perf_counter()
                if k:
                    g.exact_search_dev(nq, q, d, k, od, ol)
                else:
                    g.exact_range_search_dev(nq, q, d, radius, lims)
                torch.cuda.synchronize(dev)
                c = time.perf_counter() - t0
                log("[exact_bench] %s slots k=%d rep %d: slots call %.4f s, loop %.4f s (searches alone %.4f s), plain %.4f s"
                    % (name, k, rep, a, full, only, c))
                if rep >= args.warmup:
                    ta.append(a), tbi.append(full), tb.append(only), tc.append(c)
            ma, mbi, mb, mc = (statistics.median(x) for x in (ta, tbi, tb, tc))
            r = {"what": "exact_search_slots_dev" if k else "exact_range_search_slots_dev", "rows": n, "d": d, "nq": nq,
                 "k": k if k else None, "radius_value": None if k else radius, "slots": nslots, "fraction": "1/32",
                 "unfiltered_share": "1/%d" % none_share, "slots_call_s": round(ma, 5), "loop_with_installs_s": round(mbi, 5),
                 "loop_searches_only_s": round(mb, 5), "plain_unfiltered_s": round(mc, 5),
                 "loop_with_installs_over_slots": round(mbi / ma, 3), "loop_searches_only_over_slots": round(mb / ma, 3),
                 "slots_over_plain": round(ma / mc, 4), "reps_slots": [round(x, 5) for x in ta]}
            result["rows"].append(r)
            print(json.dumps(r), flush=True)
        g.clear_base_filter_slot()

    def tags_legs(n, name, d10, ntags):
        """One _tags call against the per-tag loop of single-filter calls (and, at 32 tags, one _slots call), alternating."""
        none_share, none = 33, 0xffff  # 1/33 of the queries untagged
        gen = torch.Generator(device=dev)
        gen.manual_seed(7000 + ntags)
        order = torch.randperm(n, device=dev, generator=gen)
        tags = torch.empty(n, dtype=torch.int16, device=dev)
        if ntags == 32:  # 1/32 of the rows each
            tags[order] = (torch.arange(n, device=dev) % 32).to(torch.int16)
        else:            # the distribution of tools/filter_recall.py: tags 0..3 hold 1/8 each, the others share the rest
            big = n // 8
            for t in range(4):
                tags[order[t * big:(t + 1) * big]] = t
            rest = order[4 * big:]
            tags[rest] = (4 + torch.arange(rest.numel(), device=dev) % (ntags - 4)).to(torch.int16)
        del order
        all_rows = torch.arange(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        t_set, ts_set = timed(torch, dev, lambda: g.set_base_tags_dev(n, all_rows, tags), args.warmup, args.reps,
                              "%s set_base_tags %d tags" % (name, ntags))
        tagged, total, in_use = g.base_tags_info()
        assert (tagged, total, in_use) == (n, n, ntags)
        r = {"what": "set_base_tags_dev", "rows": n, "tags": ntags, "seconds": round(t_set, 5), "reps": [round(x, 5) for x in ts_set],
             "memory_GB": round(g.memory_bytes() / 1e9, 3)}
        result["rows"].append(r)
        print(json.dumps(r), flush=True)
        del all_rows
        qt = (torch.arange(nq, device=dev) % ntags).to(torch.int32)
        qt[torch.arange(nq, device=dev) % none_share == none_share - 1] = none
        qt = qt[torch.randperm(nq, device=dev, generator=gen)].contiguous()
        qtags = qt.to(torch.int16).contiguous()  # the bit pattern of the uint16
        # the rows of every tag, ascending: one stable sort
        by_tag = torch.sort(tags.to(torch.int32), stable=True)
        counts = torch.bincount(by_tag.values, minlength=ntags).cpu().tolist()
        row_lists, at = [], 0
        for t in range(ntags):
            row_lists.append(by_tag.indices[at:at + counts[t]].to(torch.int32).contiguous())
            at += counts[t]
        del by_tag
        present = sorted(set(qt.cpu().tolist()))
        sub = [(t, q[(qt == t).nonzero().flatten()].contiguous()) for t in present]
        if ntags == 32:
            for s in range(32):
                g.set_base_filter_slot_dev(s, row_lists[s].numel(), row_lists[s])
            qs = qt.to(torch.uint8).contiguous()  # 0xffff -> 0xff: NONE in both
        torch.cuda.synchronize(dev)
        radius = float(d10.median())

        def loop(k, od, ol):
            """the parent commit's way, per tag present: (seconds with the installs, seconds of the searches alone)"""
            t_all = t_search = 0.0
            for t, qsub in sub:
                t0 = time.perf_counter()
                if t == none:
                    g.clear_base_filter()
                else:
                    g.set_base_filter_dev(row_lists[t].numel(), row_lists[t])
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                if k:
                    g.exact_search_dev(qsub.shape[0], qsub, d, k, od[:qsub.shape[0]], ol[:qsub.shape[0]])
                else:
                    g.exact_range_search_dev(qsub.shape[0], qsub, d, radius, lims)
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                t_all += t2 - t0
                t_search += t2 - t1
            g.clear_base_filter()
            return t_all, t_search

        for k in (1, 100, 0):  # 0: the range form
            od = torch.empty((nq, max(k, 1)), dtype=torch.float32, device=dev)
            ol = torch.empty((nq, max(k, 1)), dtype=torch.int64, device=dev)
            ta, tb, tbi, tc = [], [], [], []
            for rep in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                if k:
                    g.exact_search_tags_dev(nq, q, d, k, qtags, od, ol)
                else:
                    g.exact_range_search_tags_dev(nq, q, d, qtags, radius, lims)
                torch.cuda.synchronize(dev)
                a = time.perf_counter() - t0
                full, only = loop(k, od, ol)
                c = float("nan")
                if ntags == 32:
                    t0 = time.perf_counter()
                    if k:
                        g.exact_search_slots_dev(nq, q, d, k, qs, od, ol)
                    else:
                        g.exact_range_search_slots_dev(nq, q, d, qs, radius, lims)
                    torch.cuda.synchronize(dev)
                    c = time.perf_counter() - t0
                log("[exact_bench] %s %d tags k=%d rep %d: tags call %.4f s, loop %.4f s (searches alone %.4f s), slots call %.4f s"
                    % (name, ntags, k, rep, a, full, only, c))
                if rep >= args.warmup:
                    ta.append(a), tbi.append(full), tb.append(only), tc.append(c)
            ma, mbi, mb, mc = (statistics.median(x) for x in (ta, tbi, tb, tc))
            r = {"what": "exact_search_tags_dev" if k else "exact_range_search_tags_dev", "rows": n, "d": d, "nq": nq,
                 "k": k if k else None, "radius_value": None if k else radius, "tags": ntags, "tags_present": len(present),
                 "unfiltered_share": "1/%d" % none_share, "tags_call_s": round(ma, 5), "loop_with_installs_s": round(mbi, 5),
                 "loop_searches_only_s": round(mb, 5), "slots_call_s": round(mc, 5) if ntags == 32 else None,
                 "loop_with_installs_over_tags": round(mbi / ma, 3), "loop_searches_only_over_tags": round(mb / ma, 3),
                 "reps_tags": [round(x, 5) for x in ta]}
            result["rows"].append(r)
            print(json.dumps(r), flush=True)
        if ntags == 32:
            g.clear_base_filter_slot()
        g.clear_base_tags()

    def values_legs(n, name, d10):
        """One _values call against the per-interval loop of single-filter calls it replaces, alternating, on three
        workloads over a store whose rows hold a permutation of 0..n-1: 897 intervals of 1/8 of the rows, 1 000 intervals of
        about 100 rows, and the latter with 1/33 of the queries on (0, 0xffffffff)."""
        gen = torch.Generator(device=dev)
        gen.manual_seed(8100)
        values = torch.randperm(n, device=dev, generator=gen).to(torch.int32)  # the value of row i
        row_of = torch.argsort(values.to(torch.int64)).to(torch.int32)          # the row that holds value v
        all_rows = torch.arange(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        t_set, ts_set = timed(torch, dev, lambda: g.set_base_values_dev(n, all_rows, values), args.warmup, args.reps,
                              "%s set_base_values" % name)
        assert g.base_values_info() == (n, n)
        r = {"what": "set_base_values_dev", "rows": n, "seconds": round(t_set, 5), "reps": [round(x, 5) for x in ts_set],
             "memory_GB": round(g.memory_bytes() / 1e9, 3)}
        result["rows"].append(r)
        print(json.dumps(r), flush=True)
        del all_rows
        radius = float(d10.median())
        full = (0, 0xffffffff)

        def spread(count, width):
            return [(a, a + width - 1) for a in ((i * (n - width)) // max(1, count - 1) for i in range(count))]
        workloads = [("897 x 1/8", spread(897, n // 8), 0), ("1000 x ~100 rows", spread(1000, min(n, 100)), 0),
                     ("1000 x ~100 rows, 1/33 full", spread(1000, min(n, 100)), 33)]
        for wname, ivs, full_share in workloads:
            pick = torch.arange(nq, device=dev) % len(ivs)
            pick = pick[torch.randperm(nq, device=dev, generator=gen)]
            is_full = (torch.arange(nq, device=dev) % full_share == full_share - 1) if full_share else torch.zeros(nq, dtype=torch.bool, device=dev)
            iv_t = torch.tensor(ivs, dtype=torch.int64, device=dev)
            qr64 = iv_t[pick]
            qr64[is_full] = torch.tensor(full, dtype=torch.int64, device=dev)
            qr = torch.where(qr64 >= 2 ** 31, qr64 - 2 ** 32, qr64).to(torch.int32).contiguous()  # the bit pattern of the uint32
            # per distinct interval present: its ascending row list and its queries
            sub = []
            for i in sorted(set(pick[~is_full].cpu().tolist())):
                lo, hi = ivs[i]
                rows_i = torch.sort(row_of[lo:hi + 1]).values.contiguous()
                sub.append((rows_i, q[((pick == i) & ~is_full).nonzero().flatten()].contiguous()))
            if full_share:
                sub.append((None, q[is_full.nonzero().flatten()].contiguous()))
            torch.cuda.synchronize(dev)

            def loop(k, od, ol):
                """the parent commit's way, per interval present: (seconds with the installs, seconds of the searches alone)"""
                t_all = t_search = 0.0
                for rows_i, qsub in sub:
                    t0 = time.perf_counter()
                    if rows_i is None:
                        g.clear_base_filter()
                    else:
                        g.set_base_filter_dev(rows_i.numel(), rows_i)
                    torch.cuda.synchronize(dev)
                    t1 = time.perf_counter()
                    if k:
                        g.exact_search_dev(qsub.shape[0], qsub, d, k, od[:qsub.shape[0]], ol[:qsub.shape[0]])
                    else:
                        g.exact_range_search_dev(qsub.shape[0], qsub, d, radius, lims)
                    torch.cuda.synchronize(dev)
                    t2 = time.perf_counter()
                    t_all += t2 - t0
                    t_search += t2 - t1
                g.clear_base_filter()
                return t_all, t_search

            for k in (1, 100, 0):  # 0: the range form
                od = torch.empty((nq, max(k, 1)), dtype=torch.float32, device=dev)
                ol = torch.empty((nq, max(k, 1)), dtype=torch.int64, device=dev)
                ta, tb, tbi, reorder, results = [], [], [], [], 0
                for rep in range(args.warmup + args.reps):
                    if not k:
                        g.set_profiling(True)
                        g.reset_stage_ms()
                    t0 = time.perf_counter()
                    if k:
                        g.exact_search_values_dev(nq, q, d, k, qr, od, ol)
                    else:
                        results = g.exact_range_search_values_dev(nq, q, d, qr, radius, lims)
                    torch.cuda.synchronize(dev)
                    a = time.perf_counter() - t0
                    if not k:
                        reorder.append(g.stage_ms()["plan"][0] / 1e3)  # the reorder is accounted as the plan stage of this call
                        g.set_profiling(False)
                    full_s, only = loop(k, od, ol)
                    log("[exact_bench] %s values '%s' k=%d rep %d: values call %.4f s, loop %.4f s (searches alone %.4f s)"
                        % (name, wname, k, rep, a, full_s, only))
                    if rep >= args.warmup:
                        ta.append(a), tbi.append(full_s), tb.append(only)
                ma, mbi, mb = (statistics.median(x) for x in (ta, tbi, tb))
                r = {"what": "exact_search_values_dev" if k else "exact_range_search_values_dev", "rows": n, "d": d, "nq": nq,
                     "k": k if k else None, "radius_value": None if k else radius, "workload": wname, "intervals_present": len(sub),
                     "values_call_s": round(ma, 5), "loop_with_installs_s": round(mbi, 5), "loop_searches_only_s": round(mb, 5),
                     "loop_with_installs_over_values": round(mbi / ma, 3), "loop_searches_only_over_values": round(mb / ma, 3),
                     "reps_values": [round(x, 5) for x in ta]}
                if not k:
                    r["results"] = results
                    r["reorder_s"] = round(statistics.median(reorder[args.warmup:]), 5)
                    r["reorder_share"] = round(r["reorder_s"] / ma, 4)
                result["rows"].append(r)
                print(json.dumps(r), flush=True)
            del sub
        g.clear_base_values()

    def f16_range_splits(n, dd):
        """exact_range_f16_splits_for (capi_base_f16.cpp) restated: the split count an nq-query call gets by the rule."""
        blocks, resident = -(-min(nq, 16384) // 128), 256 * max(1, min(2, (160 << 10) // (64 * (2 * dd + 16))))
        cost = [None] + [-(-blocks * s // resident) / s for s in range(1, min(64, max(1, -(-n // 4096))) + 1)]
        return next(s for s in range(1, len(cost)) if cost[s] <= 1.05 * min(cost[1:]))

    def f16_range_legs(n, dd, qf, d10, d100):
        """The float16 range search at each radius beside the k = 1 f16 sweep, the three alternating rep by rep."""
        od, ol = torch.empty((nq, 1), dtype=torch.float32, device=dev), torch.empty((nq, 1), dtype=torch.int64, device=dev)
        r10, r100 = float(d10.median()), float(d100.median())
        rule = f16_range_splits(n, dd)
        legs = [(what, radius, -1) for what, radius in (("k=10 distance", r10), ("k=100 distance", r100), ("one step beyond", 2 * r100 - r10))]
        legs += [("k=100 distance", r100, s) for s in (rule - 1, rule, rule + 1) if 1 <= s <= 64]
        for what, radius, splits in legs:
            ts, st, total = {"sweep": [], 1: [], 0: []}, {}, 0
            for rep_i in range(args.warmup + args.reps):
                for which in ("sweep", 1, 0):
                    g.set_option("exact_splits", -1 if which == "sweep" else splits)
                    g.set_option("exact_range_map", -1 if which == "sweep" else which)
                    g.set_profiling(which != "sweep" and rep_i >= args.warmup)
                    g.reset_stage_ms()
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    if which == "sweep":
                        g.exact_search_f16_dev(nq, qf, dd, 1, od, ol)
                    else:
                        total = g.exact_range_search_f16_dev(nq, qf, dd, radius, lims)
                    torch.cuda.synchronize(dev)
                    if rep_i >= args.warmup:
                        ts[which].append(time.perf_counter() - t0)
                        if which != "sweep":
                            ms = g.stage_ms()
                            st.setdefault(which, []).append((ms["scan"][0] / 1e3, ms["select"][0] / 1e3))
            g.set_profiling(False)
            k1 = statistics.median(ts["sweep"])
            for use_map in (1, 0):
                t = statistics.median(ts[use_map])
                r = {"what": "exact_range_search_f16_dev", "rows": n, "d": dd, "nq": nq, "radius": what, "radius_value": radius,
                     "splits": splits if splits > 0 else rule, "splits_by_rule": splits < 0, "tile_map": bool(use_map), "results": total,
                     "results_per_query": round(total / nq, 2), "seconds": round(t, 5), "reps": [round(x, 5) for x in ts[use_map]],
                     "count_pass_s": round(statistics.median(a for a, _ in st[use_map]), 5),
                     "fill_pass_s": round(statistics.median(b for _, b in st[use_map]), 5), "k1_sweep_s": round(k1, 5),
                     "k1_sweep_reps": [round(x, 5) for x in ts["sweep"]]}
                for key in ("seconds", "count_pass_s", "fill_pass_s"):
                    r[key.replace("_s", "").replace("seconds", "total") + "_over_k1"] = round(r[key] / k1, 3)
                result["rows"].append(r)
                print(json.dumps(r), flush=True)
        g.set_option("exact_splits", -1)
        g.set_option("exact_range_map", -1)

    def alternate(calls, what):
        """{name: seconds of every timed rep} of calls [(name, fn)] run in turn, rep by rep"""
        ts = {name: [] for name, _ in calls}
        for rep in range(args.warmup + args.reps):
            for name, fn in calls:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                if rep >= args.warmup:
                    ts[name].append(time.perf_counter() - t0)
                log("[exact_bench] f16 %s rep %d %s: %.4f s" % (what, rep, name, time.perf_counter() - t0))
        return ts

    def f16_values_legs(n, dd, g8, qf, qb):
        """Base values on the float16 store (exact_search_f16_values_dev) on the rows f16_legs uploaded to both
        stores: values_legs' three workloads over a permutation of 0..n-1, k = 1 and 100, the call ALTERNATING with
        exact_search_values_dev on the uint8 store (the two must agree); then the all-FULL batch beside the plain
        exact_search_f16_dev, its plan stage (plan and gather) from the stage profiler."""
        gen = torch.Generator(device=dev)
        gen.manual_seed(8100)
        values = torch.randperm(n, device=dev, generator=gen).to(torch.int32)
        rows_i = torch.arange(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        g.set_base_values_dev(n, rows_i, values)
        g8.set_base_values_dev(n, rows_i, values)

        def spread(count, width):
            return [(a, a + width - 1) for a in ((i * (n - width)) // max(1, count - 1) for i in range(count))]
        workloads = [("897 x 1/8", spread(897, n // 8), 0), ("1000 x ~100 rows", spread(1000, min(n, 100)), 0),
                     ("1000 x ~100 rows, 1/33 full", spread(1000, min(n, 100)), 33), ("all full", [(0, 0xffffffff)], 0)]
        for wname, ivs, full_share in workloads:
            pick = (torch.arange(nq, device=dev) % len(ivs))[torch.randperm(nq, device=dev, generator=gen)]
            qr64 = torch.tensor(ivs, dtype=torch.int64, device=dev)[pick]
            if full_share:
                qr64[torch.arange(nq, device=dev) % full_share == full_share - 1] = torch.tensor((0, 0xffffffff), dtype=torch.int64, device=dev)
            qr = torch.where(qr64 >= 2 ** 31, qr64 - 2 ** 32, qr64).to(torch.int32).contiguous()  # the bit pattern of the uint32
            for k in (1, 100):
                od = torch.empty((nq, k), dtype=torch.float32, device=dev)
                ol = torch.empty((nq, k), dtype=torch.int64, device=dev)
                od8, ol8 = torch.empty_like(od), torch.empty_like(ol)
                plan_ms = []

                def valued():
                    g.set_profiling(True)
                    g.reset_stage_ms()
                    g.exact_search_f16_values_dev(nq, qf, dd, k, qr, od, ol)
                    torch.cuda.synchronize(dev)
                    plan_ms.append(g.stage_ms()["plan"][0])
                    g.set_profiling(False)

                if wname == "all full":
                    other = ("exact_search_f16_dev", lambda: g.exact_search_f16_dev(nq, qf, dd, k, od8, ol8))
                else:
                    other = ("exact_search_values_dev (uint8 store)", lambda: g8.exact_search_values_dev(nq, qb, dd, k, qr, od8, ol8))
                ts = alternate([("exact_search_f16_values_dev", valued), other], "values '%s' k=%d" % (wname, k))
                assert torch.equal(ol, ol8) and torch.equal(od, od8), "exact_search_f16_values_dev and %s disagree" % other[0]
                a, b = ts["exact_search_f16_values_dev"], ts[other[0]]
                r = {"what": "exact_search_f16_values_dev", "beside": other[0], "rows": n, "d": dd, "nq": nq, "k": k, "workload": wname,
                     "seconds": round(statistics.median(a), 5), "reps": [round(x, 5) for x in a],
                     "beside_seconds": round(statistics.median(b), 5), "beside_reps": [round(x, 5) for x in b],
                     "plan_and_gather_ms": round(statistics.median(plan_ms[args.warmup:]), 4)}
                result["rows"].append(r)
                print(json.dumps(r), flush=True)
            # (od: the k = 100 distances under the intervals) a radius that gives some tens of hits per query
            f16_values_range_leg(n, dd, g8, qf, qb, qr, wname, float(od[:, 29][od[:, 29] < 3e38].median()))
        g.clear_base_values()
        g8.clear_base_values()

    def f16_values_range_leg(n, dd, g8, qf, qb, qr, wname, radius):
        """The range form under base values (exact_range_search_f16_values_dev) on one workload of
        f16_values_legs: beside exact_range_search_values_dev of the uint8 store (equal lims, labels and distances required),
        the k = 1 search under the same intervals, the call without the tile map and under the neighbours of the windowed
        launch's split count; plan (with the reorder), count and fill by the stage profiler.  "all full": beside the plain
        exact_range_search_f16_dev."""
        od, ol = torch.empty((nq, 1), dtype=torch.float32, device=dev), torch.empty((nq, 1), dtype=torch.int64, device=dev)
        lims8, passes = torch.zeros_like(lims), []
        name = "exact_range_search_f16_values_dev"

        def valued():
            g.set_profiling(True)
            g.reset_stage_ms()
            valued.total = g.exact_range_search_f16_values_dev(nq, qf, dd, qr, radius, lims)
            ms = g.stage_ms()
            passes.append((ms["plan"][0], ms["scan"][0], ms["select"][0]))
            g.set_profiling(False)

        def with_option(key, value):
            g.set_option(key, value)
            g.exact_range_search_f16_values_dev(nq, qf, dd, qr, radius, lims)
            g.set_option(key, -1)

        if wname == "all full":
            calls = [(name, valued), ("exact_range_search_f16_dev", lambda: g.exact_range_search_f16_dev(nq, qf, dd, radius, lims8))]
        else:
            # the rule of the windowed launch (capi_base_f16.cpp exact_range_f16_window_splits_for), restated
            blocks = -(-(min(nq, 16384) // 32 + 2) * 32 // 128)
            rule = max(1, min(64, 512 // blocks, -(-n // 4096)))
            calls = [(name, valued),
                     ("exact_range_search_values_dev (uint8 store)", lambda: g8.exact_range_search_values_dev(nq, qb, dd, qr, radius, lims8)),
                     ("exact_search_f16_values_dev k=1", lambda: g.exact_search_f16_values_dev(nq, qf, dd, 1, qr, od, ol)),
                     (name + ", no tile map", lambda: with_option("exact_range_map", 0))]
            calls += [(name + ", %d splits" % s, lambda s=s: with_option("exact_splits", s)) for s in (rule - 1, rule + 1) if 1 <= s <= 64]
        ts = alternate(calls, "range values '%s'" % wname)
        other = g if wname == "all full" else g8
        calls[1][1]()
        want = other.exact_range_results(0, int(lims8[-1]))
        valued()
        got = g.exact_range_results(0, valued.total)
        assert torch.equal(lims, lims8) and (got[1] == want[1]).all() and (got[0] == want[0]).all(), \
            "the float16 range search under values and %s disagree" % calls[1][0]
        base_t = statistics.median(ts[name])
        for what, _ in calls:
            t = statistics.median(ts[what])
            r = {"what": what, "rows": n, "d": dd, "nq": nq, "workload": wname, "radius_value": radius, "results": valued.total,
                 "results_per_query": round(valued.total / nq, 2), "seconds": round(t, 5), "reps": [round(x, 5) for x in ts[what]],
                 "over_f16_range_values": round(t / base_t, 3)}
            if what == name:
                mine = passes[args.warmup:][:args.reps]
                for i, key in enumerate(("plan_gather_reorder_ms", "count_pass_ms", "fill_pass_ms")):
                    r[key] = round(statistics.median(x[i] for x in mine), 4)
            result["rows"].append(r)
            print(json.dumps(r), flush=True)

    def f16_tags_range_leg(n, dd, g8, qf, qb, qt, ntags, radius, alternate, with_splits):
        """The range form under base tags (exact_range_search_f16_tags_dev) at the radius of the tagged 10th
        neighbour: beside exact_range_search_tags_dev of the uint8 store (equal results required), the tagged k = 1 sweep,
        the call without the tile map and under the neighbours of the Indirect launch's split count; the count and the fill
        pass by the stage profiler.  qt None: the all-NONE batch beside the plain exact_range_search_f16_dev."""
        od, ol = torch.empty((nq, 1), dtype=torch.float32, device=dev), torch.empty((nq, 1), dtype=torch.int64, device=dev)
        lims8, passes = torch.zeros_like(lims), []
        tags = qt if qt is not None else torch.full((nq,), -1, dtype=torch.int16, device=dev)

        def tagged():
            g.set_profiling(True)
            g.reset_stage_ms()
            tagged.total = g.exact_range_search_f16_tags_dev(nq, qf, dd, tags, radius, lims)
            ms = g.stage_ms()
            passes.append((ms["plan"][0], ms["scan"][0], ms["select"][0]))
            g.set_profiling(False)

        def no_map():
            g.set_option("exact_range_map", 0)
            g.exact_range_search_f16_tags_dev(nq, qf, dd, tags, radius, lims)
            g.set_option("exact_range_map", -1)

        if qt is None:
            calls = [("exact_range_search_f16_tags_dev, all NONE", tagged),
                     ("exact_range_search_f16_dev", lambda: g.exact_range_search_f16_dev(nq, qf, dd, radius, lims8))]
        else:
            # the rule of the Indirect launch (capi_base_f16.cpp exact_range_f16_tags_dev), restated
            blocks, longest = -(-(nq // 32 + min(nq, ntags + 1)) * 32 // 128), -(-n // ntags)
            rule = max(1, min(64, -(-512 // blocks), -(-longest // 4096)))
            calls = [("exact_range_search_f16_tags_dev", tagged),
                     ("exact_range_search_tags_dev (uint8 store)", lambda: g8.exact_range_search_tags_dev(nq, qb, dd, tags, radius, lims8)),
                     ("exact_search_f16_tags_dev k=1", lambda: g.exact_search_f16_tags_dev(nq, qf, dd, 1, tags, od, ol)),
                     ("exact_range_search_f16_tags_dev, no tile map", no_map)]
            calls += [("exact_range_search_f16_tags_dev, %d splits" % s, lambda s=s: with_splits(s, tagged))
                      for s in (rule - 1, rule + 1) if 1 <= s <= 64]
        ts = alternate(calls, "range %s" % (ntags if qt is not None else "all NONE"))
        other = g8 if qt is not None else g
        calls[1][1]()
        want = other.exact_range_results(0, int(lims8[-1]))
        tagged()
        got = g.exact_range_results(0, tagged.total)
        assert torch.equal(lims, lims8) and (got[1] == want[1]).all() and (got[0] == want[0]).all(), \
            "the tagged float16 range search and %s disagree" % calls[1][0]
        base_t = statistics.median(ts[calls[0][0]])
        for name, _ in calls:
            t = statistics.median(ts[name])
            r = {"what": name, "rows": n, "d": dd, "nq": nq, "tags": ntags, "radius_value": radius, "results": tagged.total,
                 "seconds": round(t, 5), "reps": [round(x, 5) for x in ts[name]], "over_f16_range_tags": round(t / base_t, 3)}
            if name == calls[0][0]:
                per_rep = sum(1 for other, fn in calls if fn is tagged or "splits" in other)  # the profiled calls of a rep
                mine = passes[args.warmup * per_rep:][::per_rep][:args.reps]
                for i, key in enumerate(("plan_and_gather_ms", "count_pass_ms", "fill_pass_ms")):
                    r[key] = round(statistics.median(x[i] for x in mine), 4)
            result["rows"].append(r)
            print(json.dumps(r), flush=True)

    def f16_tags_legs(n, dd, g8, qf, qb):
        """Base tags on the float16 store (exact_search_f16_tags_dev) on the rows f16_legs uploaded to both
        stores, the calls of a leg alternating rep by rep in one process.  Per tag count (row i carries tag i % ntags, query
        q asks for q % ntags) and k: the tagged call under the rule's split count and under its neighbours beside
        exact_search_tags_dev on the uint8 store; then the all-NONE batch beside the plain exact_search_f16_dev, with the
        plan stage (the plan and the gather) timed by the stage profiler."""
        def with_splits(s, fn):
            g.set_option("exact_splits", s)
            fn()
            g.set_option("exact_splits", -1)

        for ntags in (32, 1024):
            btags = (torch.arange(n, device=dev, dtype=torch.int32) % ntags).to(torch.int16)
            rows_i = torch.arange(n, device=dev, dtype=torch.int32)
            qt = (torch.arange(nq, device=dev, dtype=torch.int32) % ntags).to(torch.int16)
            torch.cuda.synchronize(dev)
            g.set_base_tags_dev(n, rows_i, btags)
            g8.set_base_tags_dev(n, rows_i, btags)
            for k in (1, 100):
                od = torch.empty((nq, k), dtype=torch.float32, device=dev)
                ol = torch.empty((nq, k), dtype=torch.int64, device=dev)
                od8, ol8 = torch.empty_like(od), torch.empty_like(ol)
                # the rule of the Indirect launch (capi_base_f16.cpp exact_f16_tag_splits), restated
                bound, rpb = nq // 32 + min(nq, ntags + 1), 128 if k <= 32 else 64
                blocks, longest = -(-bound * 32 // rpb), -(-n // ntags)
                rule = max(1, min(64, -(-512 // blocks), -(-longest // 4096)))
                tagged = lambda: g.exact_search_f16_tags_dev(nq, qf, dd, k, qt, od, ol)
                calls = [("exact_search_f16_tags_dev", tagged),
                         ("exact_search_tags_dev (uint8 store)", lambda: g8.exact_search_tags_dev(nq, qb, dd, k, qt, od8, ol8))]
                calls += [("exact_search_f16_tags_dev, %d splits" % s, lambda s=s: with_splits(s, tagged))
                          for s in (rule - 1, rule + 1) if 1 <= s <= 64]
                ts = alternate(calls, "%d tags k=%d" % (ntags, k))
                tagged()
                torch.cuda.synchronize(dev)
                assert torch.equal(ol, ol8) and torch.equal(od, od8), "the float16 and the uint8 tagged sweep disagree on integer rows"
                base_t = statistics.median(ts["exact_search_f16_tags_dev"])
                for name, _ in calls:
                    t = statistics.median(ts[name])
                    r = {"what": name, "rows": n, "d": dd, "nq": nq, "k": k, "tags": ntags, "rule_splits": rule, "seconds": round(t, 5),
                         "reps": [round(x, 5) for x in ts[name]], "over_f16_tags": round(t / base_t, 3)}
                    result["rows"].append(r)
                    print(json.dumps(r), flush=True)
            f16_tags_range_leg(n, dd, g8, qf, qb, qt, ntags, float(od[:, 9].median()), alternate, with_splits)
        none = torch.full((nq,), -1, dtype=torch.int16, device=dev)  # 0xffff: every query untagged
        for k in (1, 100):
            od = torch.empty((nq, k), dtype=torch.float32, device=dev)
            ol = torch.empty((nq, k), dtype=torch.int64, device=dev)
            odp, olp = torch.empty_like(od), torch.empty_like(ol)
            plan_ms = []

            def all_none():
                g.set_profiling(True)
                g.reset_stage_ms()
                g.exact_search_f16_tags_dev(nq, qf, dd, k, none, od, ol)
                torch.cuda.synchronize(dev)
                plan_ms.append(g.stage_ms()["plan"][0])
                g.set_profiling(False)

            ts = alternate([("exact_search_f16_tags_dev, all NONE", all_none),
                            ("exact_search_f16_dev", lambda: g.exact_search_f16_dev(nq, qf, dd, k, odp, olp))], "all NONE k=%d" % k)
            assert torch.equal(ol, olp) and torch.equal(od, odp), "the all-NONE batch and the plain call disagree"
            a, b = ts["exact_search_f16_tags_dev, all NONE"], ts["exact_search_f16_dev"]
            r = {"what": "all NONE beside the plain call", "rows": n, "d": dd, "nq": nq, "k": k, "all_none_seconds": round(statistics.median(a), 5),
                 "plain_seconds": round(statistics.median(b), 5), "plain_span": [round(min(b), 5), round(max(b), 5)],
                 "all_none_reps": [round(x, 5) for x in a], "plan_and_gather_ms": round(statistics.median(plan_ms[args.warmup:]), 4)}
            result["rows"].append(r)
            print(json.dumps(r), flush=True)
        f16_tags_range_leg(n, dd, g8, qf, qb, None, 0, float(odp[:, 9].median()), alternate, with_splits)
        g.clear_base_tags()

    def f16_tags_values_legs(n, dd, qf):
        """A tag AND an interval per query on the float16 store (exact_search_f16_tags_values_dev), the calls
        of a leg alternating rep by rep in one process.  Per tag count (row i carries tag i % ntags, query q asks for
        q % ntags) and k: intervals of 1/8 of each tag's rows under values that ascend with the row number (timestamps: most
        tiles of a list are dead) and under the same values shuffled (none is), each beside exact_search_f16_tags_dev on the
        same tags -- the same sweep without the gate; then the all-whole tagged batch beside that call, and the
        all-(NONE, whole) batch beside the plain one."""
        rows_i = torch.arange(n, device=dev, dtype=torch.int32)
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        layouts = {"ascending": rows_i.clone(), "shuffled": torch.randperm(n, device=dev, generator=gen).to(torch.int32)}
        whole = torch.tensor([0, -1], dtype=torch.int32, device=dev).repeat(nq, 1)  # (0, 0xffffffff)
        lo = ((torch.arange(nq, device=dev, dtype=torch.int64) * 7919) % (n - n // 8)).to(torch.int32)
        eighth = torch.stack([lo, lo + n // 8 - 1], 1).contiguous()  # values are 0 .. n - 1: an eighth of every tag's rows
        for ntags in (32, 1024):
            g.set_base_tags_dev(n, rows_i, (rows_i % ntags).to(torch.int16))
            qt = (torch.arange(nq, device=dev, dtype=torch.int32) % ntags).to(torch.int16)
            for k in (1, 100):
                od, ol = torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)
                odt, olt = torch.empty_like(od), torch.empty_like(ol)
                tags_only = ("exact_search_f16_tags_dev", lambda: g.exact_search_f16_tags_dev(nq, qf, dd, k, qt, odt, olt))
                for lname, values in layouts.items():
                    g.set_base_values_dev(n, rows_i, values)
                    for wname, qr in (("an eighth", eighth), ("whole", whole)):
                        if wname == "whole" and lname == "shuffled":
                            continue
                        both = ("exact_search_f16_tags_values_dev", lambda: g.exact_search_f16_tags_values_dev(nq, qf, dd, k, qt, qr, od, ol))
                        ts = alternate([both, tags_only], "%d tags k=%d %s %s" % (ntags, k, lname, wname))
                        if wname == "whole":
                            assert torch.equal(ol, olt) and torch.equal(od, odt), "the all-whole batch and the _tags call disagree"
                        a, b = ts[both[0]], ts[tags_only[0]]
                        r = {"what": both[0], "beside": tags_only[0], "rows": n, "d": dd, "nq": nq, "k": k, "tags": ntags, "values": lname,
                             "intervals": wname, "seconds": round(statistics.median(a), 5), "reps": [round(x, 5) for x in a],
                             "beside_seconds": round(statistics.median(b), 5), "beside_span": [round(min(b), 5), round(max(b), 5)],
                             "ratio": round(statistics.median(a) / statistics.median(b), 3)}
                        result["rows"].append(r)
                        print(json.dumps(r), flush=True)
        none = torch.full((nq,), -1, dtype=torch.int16, device=dev)  # 0xffff: every query untagged
        for k in (1, 100):
            od, ol = torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)
            odp, olp = torch.empty_like(od), torch.empty_like(ol)
            ts = alternate([("all (NONE, whole)", lambda: g.exact_search_f16_tags_values_dev(nq, qf, dd, k, none, whole, od, ol)),
                            ("exact_search_f16_dev", lambda: g.exact_search_f16_dev(nq, qf, dd, k, odp, olp))], "all (NONE, whole) k=%d" % k)
            assert torch.equal(ol, olp) and torch.equal(od, odp), "the all-(NONE, whole) batch and the plain call disagree"
            a, b = ts["all (NONE, whole)"], ts["exact_search_f16_dev"]
            r = {"what": "all (NONE, whole) beside the plain call", "rows": n, "d": dd, "nq": nq, "k": k, "seconds": round(statistics.median(a), 5),
                 "reps": [round(x, 5) for x in a], "plain_seconds": round(statistics.median(b), 5), "plain_span": [round(min(b), 5), round(max(b), 5)]}
            result["rows"].append(r)
            print(json.dumps(r), flush=True)
        g.clear_base_tags()
        g.clear_base_values()

    def f16_legs(n, dd):
        """The float16 store's sweep (exact_search_f16_dev) beside knn_dev on the same rows as float32 and
        exact_search_dev on a uint8 store of the same rows, alternating in one process.  The rows are random bytes, so all
        three are exact and must return the same labels."""
        g8 = pkg.GpuIndex(0)
        g8.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        gen = torch.Generator(device=dev)
        gen.manual_seed(77 + dd)
        rows = torch.empty((n, dd), dtype=torch.uint8, device=dev).random_(0, 256, generator=gen)
        qb = torch.empty((nq, dd), dtype=torch.uint8, device=dev).random_(0, 256, generator=gen)
        xf, qf = rows.to(torch.float32), qb.to(torch.float32)
        torch.cuda.synchronize(dev)
        g8.upload_base_dev(n, dd, 0, n, rows)
        t0 = time.perf_counter()
        g.upload_base_f16_dev(n, dd, 0, n, xf)
        t_up = time.perf_counter() - t0
        r = {"what": "upload_base_f16_dev", "rows": n, "d": dd, "seconds": round(t_up, 4), "memory_GB": round(g.memory_bytes() / 1e9, 3)}
        result["rows"].append(r)
        print(json.dumps(r), flush=True)
        kth = {}
        for k in (1, 10, 100):
            od = torch.empty((nq, k), dtype=torch.float32, device=dev)
            ol = torch.empty((nq, k), dtype=torch.int64, device=dev)
            od8, ol8 = torch.empty_like(od), torch.empty_like(ol)
            ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
            kd = torch.empty((nq, k), dtype=torch.float32, device=dev)
            calls = [("exact_search_f16_dev", lambda: g.exact_search_f16_dev(nq, qf, dd, k, od, ol)),
                     ("exact_search_dev (uint8 store)", lambda: g8.exact_search_dev(nq, qb, dd, k, od8, ol8))]
            if k <= 80 and not args.no_knn:  # knn_dev's limit
                calls.append(("knn_dev (f32 MFMA)", lambda: g.knn_dev(nq, n, dd, qf, xf, k, ids, kd)))
            ts = {name: [] for name, _ in calls}
            for rep in range(args.warmup + args.reps):
                for name, fn in calls:
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize(dev)
                    if rep >= args.warmup:
                        ts[name].append(time.perf_counter() - t0)
                    log("[exact_bench] f16 legs d=%d k=%d rep %d %s: %.4f s" % (dd, k, rep, name, time.perf_counter() - t0))
            assert torch.equal(ol, ol8) and torch.equal(od, od8), "the float16 and the uint8 sweep disagree on integer rows"
            base_t = statistics.median(ts["exact_search_f16_dev"])
            for name, _ in calls:
                t = statistics.median(ts[name])
                r = figures(name, n, dd, nq, k, t, ts[name], 128 if k <= 32 else 64)
                elem = {"exact_search_f16_dev": 2, "knn_dev (f32 MFMA)": 4}.get(name, 1)
                r["store_TB_per_s_per_pass"] = round(n * dd * elem / t / 1e12, 4)  # bytes of THIS call's rows
                r["streamed_TB_per_s"] = round(r["query_tiles"] * n * dd * elem / t / 1e12, 3)
                r["over_f16"] = round(t / base_t, 3)
                if name.startswith("knn"):
                    r["labels_equal"] = bool(torch.equal(ids.to(torch.int64) & 0xffffffff, ol))
                result["rows"].append(r)
                print(json.dumps(r), flush=True)
            kth[k] = od[:, k - 1].clone()
        if args.tags and dd == 128:
            f16_tags_legs(n, dd, g8, qf, qb)
        if args.values and dd == 128:
            f16_values_legs(n, dd, g8, qf, qb)
        if args.tags_values and dd == 128:
            f16_tags_values_legs(n, dd, qf)
        g8.close()
        if args.range:
            f16_range_legs(n, dd, qf, kth[10], kth[100])
        g.upload_base_f16_dev(0, dd, 0, 0, None)
        del rows, xf, qf, qb
        torch.cuda.empty_cache()

    if args.f16:
        for dd in (128, 96):
            f16_legs(args.small_rows, dd)
        g.close()
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
        return

    def yardstick_and_range(n, dense_radius=None, fractions=(1, 2, 8, 32, 1024)):
        name = "%d rows" % n
        r1, _, _ = exact(n, 1, name)
        r100, _, od100 = exact(n, 100, name)
        if args.filter:
            filter_legs(n, name, {1: r1["seconds"], 100: r100["seconds"]}, fractions)
        if args.filter_slots:
            slots_legs(n, name, od100[:, 9])
        if args.tags:
            for ntags in (32, 1024):
                tags_legs(n, name, od100[:, 9], ntags)
        if args.values:
            values_legs(n, name, od100[:, 9])
        if not args.no_range:
            range_legs(n, name, r1["seconds"], od100[:, 9], od100[:, 99], dense_radius)

    if not args.no_small:
        n = args.small_rows
        rows = fill_store(g, torch, dev, n, d, 99, keep=True)
        # the median distance of the store, from a sample: the dense radius
        sample = (q[:32].to(torch.float32)[:, None, :] - rows[:20_000].to(torch.float32)[None, :, :]).square_().sum(-1)
        dense_radius = float(sample.median())
        del sample
        if not args.no_knn:
            xf = rows.to(torch.float32)
            qf = q.to(torch.float32)
            for k in (1, 10):
                r, ol, _ = exact(n, k, "%d rows" % n)
                ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
                dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
                t, ts = timed(torch, dev, lambda: g.knn_dev(nq, n, d, qf, xf, k, ids, dist), args.warmup, args.reps,
                              "%d rows knn k=%d" % (n, k))
                rk = figures("knn_dev (f32 MFMA)", n, d, nq, k, t, ts)
                rk["labels_equal"] = bool(torch.equal(ids.to(torch.int64) & 0xffffffff, ol))
                rk["exact_speedup"] = round(t / r["seconds"], 2)
                result["rows"].append(rk)
                print(json.dumps(rk), flush=True)
                assert rk["labels_equal"], "exact_search and knn disagree"
            del xf, qf
        del rows
        torch.cuda.empty_cache()
        yardstick_and_range(n, dense_radius)
    if not args.no_big:
        n = args.rows
        fill_store(g, torch, dev, n, d, 99)
        yardstick_and_range(n, fractions=(32, 1024))
    g.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
