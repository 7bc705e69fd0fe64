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
Each figure: warm-up runs, then the median of several repetitions, each timed from the call to the end of the stream's
work.  Reported: seconds, 2 nq n d / t in TOP/s, store bytes per second per pass (n d / t) and, with one pass per query
tile, the bytes per second all tiles stream together.
usage: python tools/exact_bench.py [--rows 1000000000] [--small-rows 10000000] [--nq 10000] [--reps 3] [--warmup 1]
                                   [--no-big] [--no-small] [--no-knn] [--no-range] [--filter] [--filter-slots] [--tags] [--values]
                                   [--dense-nq 512]
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
