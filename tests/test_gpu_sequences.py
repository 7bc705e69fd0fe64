"""One long-lived handle through seeded schedules of interleaved updates, filter changes, knobs, refused calls and every
kind of query (tests/index_model.py).  After every update the handle's lists equal the host model's byte for byte; every
answer equals the oracle's on the model's state in labels and distance bits; at the middle and at the end a fresh handle
that uploads the model's state answers a fixed probe set with the same bits.  A failure names the flavour, the seed, the
step and the kinds of all steps so far: index_model.schedule(flavour, seed)[:step + 1] replays the failing prefix."""
import time

import numpy as np
import pytest

import index_model as im
import range_ref
import recon_ref
from index_model import EF, FLT_MAX, MAX_CODES, NPROBE
from test_gpu_filter import tiled
from test_gpu_remove import _upload

pytestmark = pytest.mark.gpu

CASES = [(f, s) for f in im.FLAVOURS for s in im.SEEDS]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(view)).to(torch.device("cuda", 0))


def upload_state(g, m):
    """Everything the model holds onto the handle g: lists, Grouping tables, quantizer, code books, filter, base store."""
    c = m.c
    _upload(g, c)
    g.upload_codebooks(c["d"], c["code_size"], c["pq_centroids"], c["norm_table"], c["opq_A"])
    if m.filter is not None:
        g.set_filter(*m.filter)
    if m.base is not None:
        g.upload_base(m.base)
        if m.base_filter is not None:
            g.set_base_filter(*m.base_filter)
    return g


def run_search(h, q, k, max_codes, pruning=False, heap=False, dev=False, coarse=None):
    kw = dict(efSearch=EF, do_pruning=pruning, heap_order=heap)
    if coarse is not None:
        kw = dict(coarse_ids=coarse[0], coarse_dists=coarse[1], do_pruning=pruning, heap_order=heap)
    if not dev:
        return h.search(q, k, NPROBE, max_codes, **kw)
    import torch
    d_q = _dev(q)
    d = torch.empty((len(q), k), dtype=torch.float32, device=d_q.device)
    lab = torch.empty((len(q), k), dtype=torch.int64, device=d_q.device)
    torch.cuda.synchronize(d_q.device)   # the handle's stream is not torch's
    h.search_dev(len(q), k, d_q, d, lab, NPROBE, max_codes, efSearch=EF, do_pruning=pruning, heap_order=heap)
    h.sync()
    return d.cpu().numpy(), lab.cpu().numpy()


def check_kernel(h, m):
    name = h.last_scan_kernel()
    assert name.endswith("+filter") == (m.filter is not None), name
    if name.startswith(("scan_k1_kernel", "range_scan_kernel")):   # the forms that are compiled per code size
        assert ("(run-time code size)" in name) == (m.M not in (8, 16, 32)), name


def check_search(h, m, q, k, max_codes=MAX_CODES, pruning=False, heap=False, dev=False, coarse=False, kernel=True):
    ref = m.expect_search(q, k, max_codes=max_codes, pruning=pruning)
    got = run_search(h, q, k, max_codes, pruning, heap, dev, ref[2:4] if coarse else None)
    ref_d, ref_l = ref[0].reshape(got[0].shape), ref[1].reshape(got[1].shape)
    if k == 1 or heap:       # faiss's heap array, element for element
        assert np.array_equal(got[1], ref_l), "labels"
        assert np.array_equal(bits(got[0]), bits(ref_d)), "distance bits"
    else:                    # ascending: the same k results, as tests/test_gpu_topk.py compares them
        assert np.array_equal(bits(got[0]), bits(np.sort(ref_d, axis=1))), "distance bits"
        assert np.array_equal(np.sort(got[1], axis=1), np.sort(ref_l, axis=1)), "labels"
    if k == 1:
        assert h.last_scan_counts()[0] == ref[4].ncode, "codes scored"
    if kernel and m.n:
        check_kernel(h, m)
    return got


def check_range(h, m, q, radius, max_codes, pruning):
    form, want, sc = m.expect_range(q, radius, max_codes=max_codes, pruning=pruning)
    lims, dist, lab = h.range_search(q, radius, NPROBE, max_codes, efSearch=EF, do_pruning=pruning)
    assert h.last_scan_counts()[0] == sc["ncode"].sum(), "codes scored"
    check_kernel(h, m)
    total = int(lims[-1])
    assert len(dist) == len(lab) == total
    a, b = h.range_results(0, total // 2), h.range_results(total // 2, total - total // 2)     # the results in two pieces
    assert np.array_equal(np.concatenate([a[1], b[1]]), lab) and np.array_equal(bits(np.concatenate([a[0], b[0]])), bits(dist))
    if form == "ivf":      # lims, labels in scan order, distance bits
        assert range_ref.same_range((lims, dist, lab), want), "range result"
    else:
        assert lims[0] == 0 and (np.diff(lims.astype(np.int64)) >= 0).all()
        for i in range(len(q)):
            assert np.array_equal(range_ref.result_set(lims, dist, lab, i), want[i]), "range result of query %d" % i
    if not np.isfinite(radius) and m.filter is None:
        assert np.array_equal(np.diff(lims.astype(np.int64)), sc["ncode"])
    return lims, dist, lab


def check_state(g, m):
    got = g.download_ivf()
    for x, y, name in zip(got, m.csr(), ("offsets", "ids", "codes", "norm_codes")):
        assert np.array_equal(x, np.asarray(y).reshape(x.shape)), name
    if m.grouping:
        assert np.array_equal(g.download_grouping(), m.c["subgroup_sizes"]), "subgroup_sizes"
        for x, k in zip(g.download_grouping_tables(), ("alphas", "nn_centroid_idxs", "subgroup_sizes", "inter_centroid_dists")):
            assert np.array_equal(x.view(np.uint32), np.ascontiguousarray(m.c[k]).view(np.uint32).reshape(x.shape)), k
    assert g.filter_info() == m.filter_info(), "filter_info"


def refused(g, m, pkg, what):
    q = m.c["queries"][:4]
    with pytest.raises(pkg.IvfHnswError):
        if what == "ef_below_nprobe":
            g.search(q, 1, NPROBE, MAX_CODES, efSearch=NPROBE - 1)
        elif what == "nprobe_0":
            g.search(q, 1, 0, MAX_CODES, efSearch=EF)
        elif what == "one_coarse_array":
            g.search(q, 1, 8, 1000, coarse_ids=np.zeros((4, 8), np.uint32))
        elif what == "nan_radius":
            g.range_search(q, np.float32(np.nan), NPROBE, MAX_CODES, efSearch=EF)
        elif what == "bad_option":
            g.set_option("scan_pipe", 2)
        elif what == "append_bad_list":     # the host form checks the list numbers before anything is launched
            g.append_ivf(np.array([m.nc], np.uint32), np.array([7], np.uint32), np.zeros((1, m.M), np.uint8), np.zeros(1, np.uint8))
        else:
            assert what == "append_ivf_on_grouping"
            g.append_ivf(np.zeros(1, np.uint32), np.array([7], np.uint32), np.zeros((1, m.M), np.uint8), np.zeros(1, np.uint8))


def run_step(gpu, pkg, g, m, kind, a):
    c = m.c
    q48 = c["queries"]
    if kind in ("append_ivf", "append_grouping"):
        keys = ("list_idx",) + (("sub_idx",) if kind == "append_grouping" else ()) + ("ids", "codes", "norm_codes")
        if a.get("dev"):
            g.append_ivf_dev(len(a["ids"]), *[_dev(a[k]) for k in keys])
        else:
            getattr(g, kind)(*[a[k] for k in keys])
        im.apply(m, kind, a)
    elif kind == "add":
        got, want = g.add(a["x"], a["ids"], efSearch=EF), im.apply(m, kind, a)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), "what add returns"
    elif kind == "add_groups":
        off, x, ids = m.group_batch(a["which"])
        g.add_groups(a["which"].astype(np.uint32), off, x, ids, 80)
        im.apply(m, kind, a)
    elif kind in ("remove_ids", "empty_index"):
        n, per = g.remove_ids(a["labels"])
        want = im.apply(m, kind, a)
        assert n == want[0] and np.array_equal(per, want[1]), "what remove_ids returns"
        if kind == "empty_index":
            check_state(g, m)
            for k, heap in ((1, False), (10, True)):
                d, lab = check_search(g, m, q48[a["qi"]], k, heap=heap)
                assert (lab == -1).all() and (d == FLT_MAX).all()
            assert g.last_scan_counts()[0] == 0
    elif kind == "reupload":
        im.apply(m, kind, a)
        _upload(g, m.c)
        g.upload_codebooks(m.c["d"], m.M, m.c["pq_centroids"], m.c["norm_table"], m.c["opq_A"])
    elif kind in ("set_filter", "clear_filter"):
        g.set_filter(a["labels"], deny=a["deny"]) if kind == "set_filter" else g.clear_filter()
        im.apply(m, kind, a)
    elif kind == "prepare_latency":
        g.prepare_latency()
        im.apply(m, kind, a)
    elif kind == "set_batch_split":
        g.set_batch_split(a["permille"])
        im.apply(m, kind, a)
    elif kind == "scan_pipe":
        g.set_option("scan_pipe", a["value"])
    elif kind == "set_profiling":
        g.set_profiling(a["on"])
    elif kind == "refused":
        refused(g, m, pkg, a["what"])
    elif kind == "q1":
        check_search(g, m, q48[a["qi"]], 1, a["max_codes"], a["pruning"], dev=a["dev"], coarse=a["coarse"])
    elif kind == "ql":
        check_search(g, m, q48[a["qi"]], 1, MAX_CODES, a["pruning"])
    elif kind == "qk":
        check_search(g, m, q48[a["qi"]], a["k"], a["max_codes"], a["pruning"], heap=a["heap"])
    elif kind == "qr":
        check_range(g, m, q48[a["qi"]], a["radius"], a["max_codes"], a["pruning"])
    elif kind == "qx":
        rows, counts = g.locate(a["labels"])
        want = m.expect_locate(a["labels"])
        assert np.array_equal(rows, want[0]) and np.array_equal(counts, want[1]), "locate"
        rec, missing = g.reconstruct(a["labels"], pkg.RECON_ROTATED)
        want = m.expect_reconstruct(a["labels"])
        assert np.array_equal(bits(rec), bits(want[0])) and missing == want[1], "reconstruct"
        q, k = q48[a["qi"]], a["k"]
        ref = m.expect_search(q, k, pruning=a["pruning"])
        d, lab, rows, rec = g.search_reconstruct(q, k, NPROBE, MAX_CODES, efSearch=EF, do_pruning=a["pruning"], heap_order=True,
                                                 space=pkg.RECON_ROTATED)
        assert np.array_equal(lab, ref[1].reshape(lab.shape)) and np.array_equal(bits(d), bits(ref[0].reshape(d.shape)))
        filled = lab >= 0
        assert np.array_equal(rows >= 0, filled) and np.array_equal(c["ids"][rows[filled]].astype(np.int64), lab[filled])
        assert np.array_equal(bits(rec.reshape(-1, c["d"])), bits(recon_ref.recon_rotated(c, rows.ravel()))), "search_reconstruct"
    elif kind == "qb":
        small = m.expect_search(q48, 1, pruning=a["pruning"])
        idx = np.arange(a["n"]) % len(q48)
        got = run_search(g, tiled(q48, a["n"]), 1, MAX_CODES, a["pruning"], dev=True)
        if m.split:
            assert g.last_batch_parts()[1] > 0, "the batch did not take the two-part path"
        check_kernel(g, m)
        assert np.array_equal(got[1][:, 0], small[1].reshape(-1)[idx]) and np.array_equal(bits(got[0][:, 0]), bits(small[0]).reshape(-1)[idx])
    elif kind == "view":
        v = g.view()
        try:
            for h in (v, g):
                check_search(h, m, q48[a["qi"][:a["nq"]]], 1)
                check_range(h, m, q48[a["qi"]], a["radius"], a["max_codes"], a["pruning"])
        finally:
            v.close()
    # ---- the base store ----
    elif kind == "upload_base":
        g.upload_base(a["rows"], n=len(m.base), first=a["first"])
        im.apply(m, kind, a)
    elif kind in ("set_base_filter", "clear_base_filter"):
        g.set_base_filter(a["labels"], deny=a["deny"]) if kind == "set_base_filter" else g.clear_base_filter()
        im.apply(m, kind, a)
        assert g.base_filter_info() == m.base_filter_info()
    elif kind == "exact_option":
        g.set_option(a["key"], a["value"])
    elif kind == "exact_search":
        d, lab = g.exact_search(im.queries_u8(q48[a["qi"]]), a["k"])
        want = m.expect_exact(im.queries_u8(q48[a["qi"]]), a["k"])
        assert np.array_equal(lab, want[1]) and np.array_equal(bits(d), bits(want[0])), "exact_search"
    elif kind == "exact_range":
        qu = im.queries_u8(q48[a["qi"]])
        lims, d, lab = g.exact_range_search(qu, a["radius"])
        want = m.expect_exact_range(qu, a["radius"])
        assert range_ref.same_range((lims, d, lab), want), "exact_range_search"
        per = np.diff(lims.astype(np.int64))
        assert (per > 0).any() or m.base_mask().sum() == 0
        t = int(lims[-1])
        x, y = g.exact_range_results(0, t // 2), g.exact_range_results(t // 2, t - t // 2)
        assert np.array_equal(np.concatenate([x[1], y[1]]), lab) and np.array_equal(bits(np.concatenate([x[0], y[0]])), bits(d))
    elif kind == "rerank":
        q = q48[a["qi"]]
        _, cand = check_search(g, m, q, a["kc"])
        d, lab = g.rerank(q, cand, a["k"])
        want = m.expect_rerank(q, cand, a["k"])
        assert np.array_equal(lab, want[1]) and np.array_equal(bits(d), bits(want[0])), "rerank"
    elif kind == "search_rerank":
        q = q48[a["qi"]]
        cand = m.expect_search(q, a["kc"])[1].reshape(len(q), a["kc"])
        d, lab = g.search_rerank(q, a["k"], a["kc"], NPROBE, MAX_CODES, efSearch=EF)
        want = m.expect_rerank(q, cand, a["k"])
        assert np.array_equal(lab, want[1]) and np.array_equal(bits(d), bits(want[0])), "search_rerank"
    else:
        raise KeyError(kind)
    if kind in im.UPDATE_KINDS or kind in ("set_filter", "clear_filter"):
        check_state(g, m)


def probe(h, m, pkg, radius):
    """The fixed probe set: a list of (name, arrays..., counts)."""
    q = m.c["queries"]
    pruning = m.grouping
    out = []
    for name, qq, k, heap in (("Q1", q, 1, False), ("QL", q[:2], 1, False), ("QK", q, 10, True)):
        d, lab = h.search(qq, k, NPROBE, MAX_CODES, efSearch=EF, do_pruning=pruning, heap_order=heap)
        out.append((name, bits(d), lab, h.last_scan_counts()))
    lims, d, lab = h.range_search(q, radius, NPROBE, MAX_CODES, efSearch=EF, do_pruning=pruning)
    out.append(("QR", lims, bits(d), lab, h.last_scan_counts()))
    labels = np.concatenate([m.c["ids"][::97], m.removed[:50], [0xffffffff]]).astype(np.uint32)
    rows, counts = h.locate(labels)
    out.append(("locate", rows, counts))
    for space in (pkg.RECON_ROTATED, pkg.RECON_ORIGINAL):
        rec, missing = h.reconstruct(labels, space)
        out.append(("reconstruct", bits(rec), missing))
    if m.base is not None:
        qu = im.queries_u8(q)
        d, lab = h.exact_search(qu, 10)
        out.append(("exact_search", bits(d), lab))
        lims, d, lab = h.exact_range_search(qu, np.float32(np.quantile(d[:, -1], 0.5)))
        out.append(("exact_range", lims, bits(d), lab))
        d, lab = h.rerank(q, out[2][2], 5)
        out.append(("rerank", bits(d), lab))
    return out


def same_probe(a, b):
    for x, y in zip(a, b):
        for u, v in zip(x[1:], y[1:]):
            assert np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v, "probe %s differs" % x[0]


def against_fresh(gpu, pkg, g, m, view=False):
    """The long-lived handle and a fresh upload of the model's state answer the probe set with the same bits."""
    if not m.n:
        return
    radius = range_ref.pooled_quantile(m.scored(m.c["queries"], pruning=m.grouping), 0.1)
    f = upload_state(pkg.GpuIndex(0), m)
    try:
        check_state(f, m)
        want = probe(f, m, pkg, radius)
    finally:
        f.close()
    same_probe(probe(g, m, pkg, radius), want)
    if view:        # a view created last answers as its parent does, and as the oracle does
        v = g.view()
        try:
            same_probe(probe(v, m, pkg, radius), want)
            check_search(v, m, m.c["queries"], 1, pruning=m.grouping)
        finally:
            v.close()


@pytest.mark.parametrize("flavour,seed", CASES, ids=["%s-%d" % c for c in CASES])
def test_sequence(gpu, pkg, flavour, seed):
    t0 = time.time()
    steps = im.schedule(flavour, seed)
    t1 = time.time()
    m = im.IndexModel(flavour)
    g = upload_state(gpu(), m)
    i, kind = -1, "upload"
    try:
        check_state(g, m)
        for i, (kind, a) in enumerate(steps):
            run_step(gpu, pkg, g, m, kind, a)
            if i + 1 in (len(steps) // 2, len(steps)):
                kind = "probe set against a fresh handle"
                against_fresh(gpu, pkg, g, m, view=i + 1 == len(steps))
    except Exception as e:
        raise AssertionError("%s seed %d, step %d (%s): %s: %s\nsteps so far: %s" % (
            flavour, seed, i, kind, type(e).__name__, e, [k for k, _ in steps[:i + 1]])) from e
    finally:
        g.close()
    print("%s seed %d: %d steps, schedule built in %.2f s, run in %.2f s" % (flavour, seed, len(steps), t1 - t0, time.time() - t1))


def test_walk_scratch_serves_growing_and_shrinking_batches(gpu):
    """The walk's overflow bitmaps (w_visited) are the one piece of state the schedules above cannot reach: on their graphs
    of 96 and 128 nodes the LDS visited set never overflows.  Here one handle walks a graph of 20 000 nodes at efSearch 1024,
    where a query visits thousands of nodes and full buckets spill into the bitmaps, in calls of 3, 300, 8, 1200 and 3
    queries: the scratch is reallocated twice, and the small calls run inside what the large ones left.  Bar as for every
    walk: the ids and distance bits of the oracle's walk."""
    import synth
    from oracle import orc
    n, d, ef, k = 20000, 32, 1024, 16
    rng = np.random.default_rng(9)
    cents = synth.sift_like(rng, n, d)
    q = (cents[rng.choice(n, 1200)] + rng.normal(0, 12.0, size=(1200, d))).astype(np.float32)
    g = gpu()
    counts, links = g.build_graph(cents, 16, 32, 64)
    g.upload_quantizer(counts, links, cents, 0)
    graph = orc.Hnsw.from_arrays(counts, links, cents, 16, 0)
    try:
        for nq in (3, 300, 8, 1200, 3):
            ids, dist = g.coarse(q[:nq], k, ef)
            for i in np.unique(np.linspace(0, nq - 1, min(nq, 24)).astype(int)):
                rid, rd = graph.search_knn(q[i], ef, k)
                assert len(rid) == k and np.array_equal(ids[i], rid), "call of %d queries, query %d: ids differ" % (nq, i)
                assert np.array_equal(bits(dist[i]), bits(rd)), "call of %d queries, query %d: distances differ" % (nq, i)
    finally:
        graph.free()
