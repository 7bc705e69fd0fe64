"""Row tags: each query searches only the rows that carry its 16-bit tag (ivfhnsw_gpu_search_tags).

Expected values, both exact (labels and distance bits): (A) the oracle on the poisoned corpus of every tag (tags_ref),
(B) the single-filter path -- a second handle with set_filter(labels of the tag) and the plain call.  last_scan_kernel
proves that the tag form of the expected scan kernel ran, last_scan_counts that it scored what the plain call scores."""
import numpy as np
import pytest

import tags_ref as tr
from test_gpu_filter_slots import assert_same, base
from test_gpu_remove import BASE, CODE_SIZES, GROUPING, _upload, _same_search

pytestmark = pytest.mark.gpu

NPROBE, MAX_CODES, EF = tr.IVF_PARAMS
NONE, ABSENT = tr.NONE, tr.ABSENT


def handle_per_tag(f, b, asg, nq, k, call, tags=None):
    """{tag: (dist, labels)} from the single-filter path: call(f) -> (dist, labels) under set_filter(labels of the tag)."""
    out = {}
    for t in sorted({int(t) for t in (tr.PATTERN if tags is None else tags)}):
        if t == NONE:
            f.clear_filter()
        else:
            f.set_filter(tr.labels_of(asg, t))  # (a tag no label carries: the empty allow set)
        r = call(f)
        out[t] = (r[0].reshape(nq, k), r[1].reshape(nq, k))
    f.clear_filter()
    return out


def two_handles(gpu, b, asg=None):
    """(handle with the tags installed, plain handle on the same corpus, the assignment)."""
    asg = tr.assignment(b) if asg is None else asg
    g = tr.install(_upload(gpu(), b), asg)
    rt = tr.row_tags(b["ids"], asg)
    assert g.tags_info() == (int((rt != NONE).sum()), len(rt), int(tr.tagged(asg)[0].max()) + 1)
    for t in set(tr.PATTERN):
        assert g.tag_rows(t) == int((rt == t).sum()), t
    return g, _upload(gpu(), b), asg


def _dev_search(g, q, k, qt, nprobe, max_codes, ef, heap=False, keys=False):
    """search_tags_dev on device buffers: dict of dist, labels, the kernel and, asked for, out_keys and what they resolve to."""
    import torch
    dev = torch.device("cuda", 0)
    nq = len(q)
    d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    d_t = None if qt is None else torch.from_numpy(np.ascontiguousarray(qt).view(np.int16)).to(dev)
    dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ll = torch.empty((nq, k), dtype=torch.int64, device=dev)
    kk = torch.empty((nq, k), dtype=torch.int64, device=dev) if keys else None
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    g.search_tags_dev(nq, k, d_q, d_t, dd, ll, nprobe, max_codes, efSearch=ef, d_out_keys=kk, heap_order=heap)
    g.sync()
    r = dict(dist=dd.cpu().numpy(), labels=ll.cpu().numpy(), kernel=g.last_scan_kernel())
    if keys:
        r["keys"] = kk.cpu().numpy()
        d2 = torch.empty((nq, k), dtype=torch.float32, device=dev)
        l2 = torch.empty((nq, k), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        g.resolve_keys_dev(nq, k, kk, d2, l2)
        g.sync()
        r["resolved"] = (d2.cpu().numpy(), l2.cpu().numpy())
    return r


# ---- 1. k = 1, every code size, both forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CODE_SIZES, ids=lambda kw: "M%d" % kw["M"])
def test_k1_code_sizes(gpu, kw):
    b = base(**kw)
    g, f, asg = two_handles(gpu, b)
    q128 = tr.tiled(b["queries"], 128)
    refs = tr.per_tag(tr.oracle_search(tr.IVF_PARAMS, 1), b, asg, q128, 1)
    hrefs = handle_per_tag(f, b, asg, 128, 1, lambda h: h.search(q128, 1, NPROBE, MAX_CODES, efSearch=EF))
    plain = "scan_k1_kernel" if kw["M"] in (8, 16, 32) else "scan_k1_kernel (run-time code size)"
    for rep in (1, 8):  # 128 queries: several workgroups per query (atomicMin); 1024: one, which resolves the label itself
        q = tr.tiled(q128, 128 * rep)
        qt = tr.query_tags(len(q))
        idx = np.arange(len(q)) % 128
        got = g.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF)
        assert g.last_scan_kernel() == plain + "+tags"
        counts = g.last_scan_counts()
        assert_same(got, tr.compose(refs, qt, idx), (rep, "oracle"))
        assert_same(got, tr.compose(hrefs, qt, idx), (rep, "single filter"))
        f.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
        assert f.last_scan_kernel() == plain and counts == f.last_scan_counts()
    for t in set(tr.PATTERN) - {ABSENT}:
        assert (got[1][qt == t] >= 0).any(), t
    assert (got[1][qt == ABSENT] == -1).all() and (got[0][qt == ABSENT] == tr.FLT_MAX).all()
    assert (got[1][qt == NONE] >= 0).all()


# ---- 2. Grouping -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pruning", [False, True], ids=["all", "pruned"])
@pytest.mark.parametrize("kw", GROUPING[:2], ids=lambda kw: "nsubc%d" % kw["nsubc"])
def test_grouping(gpu, kw, pruning):
    b = base(**kw)
    g, f, asg = two_handles(gpu, b)
    nprobe, mc, ef = tr.GROUPING_PARAMS
    q128 = tr.tiled(b["queries"], 128)
    for k in (1, 10):
        refs = tr.per_tag(tr.oracle_search(tr.GROUPING_PARAMS, k, pruning), b, asg, q128, k)
        for rep in ((1, 8) if k == 1 else (1,)):
            q = tr.tiled(q128, 128 * rep)
            qt = tr.query_tags(len(q))
            got = g.search_tags(q, k, qt, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=True)
            assert g.last_scan_kernel() == ("scan_k1_bitmap_kernel+tags" if k == 1 else "scan_topk_kernel+tags")
            counts = g.last_scan_counts()
            assert_same(got, tr.compose(refs, qt, np.arange(len(q)) % 128), (k, rep))
            f.search(q, k, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=True)
            assert counts == f.last_scan_counts()
        assert (got[1][qt == 0] >= 0).any() and (got[1][qt == ABSENT] == -1).all()


# ---- 3. k > 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
def test_topk_both_orders(gpu, k):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    q = b["queries"]
    qt = tr.query_tags(len(q))
    refs = tr.per_tag(tr.oracle_search(tr.IVF_PARAMS, k), b, asg, q, k)
    got = g.search_tags(q, k, qt, NPROBE, MAX_CODES, efSearch=EF, heap_order=True)
    assert g.last_scan_kernel() == "scan_topk_kernel+tags"
    assert_same(got, tr.compose(refs, qt), "heap order, oracle")  # faiss's heap array, element for element
    for heap in (True, False):
        hrefs = handle_per_tag(f, b, asg, len(q), k,
                               lambda h: h.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap))
        got = g.search_tags(q, k, qt, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
        assert_same(got, tr.compose(hrefs, qt), ("single filter", heap))
    short = got[1][qt == 1]  # 1 % of the ~2000 codes a query scans: the 1 % tag leaves places unfilled
    assert ((short >= 0).sum(1) < k).any() and (short >= 0).any()


def test_heap_scan_k2000(gpu):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    nprobe, ef, k, mc = 64, 80, 2000, 10 ** 9
    q = b["queries"][:32]
    qt = tr.query_tags(32)
    refs = tr.per_tag(tr.oracle_search((nprobe, mc, ef), k), b, asg, q, k)
    assert ((refs[0][1] >= 0).sum(1) == k)[qt == 0].any(), "fixture: a query tagged 0 must admit more than k passing codes"
    got = g.search_tags(q, k, qt, nprobe, mc, efSearch=ef, heap_order=True)
    assert g.last_scan_kernel() == "heap_scan_kernel+tags"
    assert_same(got, tr.compose(refs, qt), "oracle")
    hrefs = handle_per_tag(f, b, asg, 32, k, lambda h: h.search(q, k, nprobe, mc, efSearch=ef, heap_order=True))
    assert_same(got, tr.compose(hrefs, qt), "single filter")


def test_heap_redo_path(gpu):
    """The stream of the query tagged 0xfffe overflows: heap_scan_kernel's tag form redoes it, and resolves the tag of every
    listed query anew -- the same query beside it under NONE (overflows too) and tagged 4242."""
    from test_gpu_heap_unbounded import CAP
    import torch
    b, q, qt, asg, (nprobe, max_codes, ef, k) = tr.redo_case(base)
    g = tr.install(_upload(gpu(), b), asg)
    refs = tr.per_tag(tr.oracle_search((nprobe, max_codes, ef), k), b, asg, q, k, tags=qt)
    r = _dev_search(g, q, k, qt, nprobe, max_codes, ef, heap=True)
    assert r["kernel"] == "scan_topk_kernel+tags"
    ln = torch.empty((3,), dtype=torch.int32, device=torch.device("cuda", 0))
    g.last_stream_dev(3, d_len=ln)
    g.sync()
    ln = ln.cpu().numpy()
    assert ln[0] > CAP, "the stream must overflow for the redo path to run (length %d)" % ln[0]
    assert ln[2] == 0
    assert_same((r["dist"], r["labels"]), tr.compose(refs, qt))
    other = tr.labels_of(asg, 255)
    assert not np.isin(r["labels"][0], other).any() and np.isin(r["labels"][1], other).any()
    assert (r["labels"][2] == -1).all()


# ---- 4. keys --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,heap", [(1, False), (10, True)])
def test_out_keys_and_resolve(gpu, k, heap):
    """out_keys and resolve_keys_dev of every query equal those of an unfiltered handle that uploaded the poisoned corpus of
    the query's tag."""
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    q = b["queries"]
    qt = tr.query_tags(len(q))
    a = _dev_search(g, q, k, qt, NPROBE, MAX_CODES, EF, heap=heap, keys=True)
    assert a["kernel"].endswith("+tags")
    for t in sorted(set(tr.PATTERN)):
        _upload(f, tr.tag_corpus(b, asg, t), graph=False)
        c = _dev_search(f, q, k, None, NPROBE, MAX_CODES, EF, heap=heap, keys=True)
        assert not c["kernel"].endswith("+tags")
        m = qt == t
        assert np.array_equal(a["keys"][m], c["keys"][m]), t
        assert _same_search((a["resolved"][0][m], a["resolved"][1][m]), (c["resolved"][0][m], c["resolved"][1][m])), t
        assert _same_search((a["dist"][m], a["labels"][m]), (c["dist"][m], c["labels"][m])), t
    lab = a["resolved"][1][qt == 255]
    assert np.isin(lab[lab >= 0], tr.labels_of(asg, 255)).all() and (lab >= 0).any()


# ---- 5. split batch -------------------------------------------------------------------------------------------------------
def test_split_batch(gpu):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    nq = 8192 + 128
    q = tr.tiled(b["queries"], nq)
    qt = tr.query_tags(nq)
    r = _dev_search(g, q, 1, qt, NPROBE, MAX_CODES, EF)
    assert g.last_batch_parts()[1] > 0, "the batch did not take the two-part path"
    assert g.last_batch_parts()[0] % 9 != 0  # the second part's tags start inside the pattern
    assert r["kernel"] == "scan_k1_kernel+tags"
    small = [g.search_tags(q[i:i + 128], 1, qt[i:i + 128], NPROBE, MAX_CODES, efSearch=EF) for i in range(0, nq, 128)]
    want = (np.concatenate([s[0] for s in small]), np.concatenate([s[1] for s in small]))
    assert_same((r["dist"], r["labels"]), want)


# ---- 6. range search ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,params", [(BASE, tr.IVF_PARAMS), (GROUPING[1], tr.GROUPING_PARAMS)], ids=["ivfadc", "grouping"])
def test_range_search(gpu, kw, params):
    b = base(**kw)
    g, f, asg = two_handles(gpu, b)
    nprobe, mc, ef = params
    q = tr.tiled(b["queries"], 128)
    qt = tr.query_tags(len(q))
    tenth = f.search(q, 10, nprobe, mc, efSearch=ef)[0][:, 9]
    radius = float(np.median(tenth))  # ten codes or more inside for half of the queries
    lims, dist, lab = g.range_search_tags(q, radius, qt, nprobe, mc, efSearch=ef)
    assert g.last_scan_kernel().endswith("+tags")
    assert len(lims) == len(q) + 1 and lims[0] == 0 and lims[-1] == len(dist) == len(lab)
    sizes = np.diff(lims.astype(np.int64))
    assert (sizes[qt == ABSENT] == 0).all()
    assert 100 <= sizes[qt == 0].sum() <= 2000, "the 50 % tag returns a few hundred rows at this radius"
    for t in sorted(set(tr.PATTERN)):
        mine = np.nonzero(qt == t)[0]
        if t == NONE:
            f.clear_filter()
        else:
            f.set_filter(tr.labels_of(asg, t))
        rl, rd, rb = f.range_search(q[mine], radius, nprobe, mc, efSearch=ef)
        for j, i in enumerate(mine):
            a0, a1, r0, r1 = int(lims[i]), int(lims[i + 1]), int(rl[j]), int(rl[j + 1])
            assert np.array_equal(lab[a0:a1], rb[r0:r1]), (t, i)
            assert np.array_equal(dist[a0:a1].view(np.uint32), rd[r0:r1].view(np.uint32)), (t, i)
    f.clear_filter()


# ---- 7. latency path, no table, all NONE ----------------------------------------------------------------------------------
def test_latency_path(gpu):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    g.prepare_latency()
    q = b["queries"][:8]
    qt = np.array([0, 0xfffe, 255, 1, 256, NONE, ABSENT, 0], np.uint16)
    plain = g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel() == "ivf_tail_kernel"
    refs = tr.per_tag(tr.oracle_search(tr.IVF_PARAMS, 1), b, asg, q, 1, tags=qt)
    got = g.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel() == "scan_k1_kernel+tags"
    assert_same(got, tr.compose(refs, qt))
    assert _same_search(g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF), plain)
    assert g.last_scan_kernel() == "ivf_tail_kernel"


@pytest.mark.parametrize("k,heap", [(1, False), (10, True)])
def test_no_tag_table(gpu, k, heap):
    """A _tags call on a handle without a tag table: every row is NONE, so a tagged query finds nothing and an untagged
    one what the plain call finds."""
    b = base(**BASE)
    g = _upload(gpu(), b)
    assert g.tags_info() == (0, len(b["ids"]), 0) and g.tag_rows(NONE) == len(b["ids"]) and g.tag_rows(0) == 0
    q = b["queries"]
    qt = tr.query_tags(len(q))
    plain = g.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
    for got in (g.search_tags(q, k, qt, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap),
                tuple(_dev_search(g, q, k, qt, NPROBE, MAX_CODES, EF, heap=heap)[x] for x in ("dist", "labels"))):
        assert g.last_scan_kernel().endswith("+tags")
        assert (got[1][qt != NONE] == -1).all() and (got[0][qt != NONE] == tr.FLT_MAX).all()
        assert _same_search((got[0][qt == NONE], got[1][qt == NONE]), (plain[0][qt == NONE], plain[1][qt == NONE]))
    lims, dist, lab = g.range_search_tags(q, 1e30, qt, NPROBE, MAX_CODES, efSearch=EF)
    sizes = np.diff(lims.astype(np.int64))
    assert (sizes[qt != NONE] == 0).all() and (sizes[qt == NONE] > 0).all()


@pytest.mark.parametrize("k,heap", [(1, False), (10, True), (10, False)])
def test_all_none_equals_plain(gpu, k, heap):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    q = b["queries"]
    plain = f.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
    kernel, counts = f.last_scan_kernel(), f.last_scan_counts()
    got = g.search_tags(q, k, np.full(len(q), NONE, np.uint16), NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
    assert _same_search(got, plain)
    assert g.last_scan_kernel() == kernel + "+tags" and g.last_scan_counts() == counts
    # query_tags None is the plain call, path and kernel name included; plain calls never read tags
    assert _same_search(g.search_tags(q, k, None, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap), plain)
    assert g.last_scan_kernel() == kernel
    assert _same_search(g.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap), plain)


def test_tags_ignore_slots_and_slots_ignore_tags(gpu):
    import filter_slots_ref as fs
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    q = b["queries"]
    qt = tr.query_tags(len(q))
    qs = fs.query_slots(len(q))
    before = g.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF)
    sets = fs.slot_sets(b)
    fs.install(g, sets)
    fs.install(f, sets)
    assert _same_search(g.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF), before)
    assert _same_search(g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF),
                        f.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF))
    assert g.last_scan_kernel() == "scan_k1_kernel+slots"
