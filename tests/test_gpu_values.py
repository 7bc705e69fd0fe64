"""Row values: each query searches only the rows whose uint32 value lies in its interval (ivfhnsw_gpu_search_values,
DESIGN.md 3.24).

Expected values, both exact (labels and distance bits): (A) the oracle on the poisoned corpus of every interval
(values_ref), (B) the single-filter path -- a second handle with set_filter(labels whose value lies in the interval) and
the plain call.  last_scan_kernel proves that the value form of the expected scan kernel ran, last_scan_counts that it
scored what the plain call scores."""
import numpy as np
import pytest

import values_ref as vr
from test_gpu_filter_slots import assert_same, base
from test_gpu_remove import BASE, CODE_SIZES, GROUPING, _upload, _same_search

pytestmark = pytest.mark.gpu

NPROBE, MAX_CODES, EF = vr.IVF_PARAMS
NONE, FULL, VALUED, POINT, INVERTED = vr.NONE, vr.FULL, vr.VALUED, vr.POINT, vr.INVERTED


def handle_per_range(f, b, asg, nq, k, call, ranges=None):
    """{(lo, hi): (dist, labels)} from the single-filter path: call(f) -> (dist, labels) under set_filter(labels whose value
    lies in the interval); the full interval is the call without a filter."""
    out = {}
    for r in sorted({vr.key(r) for r in (vr.PATTERN if ranges is None else ranges)}):
        if r == FULL:
            f.clear_filter()
        else:
            f.set_filter(vr.labels_in(asg, r))  # (an interval no label lies in: the empty allow set)
        res = call(f)
        out[r] = (res[0].reshape(nq, k), res[1].reshape(nq, k))
    f.clear_filter()
    return out


def count_rows(rv, r):
    v = rv.astype(np.uint64)
    return int(((v >= r[0]) & (v <= r[1])).sum())


def two_handles(gpu, b, asg=None):
    """(handle with the values installed, plain handle on the same corpus, the assignment)."""
    asg = vr.assignment(b) if asg is None else asg
    g = vr.install(_upload(gpu(), b), asg)
    rv = vr.row_values(b["ids"], asg)
    assert g.values_info() == (int((rv != NONE).sum()), len(rv), int(vr.valued(asg)[0].max()) + 1)
    for r in vr.PATTERN:
        assert g.value_rows(*r) == count_rows(rv, r), r
    return g, _upload(gpu(), b), asg


def _dev_search(g, q, k, qr, nprobe, max_codes, ef, heap=False, keys=False, stream=False):
    """search_values_dev on device buffers: dict of dist, labels, the kernel and, asked for, out_keys with what they resolve
    to, and the candidate streams with their lengths."""
    import torch
    dev = torch.device("cuda", 0)
    nq = len(q)
    d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    d_r = None if qr is None else torch.from_numpy(np.ascontiguousarray(qr).view(np.int32)).to(dev)
    dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ll = torch.empty((nq, k), dtype=torch.int64, device=dev)
    kk = torch.empty((nq, k), dtype=torch.int64, device=dev) if keys else None
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    g.search_values_dev(nq, k, d_q, d_r, dd, ll, nprobe, max_codes, efSearch=ef, d_out_keys=kk, heap_order=heap)
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
    if stream:
        ln = torch.empty((nq,), dtype=torch.int32, device=dev)
        r["cap"] = g.last_stream_dev(nq, d_len=ln)
        g.sync()
        r["len"] = ln.cpu().numpy()
        L = max(1, min(int(r["len"].max()), r["cap"]))
        st = torch.zeros((nq, L), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        g.last_stream_dev(nq, L, d_keys=st)
        g.sync()
        st = st.cpu().numpy()
        r["stream"] = [st[i, :min(r["len"][i], L)] for i in range(nq)]
    return r


# ---- 1. k = 1, every code size, both forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CODE_SIZES, ids=lambda kw: "M%d" % kw["M"])
def test_k1_code_sizes(gpu, kw):
    b = base(**kw)
    g, f, asg = two_handles(gpu, b)
    q128 = vr.tiled(b["queries"], 128)
    refs = vr.per_range(vr.oracle_search(vr.IVF_PARAMS, 1), b, asg, q128, 1)
    hrefs = handle_per_range(f, b, asg, 128, 1, lambda h: h.search(q128, 1, NPROBE, MAX_CODES, efSearch=EF))
    plain = "scan_k1_kernel" if kw["M"] in (8, 16, 32) else "scan_k1_kernel (run-time code size)"
    for rep in (1, 8):  # 128 queries: several workgroups per query (atomicMin); 1024: one, which resolves the label itself
        q = vr.tiled(q128, 128 * rep)
        qr = vr.query_ranges(len(q))
        idx = np.arange(len(q)) % 128
        got = g.search_values(q, 1, qr, NPROBE, MAX_CODES, efSearch=EF)
        assert g.last_scan_kernel() == plain + "+values"
        counts = g.last_scan_counts()
        assert_same(got, vr.compose(refs, qr, idx), (rep, "oracle"))
        assert_same(got, vr.compose(hrefs, qr, idx), (rep, "single filter"))
        f.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
        assert f.last_scan_kernel() == plain and counts == f.last_scan_counts()
    for r in vr.PATTERN:
        if r != INVERTED:
            assert (got[1][vr.mine(qr, r)] >= 0).any(), r
    assert (got[1][vr.mine(qr, INVERTED)] == -1).all() and (got[0][vr.mine(qr, INVERTED)] == vr.FLT_MAX).all()
    assert (got[1][vr.mine(qr, FULL)] >= 0).all()


# ---- 2. Grouping -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pruning", [False, True], ids=["all", "pruned"])
@pytest.mark.parametrize("kw", GROUPING[:2], ids=lambda kw: "nsubc%d" % kw["nsubc"])
def test_grouping(gpu, kw, pruning):
    b = base(**kw)
    g, f, asg = two_handles(gpu, b)
    nprobe, mc, ef = vr.GROUPING_PARAMS
    q128 = vr.tiled(b["queries"], 128)
    for k in (1, 10):
        refs = vr.per_range(vr.oracle_search(vr.GROUPING_PARAMS, k, pruning), b, asg, q128, k)
        for rep in ((1, 8) if k == 1 else (1,)):
            q = vr.tiled(q128, 128 * rep)
            qr = vr.query_ranges(len(q))
            got = g.search_values(q, k, qr, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=True)
            assert g.last_scan_kernel() == ("scan_k1_bitmap_kernel+values" if k == 1 else "scan_topk_kernel+values")
            counts = g.last_scan_counts()
            assert_same(got, vr.compose(refs, qr, np.arange(len(q)) % 128), (k, rep))
            f.search(q, k, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=True)
            assert counts == f.last_scan_counts()
        assert (got[1][vr.mine(qr, (0, 0))] >= 0).any() and (got[1][vr.mine(qr, INVERTED)] == -1).all()


# ---- 3. k > 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
def test_topk_both_orders(gpu, k):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    q = b["queries"]
    qr = vr.query_ranges(len(q))
    refs = vr.per_range(vr.oracle_search(vr.IVF_PARAMS, k), b, asg, q, k)
    got = g.search_values(q, k, qr, NPROBE, MAX_CODES, efSearch=EF, heap_order=True)
    assert g.last_scan_kernel() == "scan_topk_kernel+values"
    assert_same(got, vr.compose(refs, qr), "heap order, oracle")  # faiss's heap array, element for element
    for heap in (True, False):
        hrefs = handle_per_range(f, b, asg, len(q), k,
                                 lambda h: h.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap))
        got = g.search_values(q, k, qr, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
        assert_same(got, vr.compose(hrefs, qr), ("single filter", heap))
    short = got[1][vr.mine(qr, POINT)]  # 1 % of the ~2000 codes a query scans: the 1 % point leaves places unfilled
    assert ((short >= 0).sum(1) < k).any() and (short >= 0).any()


def test_heap_scan_k2000(gpu):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    nprobe, ef, k, mc = 64, 80, 2000, 10 ** 9
    q = b["queries"][:32]
    qr = vr.query_ranges(32)
    band = vr.PATTERN[3]
    refs = vr.per_range(vr.oracle_search((nprobe, mc, ef), k), b, asg, q, k)
    assert ((refs[band][1] >= 0).sum(1) == k)[vr.mine(qr, band)].any(), \
        "fixture: a query on the 50 % band must admit more than k passing codes"
    got = g.search_values(q, k, qr, nprobe, mc, efSearch=ef, heap_order=True)
    assert g.last_scan_kernel() == "heap_scan_kernel+values"
    assert_same(got, vr.compose(refs, qr), "oracle")
    hrefs = handle_per_range(f, b, asg, 32, k, lambda h: h.search(q, k, nprobe, mc, efSearch=ef, heap_order=True))
    assert_same(got, vr.compose(hrefs, qr), "single filter")


def test_heap_redo_path(gpu):
    """The stream of the query on (100, 200) overflows: heap_scan_kernel's value form redoes it, and resolves the interval
    of every listed query anew -- the same query beside it on the full interval (overflows too) and on the inverted one."""
    from test_gpu_heap_unbounded import CAP
    import torch
    b, q, qr, asg, (nprobe, max_codes, ef, k) = vr.redo_case(base)
    g = vr.install(_upload(gpu(), b), asg)
    refs = vr.per_range(vr.oracle_search((nprobe, max_codes, ef), k), b, asg, q, k, ranges=qr)
    r = _dev_search(g, q, k, qr, nprobe, max_codes, ef, heap=True)
    assert r["kernel"] == "scan_topk_kernel+values"
    ln = torch.empty((3,), dtype=torch.int32, device=torch.device("cuda", 0))
    g.last_stream_dev(3, d_len=ln)
    g.sync()
    ln = ln.cpu().numpy()
    assert ln[0] > CAP, "the stream must overflow for the redo path to run (length %d)" % ln[0]
    assert ln[2] == 0
    assert_same((r["dist"], r["labels"]), vr.compose(refs, qr))
    other = vr.labels_in(asg, (0x80000005, 0x80000005))
    assert not np.isin(r["labels"][0], other).any() and np.isin(r["labels"][1], other).any()
    assert (r["labels"][2] == -1).all()


# ---- 4. keys and streams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,heap", [(1, False), (10, False), (10, True)])
def test_keys_and_streams(gpu, k, heap):
    """out_keys, resolve_keys_dev and, in heap order, the candidate stream of every query (its length and its keys, entry
    for entry) equal those of an unfiltered handle that uploaded the poisoned corpus of the query's interval."""
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    q = b["queries"]
    qr = vr.query_ranges(len(q))
    a = _dev_search(g, q, k, qr, NPROBE, MAX_CODES, EF, heap=heap, keys=True, stream=heap)
    assert a["kernel"].endswith("+values")
    if heap:
        assert a["kernel"] == "scan_topk_kernel+values"
    for r in sorted(set(vr.PATTERN)):
        _upload(f, vr.range_corpus(b, asg, r), graph=False)
        c = _dev_search(f, q, k, None, NPROBE, MAX_CODES, EF, heap=heap, keys=True, stream=heap)
        assert not c["kernel"].endswith("+values")
        m = vr.mine(qr, r)
        assert np.array_equal(a["keys"][m], c["keys"][m]), r
        assert _same_search((a["resolved"][0][m], a["resolved"][1][m]), (c["resolved"][0][m], c["resolved"][1][m])), r
        assert _same_search((a["dist"][m], a["labels"][m]), (c["dist"][m], c["labels"][m])), r
        if heap:
            assert np.array_equal(a["len"][m], c["len"][m]), r
            for i in np.nonzero(m)[0]:
                assert np.array_equal(a["stream"][i], c["stream"][i]), (r, i)
            if r in (FULL, vr.PATTERN[3]):
                assert (a["len"][m] >= k).all(), r  # the comparison is of real streams, not of empty ones
            if r == INVERTED:
                assert (a["len"][m] == 0).all()
    lab = a["resolved"][1][vr.mine(qr, vr.PATTERN[6])]
    assert np.isin(lab[lab >= 0], vr.labels_in(asg, vr.PATTERN[6])).all() and (lab >= 0).any()


# ---- 5. split batch -------------------------------------------------------------------------------------------------------
def test_split_batch(gpu):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    nq = 8192 + 9
    q = vr.tiled(b["queries"], nq)
    qr = vr.query_ranges(nq)
    r = _dev_search(g, q, 1, qr, NPROBE, MAX_CODES, EF)
    assert g.last_batch_parts()[1] > 0, "the batch did not take the two-part path"
    assert g.last_batch_parts()[0] % 9 != 0  # the second part's intervals start inside the pattern
    assert r["kernel"] == "scan_k1_kernel+values"
    small = [g.search_values(q[i:i + 128], 1, qr[i:i + 128], NPROBE, MAX_CODES, efSearch=EF) for i in range(0, nq, 128)]
    want = (np.concatenate([s[0] for s in small]), np.concatenate([s[1] for s in small]))
    assert_same((r["dist"], r["labels"]), want)
    # ... and the small calls are the oracle's answers (the first 128 queries)
    refs = vr.per_range(vr.oracle_search(vr.IVF_PARAMS, 1), b, asg, q[:128], 1)
    assert_same((r["dist"][:128], r["labels"][:128]), vr.compose(refs, qr[:128]))


# ---- 6. range search ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,params", [(BASE, vr.IVF_PARAMS), (GROUPING[1], vr.GROUPING_PARAMS)], ids=["ivfadc", "grouping"])
def test_range_search(gpu, kw, params):
    import torch
    b = base(**kw)
    g, f, asg = two_handles(gpu, b)
    nprobe, mc, ef = params
    q = vr.tiled(b["queries"], 128)
    qr = vr.query_ranges(len(q))
    tenth = f.search(q, 10, nprobe, mc, efSearch=ef)[0][:, 9]
    radius = float(np.median(tenth))  # ten codes or more inside for half of the queries
    lims, dist, lab = g.range_search_values(q, radius, qr, nprobe, mc, efSearch=ef)
    assert g.last_scan_kernel().endswith("+values")
    assert len(lims) == len(q) + 1 and lims[0] == 0 and lims[-1] == len(dist) == len(lab)
    sizes = np.diff(lims.astype(np.int64))
    assert (sizes[vr.mine(qr, INVERTED)] == 0).all()
    assert 100 <= sizes[vr.mine(qr, vr.PATTERN[3])].sum() <= 2000, "the 50 % band returns a few hundred rows at this radius"
    # the _dev form: the same lims and the same results in scan order
    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(q).to(dev)
    d_r = torch.from_numpy(qr.view(np.int32)).to(dev)
    d_lims = torch.zeros(len(q) + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    total = g.range_search_values_dev(len(q), d_q, radius, d_r, d_lims, nprobe, mc, efSearch=ef)
    g.sync()
    assert total == len(dist) and np.array_equal(d_lims.cpu().numpy().astype(np.uint64), lims)
    dd, dl = g.range_results(0, total)
    assert np.array_equal(dl, lab) and np.array_equal(dd.view(np.uint32), dist.view(np.uint32))
    for r in sorted(set(vr.PATTERN)):
        mine = np.nonzero(vr.mine(qr, r))[0]
        if r == FULL:
            f.clear_filter()
        else:
            f.set_filter(vr.labels_in(asg, r))
        rl, rd, rb = f.range_search(q[mine], radius, nprobe, mc, efSearch=ef)
        for j, i in enumerate(mine):
            a0, a1, r0, r1 = int(lims[i]), int(lims[i + 1]), int(rl[j]), int(rl[j + 1])
            assert np.array_equal(lab[a0:a1], rb[r0:r1]), (r, i)
            assert np.array_equal(dist[a0:a1].view(np.uint32), rd[r0:r1].view(np.uint32)), (r, i)
    f.clear_filter()


# ---- 7. latency path, no table, all NONE ----------------------------------------------------------------------------------
def test_latency_path(gpu):
    """One query per call: the latency walk serves the coarse stage, the value form of the scan follows it."""
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    g.prepare_latency()
    q = b["queries"][:9]
    qr = vr.query_ranges(9)
    plain = g.search(q[:1], 1, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel() == "ivf_tail_kernel"
    refs = vr.per_range(vr.oracle_search(vr.IVF_PARAMS, 1), b, asg, q, 1, ranges=qr)
    want = vr.compose(refs, qr)
    for i in range(9):
        got = g.search_values(q[i:i + 1], 1, qr[i:i + 1], NPROBE, MAX_CODES, efSearch=EF)
        assert g.last_scan_kernel() == "scan_k1_kernel+values"
        assert_same(got, (want[0][i:i + 1], want[1][i:i + 1]), i)
    assert _same_search(g.search(q[:1], 1, NPROBE, MAX_CODES, efSearch=EF), plain)
    assert g.last_scan_kernel() == "ivf_tail_kernel"


@pytest.mark.parametrize("k,heap", [(1, False), (10, True)])
def test_no_value_table(gpu, k, heap):
    """A _values call on a handle without a table: every row is NONE, so only an interval that reaches 0xffffffff finds
    anything, and it finds what the plain call finds."""
    b = base(**BASE)
    g = _upload(gpu(), b)
    n = len(b["ids"])
    assert g.values_info() == (0, n, 0) and g.value_rows(0, NONE) == n and g.value_rows(NONE, NONE) == n
    assert g.value_rows(0, NONE - 1) == 0 and g.value_rows(NONE, 0) == 0
    q = b["queries"]
    qr = vr.query_ranges(len(q))
    qr[vr.mine(qr, POINT)] = (0x80000000, NONE)  # a second interval that ends at NONE, from the upper half
    full = (qr[:, 1] == NONE) & (qr[:, 0] <= qr[:, 1])
    assert full.sum() >= 2 * (len(q) // 9)
    plain = g.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
    for got in (g.search_values(q, k, qr, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap),
                tuple(_dev_search(g, q, k, qr, NPROBE, MAX_CODES, EF, heap=heap)[x] for x in ("dist", "labels"))):
        assert g.last_scan_kernel().endswith("+values")
        assert (got[1][~full] == -1).all() and (got[0][~full] == vr.FLT_MAX).all()
        assert _same_search((got[0][full], got[1][full]), (plain[0][full], plain[1][full]))
    lims, dist, lab = g.range_search_values(q, 1e30, qr, NPROBE, MAX_CODES, efSearch=EF)
    sizes = np.diff(lims.astype(np.int64))
    assert (sizes[~full] == 0).all() and (sizes[full] > 0).all()


def test_table_of_none_only(gpu):
    """A table in which every label is NONE answers as no table does, and counts as one."""
    b = base(**BASE)
    g = _upload(gpu(), b)
    ids = np.unique(b["ids"]).astype(np.uint32)
    g.set_values(ids, np.full(len(ids), NONE, np.uint32))
    n = len(b["ids"])
    assert g.values_info() == (0, n, int(ids.max()) + 1) and g.value_rows(0, NONE) == n and g.value_rows(0, NONE - 1) == 0
    q = b["queries"]
    qr = vr.query_ranges(len(q))
    full = vr.mine(qr, FULL)
    plain = g.search(q, 10, NPROBE, MAX_CODES, efSearch=EF)
    got = g.search_values(q, 10, qr, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel() == "scan_topk_kernel+values"
    assert (got[1][~full] == -1).all() and (got[0][~full] == vr.FLT_MAX).all()
    assert _same_search((got[0][full], got[1][full]), (plain[0][full], plain[1][full]))


@pytest.mark.parametrize("k,heap", [(1, False), (10, True), (10, False)])
def test_full_interval_equals_plain(gpu, k, heap):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    q = b["queries"]
    plain = f.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
    kernel, counts = f.last_scan_kernel(), f.last_scan_counts()
    got = g.search_values(q, k, np.tile(np.array(FULL, np.uint32), (len(q), 1)), NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
    assert _same_search(got, plain)
    assert g.last_scan_kernel() == kernel + "+values" and g.last_scan_counts() == counts
    # query_ranges None is the plain call, path and kernel name included; plain calls never read values
    assert _same_search(g.search_values(q, k, None, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap), plain)
    assert g.last_scan_kernel() == kernel
    assert _same_search(g.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap), plain)


def test_values_ignore_slots_and_tags(gpu):
    """Four independent states: a _values call ignores slots and tags, and _slots / _tags calls ignore the values."""
    import filter_slots_ref as fs
    import tags_ref as tr
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    q = b["queries"]
    qr = vr.query_ranges(len(q))
    qs = fs.query_slots(len(q))
    qt = tr.query_tags(len(q))
    before = g.search_values(q, 1, qr, NPROBE, MAX_CODES, efSearch=EF)
    sets = fs.slot_sets(b)
    tasg = tr.assignment(b)
    for h in (g, f):
        fs.install(h, sets)
        tr.install(h, tasg)
    assert _same_search(g.search_values(q, 1, qr, NPROBE, MAX_CODES, efSearch=EF), before)
    assert _same_search(g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF),
                        f.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF))
    assert g.last_scan_kernel() == "scan_k1_kernel+slots"
    assert _same_search(g.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF),
                        f.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF))
    assert g.last_scan_kernel() == "scan_k1_kernel+tags"
