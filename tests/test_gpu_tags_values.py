"""Tag AND value: each query searches only the rows that carry its tag and whose value lies in its interval
(ivfhnsw_gpu_search_tags_values).

Expected values, both exact (labels and distance bits): (A) the oracle on the poisoned corpus of every pair
(tags_values_ref), (B) the single-filter path -- a second handle with set_filter(labels that pass the pair) and the plain
call.  last_scan_kernel proves that the tag-and-value form of the expected scan kernel ran, last_scan_counts that it scored
what the plain call scores."""
import numpy as np
import pytest

import tags_values_ref as tv
from test_gpu_filter_slots import assert_same, base
from test_gpu_remove import BASE, CODE_SIZES, GROUPING, _upload, _same_search

pytestmark = pytest.mark.gpu

NPROBE, MAX_CODES, EF = tv.IVF_PARAMS
SUFFIX = "+tags+values"


def handle_per_pair(f, b, asg, nq, k, call, pairs=None):
    """{pair: (dist, labels)} from the single-filter path: call(f) -> (dist, labels) under set_filter(labels that pass the
    pair); the unfiltered pair is the call without a filter."""
    out = {}
    for p in sorted({tv.key(p) for p in (tv.PATTERN if pairs is None else pairs)}):
        if p == tv.key(tv.UNFILTERED):
            f.clear_filter()
        else:
            f.set_filter(tv.labels_in(asg, p))  # (a pair no label passes: the empty allow set)
        res = call(f)
        out[p] = (res[0].reshape(nq, k), res[1].reshape(nq, k))
    f.clear_filter()
    return out


def check_rows(g, b, asg):
    """tag_value_rows against numpy for every pattern entry (asg: what the handle holds)."""
    for p in tv.PATTERN:
        t, (lo, hi) = tv.key(p)
        assert g.tag_value_rows(t, lo, hi) == int(tv.passing_rows(b, asg, p).sum()), p


def two_handles(gpu, b, asg=None):
    """(handle with tags and values installed, plain handle on the same corpus, the assignment)."""
    asg = tv.assignment(b) if asg is None else asg
    g = tv.install(_upload(gpu(), b), asg)
    check_rows(g, b, asg)
    return g, _upload(gpu(), b), asg


def _dev_search(g, q, k, qt, qr, nprobe, max_codes, ef, heap=False, keys=False, stream=False):
    """search_tags_values_dev on device buffers: dict of dist, labels, the kernel and, asked for, out_keys with what they
    resolve to, and the candidate streams with their lengths."""
    import torch
    dev = torch.device("cuda", 0)
    nq = len(q)
    d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    d_t = None if qt is None else torch.from_numpy(np.ascontiguousarray(qt).view(np.int16)).to(dev)
    d_r = None if qr is None else torch.from_numpy(np.ascontiguousarray(qr).view(np.int32)).to(dev)
    dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ll = torch.empty((nq, k), dtype=torch.int64, device=dev)
    kk = torch.empty((nq, k), dtype=torch.int64, device=dev) if keys else None
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    g.search_tags_values_dev(nq, k, d_q, d_t, d_r, dd, ll, nprobe, max_codes, efSearch=ef, d_out_keys=kk, heap_order=heap)
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


def _padding_only(got, m):
    return (got[1][m] == -1).all() and (got[0][m] == tv.FLT_MAX).all()


# ---- 1. k = 1, every code size, both forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CODE_SIZES, ids=lambda kw: "M%d" % kw["M"])
def test_k1_code_sizes(gpu, kw):
    b = base(**kw)
    g, f, asg = two_handles(gpu, b)
    q128 = tv.tiled(b["queries"], 128)
    refs = tv.per_pair(tv.oracle_search(tv.IVF_PARAMS, 1), b, asg, q128, 1)
    hrefs = handle_per_pair(f, b, asg, 128, 1, lambda h: h.search(q128, 1, NPROBE, MAX_CODES, efSearch=EF))
    plain = "scan_k1_kernel" if kw["M"] in (8, 16, 32) else "scan_k1_kernel (run-time code size)"
    for rep in (1, 8):  # 128 queries: several workgroups per query (atomicMin); 1024: one, which resolves the label itself
        q = tv.tiled(q128, 128 * rep)
        qt, qr = tv.query_tags(len(q)), tv.query_ranges(len(q))
        idx = np.arange(len(q)) % 128
        got = g.search_tags_values(q, 1, qt, qr, NPROBE, MAX_CODES, efSearch=EF)
        assert g.last_scan_kernel() == plain + SUFFIX
        counts = g.last_scan_counts()
        assert_same(got, tv.compose(refs, qt, qr, idx), (rep, "oracle"))
        assert_same(got, tv.compose(hrefs, qt, qr, idx), (rep, "single filter"))
        f.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
        assert f.last_scan_kernel() == plain and counts == f.last_scan_counts()
    for p in tv.PATTERN:
        m = tv.mine(qt, qr, p)
        if p in tv.PADDING:
            assert _padding_only(got, m), p
        else:
            assert (got[1][m] >= 0).any(), p
    assert (got[1][tv.mine(qt, qr, tv.UNFILTERED)] >= 0).all()


# ---- 2. Grouping -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pruning", [False, True], ids=["all", "pruned"])
@pytest.mark.parametrize("kw", GROUPING[:2], ids=lambda kw: "nsubc%d" % kw["nsubc"])
def test_grouping(gpu, kw, pruning):
    b = base(**kw)
    g, f, asg = two_handles(gpu, b)
    nprobe, mc, ef = tv.GROUPING_PARAMS
    q128 = tv.tiled(b["queries"], 128)
    for k in (1, 10):
        refs = tv.per_pair(tv.oracle_search(tv.GROUPING_PARAMS, k, pruning), b, asg, q128, k)
        for rep in ((1, 8) if k == 1 else (1,)):
            q = tv.tiled(q128, 128 * rep)
            qt, qr = tv.query_tags(len(q)), tv.query_ranges(len(q))
            got = g.search_tags_values(q, k, qt, qr, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=True)
            assert g.last_scan_kernel() == ("scan_k1_bitmap_kernel" if k == 1 else "scan_topk_kernel") + SUFFIX
            counts = g.last_scan_counts()
            assert_same(got, tv.compose(refs, qt, qr, np.arange(len(q)) % 128), (k, rep))
            f.search(q, k, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=True)
            assert counts == f.last_scan_counts()
        assert (got[1][tv.mine(qt, qr, (255, (0, 0)))] >= 0).any() and _padding_only(got, tv.mine(qt, qr, tv.DISJOINT))


# ---- 3. k > 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
def test_topk_both_orders(gpu, k):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    q = b["queries"]
    qt, qr = tv.query_tags(len(q)), tv.query_ranges(len(q))
    refs = tv.per_pair(tv.oracle_search(tv.IVF_PARAMS, k), b, asg, q, k)
    got = g.search_tags_values(q, k, qt, qr, NPROBE, MAX_CODES, efSearch=EF, heap_order=True)
    assert g.last_scan_kernel() == "scan_topk_kernel" + SUFFIX
    assert_same(got, tv.compose(refs, qt, qr), "heap order, oracle")  # faiss's heap array, element for element
    for heap in (True, False):
        hrefs = handle_per_pair(f, b, asg, len(q), k,
                                lambda h: h.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap))
        got = g.search_tags_values(q, k, qt, qr, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
        assert_same(got, tv.compose(hrefs, qt, qr), ("single filter", heap))
    short = got[1][tv.mine(qt, qr, tv.FEW)]  # a tag of 2 to 6 rows: places stay unfilled
    assert ((short >= 0).sum(1) < k).all() and (short >= 0).any()
    assert _padding_only(got, tv.mine(qt, qr, tv.DISJOINT))


def test_heap_scan_k2000(gpu):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    nprobe, ef, k, mc = 64, 80, 2000, 10 ** 9
    q = b["queries"][:39]
    qt, qr = tv.query_tags(39), tv.query_ranges(39)
    refs = tv.per_pair(tv.oracle_search((nprobe, mc, ef), k), b, asg, q, k)
    half = tv.key((0, tv.FULL))
    assert ((refs[half][1] >= 0).sum(1) == k)[tv.mine(qt, qr, half)].any(), \
        "fixture: a query on the 50 % tag must admit more than k passing codes"
    got = g.search_tags_values(q, k, qt, qr, nprobe, mc, efSearch=ef, heap_order=True)
    assert g.last_scan_kernel() == "heap_scan_kernel" + SUFFIX
    assert_same(got, tv.compose(refs, qt, qr), "oracle")
    hrefs = handle_per_pair(f, b, asg, 39, k, lambda h: h.search(q, k, nprobe, mc, efSearch=ef, heap_order=True))
    assert_same(got, tv.compose(hrefs, qt, qr), "single filter")


# ---- 4. keys and streams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,heap", [(1, False), (10, False), (10, True)])
def test_keys_and_streams(gpu, k, heap):
    """out_keys, resolve_keys_dev and, in heap order, the candidate stream of every query (its length and its keys, entry
    for entry) equal those of an unfiltered handle that uploaded the poisoned corpus of the query's pair."""
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    q = b["queries"]
    qt, qr = tv.query_tags(len(q)), tv.query_ranges(len(q))
    a = _dev_search(g, q, k, qt, qr, NPROBE, MAX_CODES, EF, heap=heap, keys=True, stream=heap)
    assert a["kernel"].endswith(SUFFIX)
    if heap:
        assert a["kernel"] == "scan_topk_kernel" + SUFFIX
    for p in tv.PATTERN:
        _upload(f, tv.pair_corpus(b, asg, p), graph=False)
        c = _dev_search(f, q, k, None, None, NPROBE, MAX_CODES, EF, heap=heap, keys=True, stream=heap)
        assert "+" not in c["kernel"]
        m = tv.mine(qt, qr, p)
        assert np.array_equal(a["keys"][m], c["keys"][m]), p
        assert _same_search((a["resolved"][0][m], a["resolved"][1][m]), (c["resolved"][0][m], c["resolved"][1][m])), p
        assert _same_search((a["dist"][m], a["labels"][m]), (c["dist"][m], c["labels"][m])), p
        if heap:
            assert np.array_equal(a["len"][m], c["len"][m]), p
            for i in np.nonzero(m)[0]:
                assert np.array_equal(a["stream"][i], c["stream"][i]), (p, i)
            if p in (tv.UNFILTERED, (0, tv.FULL)):
                assert (a["len"][m] >= k).all(), p  # the comparison is of real streams, not of empty ones
            if p in tv.PADDING:
                assert (a["len"][m] == 0).all(), p
    pair = (0xfffe, tv.UPPER31)
    lab = a["resolved"][1][tv.mine(qt, qr, pair)]
    assert np.isin(lab[lab >= 0], tv.labels_in(asg, pair)).all() and (lab >= 0).any()


# ---- 5. split batch -------------------------------------------------------------------------------------------------------
def test_split_batch(gpu):
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    nq = 8192 + 13
    q = tv.tiled(b["queries"], nq)
    qt, qr = tv.query_tags(nq), tv.query_ranges(nq)
    r = _dev_search(g, q, 1, qt, qr, NPROBE, MAX_CODES, EF)
    assert g.last_batch_parts()[1] > 0, "the batch did not take the two-part path"
    assert g.last_batch_parts()[0] % 13 != 0  # the second part's tags and pairs start inside the pattern
    assert r["kernel"] == "scan_k1_kernel" + SUFFIX
    small = [g.search_tags_values(q[i:i + 128], 1, qt[i:i + 128], qr[i:i + 128], NPROBE, MAX_CODES, efSearch=EF)
             for i in range(0, nq, 128)]
    want = (np.concatenate([s[0] for s in small]), np.concatenate([s[1] for s in small]))
    assert_same((r["dist"], r["labels"]), want)
    # ... and the small calls are the oracle's answers (the first 128 queries)
    refs = tv.per_pair(tv.oracle_search(tv.IVF_PARAMS, 1), b, asg, q[:128], 1)
    assert_same((r["dist"][:128], r["labels"][:128]), tv.compose(refs, qt[:128], qr[:128]))
    # the host form of the same batch: both arrays staged in one block
    got = g.search_tags_values(q, 1, qt, qr, NPROBE, MAX_CODES, efSearch=EF)
    assert_same(got, want)


# ---- 6. range search ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,params", [(BASE, tv.IVF_PARAMS), (GROUPING[1], tv.GROUPING_PARAMS)], ids=["ivfadc", "grouping"])
def test_range_search(gpu, kw, params):
    import torch
    b = base(**kw)
    g, f, asg = two_handles(gpu, b)
    nprobe, mc, ef = params
    q = tv.tiled(b["queries"], 128)
    qt, qr = tv.query_tags(len(q)), tv.query_ranges(len(q))
    tenth = f.search(q, 10, nprobe, mc, efSearch=ef)[0][:, 9]
    radius = float(np.median(tenth))  # ten codes or more inside for half of the queries
    lims, dist, lab = g.range_search_tags_values(q, radius, qt, qr, nprobe, mc, efSearch=ef)
    assert g.last_scan_kernel().startswith("range_scan_") and g.last_scan_kernel().endswith(SUFFIX)
    assert len(lims) == len(q) + 1 and lims[0] == 0 and lims[-1] == len(dist) == len(lab)
    sizes = np.diff(lims.astype(np.int64))
    for p in tv.PADDING:
        assert (sizes[tv.mine(qt, qr, p)] == 0).all(), p
    assert sizes[tv.mine(qt, qr, (0, tv.FULL))].sum() >= 5, "the 50 % tag returns rows at this radius"
    # the _dev form: the same lims and the same results in scan order
    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(q).to(dev)
    d_t = torch.from_numpy(qt.view(np.int16)).to(dev)
    d_r = torch.from_numpy(qr.view(np.int32)).to(dev)
    d_lims = torch.zeros(len(q) + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    total = g.range_search_tags_values_dev(len(q), d_q, radius, d_t, d_r, d_lims, nprobe, mc, efSearch=ef)
    g.sync()
    assert total == len(dist) and np.array_equal(d_lims.cpu().numpy().astype(np.uint64), lims)
    dd, dl = g.range_results(0, total)
    assert np.array_equal(dl, lab) and np.array_equal(dd.view(np.uint32), dist.view(np.uint32))
    for p in tv.PATTERN:
        mine = np.nonzero(tv.mine(qt, qr, p))[0]
        if p == tv.UNFILTERED:
            f.clear_filter()
        else:
            f.set_filter(tv.labels_in(asg, p))
        rl, rd, rb = f.range_search(q[mine], radius, nprobe, mc, efSearch=ef)
        for j, i in enumerate(mine):
            a0, a1, r0, r1 = int(lims[i]), int(lims[i + 1]), int(rl[j]), int(rl[j + 1])
            assert np.array_equal(lab[a0:a1], rb[r0:r1]), (p, i)
            assert np.array_equal(dist[a0:a1].view(np.uint32), rd[r0:r1].view(np.uint32)), (p, i)
    f.clear_filter()


# ---- 7. one query per call, delegations, missing tables, independence -------------------------------------------------------
def test_one_query_per_call(gpu):
    """One query per call: the latency walk serves the coarse stage, the tag-and-value form of the scan follows it; the
    pinned block carries the pair 8-byte aligned and the tag behind it."""
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    g.prepare_latency()
    q = b["queries"][:13]
    qt, qr = tv.query_tags(13), tv.query_ranges(13)
    plain = g.search(q[:1], 1, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel() == "ivf_tail_kernel"
    refs = tv.per_pair(tv.oracle_search(tv.IVF_PARAMS, 1), b, asg, q, 1)
    want = tv.compose(refs, qt, qr)
    for i in range(13):
        got = g.search_tags_values(q[i:i + 1], 1, qt[i:i + 1], qr[i:i + 1], NPROBE, MAX_CODES, efSearch=EF)
        assert g.last_scan_kernel() == "scan_k1_kernel" + SUFFIX
        assert_same(got, (want[0][i:i + 1], want[1][i:i + 1]), i)
    # three queries: an odd number of floats before the pick's arrays
    got = g.search_tags_values(q[3:6], 1, qt[3:6], qr[3:6], NPROBE, MAX_CODES, efSearch=EF)
    assert_same(got, (want[0][3:6], want[1][3:6]), "three")
    assert _same_search(g.search(q[:1], 1, NPROBE, MAX_CODES, efSearch=EF), plain)
    assert g.last_scan_kernel() == "ivf_tail_kernel"


@pytest.mark.parametrize("k,heap", [(1, False), (10, True)])
def test_delegations(gpu, k, heap):
    """query_tags None is the _values call, query_ranges None the _tags call, both None the plain call: answers and kernel
    names; and the wildcards on one side give the other side's answers under the compound kernel."""
    import tags_ref as tr
    import values_ref as vr
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    q = b["queries"]
    nq = len(q)
    kw = dict(efSearch=EF, heap_order=heap)
    plain = g.search(q, k, NPROBE, MAX_CODES, **kw)
    name, counts = g.last_scan_kernel(), g.last_scan_counts()
    vqr = vr.query_ranges(nq)
    want_v = g.search_values(q, k, vqr, NPROBE, MAX_CODES, **kw)
    assert g.last_scan_kernel() == name + "+values"
    tqt = tr.query_tags(nq)
    want_t = g.search_tags(q, k, tqt, NPROBE, MAX_CODES, **kw)
    assert g.last_scan_kernel() == name + "+tags"
    assert _same_search(g.search_tags_values(q, k, None, vqr, NPROBE, MAX_CODES, **kw), want_v)
    assert g.last_scan_kernel() == name + "+values"
    assert _same_search(g.search_tags_values(q, k, tqt, None, NPROBE, MAX_CODES, **kw), want_t)
    assert g.last_scan_kernel() == name + "+tags"
    assert _same_search(g.search_tags_values(q, k, None, None, NPROBE, MAX_CODES, **kw), plain)
    assert g.last_scan_kernel() == name
    for dev_args, want, suffix in ((( None, vqr), want_v, "+values"), ((tqt, None), want_t, "+tags"), ((None, None), plain, "")):
        r = _dev_search(g, q, k, dev_args[0], dev_args[1], NPROBE, MAX_CODES, EF, heap=heap)
        assert r["kernel"] == name + suffix and _same_search((r["dist"], r["labels"]), want)
    # the wildcards: (t, FULL) is the _tags query, (NONE, (lo, hi)) the _values query, (NONE, FULL) the plain one
    full = np.tile(np.array(tv.FULL, np.uint32), (nq, 1))
    none = np.full(nq, tv.TAG_NONE, np.uint16)
    assert _same_search(g.search_tags_values(q, k, tqt, full, NPROBE, MAX_CODES, **kw), want_t)
    assert g.last_scan_kernel() == name + SUFFIX and g.last_scan_counts() == counts
    assert _same_search(g.search_tags_values(q, k, none, vqr, NPROBE, MAX_CODES, **kw), want_v)
    assert _same_search(g.search_tags_values(q, k, none, full, NPROBE, MAX_CODES, **kw), plain)
    assert g.last_scan_kernel() == name + SUFFIX and g.last_scan_counts() == counts
    # range search delegates the same way
    rv = g.range_search_values(q, 1e30, vqr, NPROBE, MAX_CODES, efSearch=EF)
    rt = g.range_search_tags_values(q, 1e30, None, vqr, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel().endswith("+values") and not g.last_scan_kernel().endswith(SUFFIX)
    assert all(np.array_equal(x, y) for x, y in zip(rv, rt))
    rv = g.range_search_tags(q, 1e30, tqt, NPROBE, MAX_CODES, efSearch=EF)
    rt = g.range_search_tags_values(q, 1e30, tqt, None, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel().endswith("+tags")
    assert all(np.array_equal(x, y) for x, y in zip(rv, rt))


@pytest.mark.parametrize("tags,values", [(True, False), (False, True), (False, False)], ids=["tags-only", "values-only", "neither"])
def test_missing_tables(gpu, tags, values):
    """A handle that lacks the tag table, the value table or both: the missing one reads as NONE for every row."""
    b = base(**BASE)
    asg = tv.assignment(b)
    g = tv.install(_upload(gpu(), b), asg, tags=tags, values=values)
    f = _upload(gpu(), b)
    seen = tv.without(asg, tags=tags, values=values)
    check_rows(g, b, seen)
    q = b["queries"]
    qt, qr = tv.query_tags(len(q)), tv.query_ranges(len(q))
    for k, heap in ((1, False), (10, True)):
        hrefs = handle_per_pair(f, b, seen, len(q), k, lambda h: h.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap))
        want = tv.compose(hrefs, qt, qr)
        got = g.search_tags_values(q, k, qt, qr, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
        assert g.last_scan_kernel().endswith(SUFFIX)
        assert_same(got, want, (k, "host"))
        r = _dev_search(g, q, k, qt, qr, NPROBE, MAX_CODES, EF, heap=heap)
        assert_same((r["dist"], r["labels"]), want, (k, "dev"))
    assert (got[1][tv.mine(qt, qr, tv.UNFILTERED)] >= 0).all()
    if not tags:
        assert _padding_only(got, tv.mine(qt, qr, (0, tv.FULL)))
    if not values:
        assert _padding_only(got, tv.mine(qt, qr, (256, tv.VALUED)))
    lims, dist, lab = g.range_search_tags_values(q, 1e30, qt, qr, NPROBE, MAX_CODES, efSearch=EF)
    sizes = np.diff(lims.astype(np.int64))
    for p in tv.PATTERN:
        m = tv.mine(qt, qr, p)
        assert (sizes[m] > 0).any() == bool(tv.passing_rows(b, seen, p).any()), p


def test_independence(gpu):
    """No new state: after the new call, search, search_slots, search_tags and search_values answer what they answered
    before, and the new call ignores slots."""
    import filter_slots_ref as fs
    import tags_ref as tr
    import values_ref as vr
    b = base(**BASE)
    g, f, asg = two_handles(gpu, b)
    fs.install(g, fs.slot_sets(b))
    q = b["queries"]
    nq = len(q)
    qs, tqt, vqr = fs.query_slots(nq), tr.query_tags(nq), vr.query_ranges(nq)
    qt, qr = tv.query_tags(nq), tv.query_ranges(nq)

    def others():
        return [g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF), g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF),
                g.search_tags(q, 1, tqt, NPROBE, MAX_CODES, efSearch=EF), g.search_values(q, 1, vqr, NPROBE, MAX_CODES, efSearch=EF)]

    before = others()
    assert g.last_scan_kernel() == "scan_k1_kernel+values"
    mem = g.memory_bytes()  # (the _values call before has staged its 8 bytes per query)
    refs = tv.per_pair(tv.oracle_search(tv.IVF_PARAMS, 1), b, asg, q, 1)
    got = g.search_tags_values(q, 1, qt, qr, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel() == "scan_k1_kernel" + SUFFIX
    assert_same(got, tv.compose(refs, qt, qr), "with slots installed")
    for x, y in zip(before, others()):
        assert _same_search(x, y)
    # the staging of a host call is all that memory_bytes moves by: 2 + 8 bytes per query at the most
    assert 0 <= g.memory_bytes() - mem <= 10 * nq
    check_rows(g, b, asg)
    with pytest.raises(Exception):
        g.tag_value_rows(0x10000, 0, 1)
