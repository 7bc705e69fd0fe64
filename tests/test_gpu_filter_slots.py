"""Filter slots: a label filter per query (ivfhnsw_gpu_search_slots).

Expected values, both exact (labels and distance bits): (A) the oracle on the poisoned corpus of every slot
(filter_slots_ref), (B) the single-filter path -- a second handle with set_filter(labels of the slot) and the plain call
on the slot's queries.  last_scan_kernel proves that the per-query form of the expected scan kernel ran."""
import numpy as np
import pytest

from conftest import corpus
import filter_ref
import filter_slots_ref as fs
from test_gpu_remove import BASE, CODE_SIZES, GROUPING, _upload, _same_search, _with_ids

pytestmark = pytest.mark.gpu

NPROBE, MAX_CODES, EF = fs.IVF_PARAMS
NONE, UNSET = fs.NONE, fs.UNSET

_CLIPPED = {}


def base(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _CLIPPED:
        _CLIPPED[key] = filter_ref.clipped(corpus(**kw))
    return _CLIPPED[key]


def handle_per_slot(f, sets, nq, k, call, slots=None):
    """{slot: (dist, labels)} from the single-filter path: call(f) -> (dist, labels) under set_filter of every slot."""
    out = {}
    for s in sorted({int(s) for s in (fs.PATTERN if slots is None else slots)}):
        if s == NONE:
            f.clear_filter()
        elif s in sets:
            f.set_filter(sets[s][0], deny=sets[s][1])
        else:
            out[s] = (np.full((nq, k), fs.FLT_MAX, np.float32), np.full((nq, k), -1, np.int64))
            continue
        r = call(f)
        out[s] = (r[0].reshape(nq, k), r[1].reshape(nq, k))
    f.clear_filter()
    return out


def two_handles(gpu, b, sets=None):
    """(handle with the slots installed, plain handle on the same corpus, the sets)."""
    sets = fs.slot_sets(b) if sets is None else sets
    g = fs.install(_upload(gpu(), b), sets)
    for s, (labels, deny) in sets.items():
        rows = fs.passing_rows(b, sets, s)
        assert g.filter_slot_info(s) == (1 if deny else 0, int(rows.sum()), len(rows))
    assert g.filter_slot_info(UNSET) == (-1, 0, len(b["ids"]))
    return g, _upload(gpu(), b), sets


def assert_same(got, want, what=""):
    assert fs.same_bits(got, want), (what, fs.first_mismatch(got, want))


# ---- 1. k = 1, every code size, both forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CODE_SIZES, ids=lambda kw: "M%d" % kw["M"])
def test_k1_code_sizes(gpu, kw):
    b = base(**kw)
    g, f, sets = two_handles(gpu, b)
    q128 = fs.tiled(b["queries"], 128)
    refs = fs.per_slot(fs.oracle_search(fs.IVF_PARAMS, 1), b, sets, q128, 1)
    hrefs = handle_per_slot(f, sets, 128, 1, lambda h: h.search(q128, 1, NPROBE, MAX_CODES, efSearch=EF))
    plain = "scan_k1_kernel" if kw["M"] in (8, 16, 32) else "scan_k1_kernel (run-time code size)"
    for rep in (1, 8):  # 128 queries: several workgroups per query (atomicMin); 1024: one, which resolves the label itself
        q = fs.tiled(q128, 128 * rep)
        qs = fs.query_slots(len(q))
        idx = np.arange(len(q)) % 128
        got = g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF)
        assert g.last_scan_kernel() == plain + "+slots"
        counts = g.last_scan_counts()
        assert_same(got, fs.compose(refs, qs, idx), (rep, "oracle"))
        assert_same(got, fs.compose(hrefs, qs, idx), (rep, "single filter"))
        f.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
        assert f.last_scan_kernel() == plain and counts == f.last_scan_counts()
    for s in fs.SPECS:
        assert (got[1][qs == s] >= 0).any()
    assert (got[1][qs == UNSET] == -1).all() and (got[0][qs == UNSET] == fs.FLT_MAX).all()
    assert (got[1][qs == NONE] >= 0).all()


# ---- 2. Grouping -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pruning", [False, True], ids=["all", "pruned"])
@pytest.mark.parametrize("kw", GROUPING[:2], ids=lambda kw: "nsubc%d" % kw["nsubc"])
def test_grouping(gpu, kw, pruning):
    b = base(**kw)
    g, f, sets = two_handles(gpu, b)
    nprobe, mc, ef = fs.GROUPING_PARAMS
    q128 = fs.tiled(b["queries"], 128)
    for k in (1, 10):
        refs = fs.per_slot(fs.oracle_search(fs.GROUPING_PARAMS, k, pruning), b, sets, q128, k)
        for rep in ((1, 8) if k == 1 else (1,)):
            q = fs.tiled(q128, 128 * rep)
            qs = fs.query_slots(len(q))
            got = g.search_slots(q, k, qs, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=True)
            assert g.last_scan_kernel() == ("scan_k1_bitmap_kernel+slots" if k == 1 else "scan_topk_kernel+slots")
            counts = g.last_scan_counts()
            assert_same(got, fs.compose(refs, qs, np.arange(len(q)) % 128), (k, rep))
            f.search(q, k, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=True)
            assert counts == f.last_scan_counts()
        assert (got[1][qs == 0] >= 0).any() and (got[1][qs == UNSET] == -1).all()


# ---- 3. k > 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
def test_topk_both_orders(gpu, k):
    b = base(**BASE)
    g, f, sets = two_handles(gpu, b)
    q = b["queries"]
    qs = fs.query_slots(len(q))
    refs = fs.per_slot(fs.oracle_search(fs.IVF_PARAMS, k), b, sets, q, k)
    got = g.search_slots(q, k, qs, NPROBE, MAX_CODES, efSearch=EF, heap_order=True)
    assert g.last_scan_kernel() == "scan_topk_kernel+slots"
    assert_same(got, fs.compose(refs, qs), "heap order, oracle")  # faiss's heap array, element for element
    for heap in (True, False):
        hrefs = handle_per_slot(f, sets, len(q), k,
                                lambda h: h.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap))
        got = g.search_slots(q, k, qs, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
        assert_same(got, fs.compose(hrefs, qs), ("single filter", heap))
    if k == 100:  # 1 % of the ~2000 codes a query scans: the 1 % slot leaves places unfilled
        short = got[1][qs == 1]
        assert (short == -1).any() and (short >= 0).any()


def test_heap_scan_k2000(gpu):
    b = base(**BASE)
    g, f, sets = two_handles(gpu, b)
    nprobe, ef, k, mc = 64, 80, 2000, 10 ** 9
    q = b["queries"][:32]
    qs = fs.query_slots(32)
    refs = fs.per_slot(fs.oracle_search((nprobe, mc, ef), k), b, sets, q, k)
    assert ((refs[0][1] >= 0).sum(1) == k)[qs == 0].any(), "fixture: a query of slot 0 must admit more than k passing codes"
    got = g.search_slots(q, k, qs, nprobe, mc, efSearch=ef, heap_order=True)
    assert g.last_scan_kernel() == "heap_scan_kernel+slots"
    assert_same(got, fs.compose(refs, qs), "oracle")
    hrefs = handle_per_slot(f, sets, 32, k, lambda h: h.search(q, k, nprobe, mc, efSearch=ef, heap_order=True))
    assert_same(got, fs.compose(hrefs, qs), "single filter")


def _dev_search(g, q, k, qs, nprobe, max_codes, ef, heap=False, keys=False, stream=False):
    """search_slots_dev on device buffers: dict of dist, labels and, asked for, out_keys, stream lengths and streams."""
    import torch
    dev = torch.device("cuda", 0)
    nq = len(q)
    d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    d_s = None if qs is None else torch.from_numpy(np.ascontiguousarray(qs)).to(dev)
    dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ll = torch.empty((nq, k), dtype=torch.int64, device=dev)
    kk = torch.empty((nq, k), dtype=torch.int64, device=dev) if keys else None
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    g.search_slots_dev(nq, k, d_q, d_s, dd, ll, nprobe, max_codes, efSearch=ef, d_out_keys=kk, heap_order=heap)
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


def test_heap_redo_path(gpu):
    """The stream of the query on slot 31 overflows: heap_scan_kernel's per-query form redoes it, and resolves the plane of
    every listed query anew -- the same query beside it under NONE (overflows too) and on a slot that is not set."""
    from test_gpu_heap_unbounded import CAP
    b, q, qs, sets, (nprobe, max_codes, ef, k) = fs.redo_case(base)
    g = fs.install(_upload(gpu(), b), sets)
    refs = fs.per_slot(fs.oracle_search((nprobe, max_codes, ef), k), b, sets, q, k, slots=qs)
    r = _dev_search(g, q, k, qs, nprobe, max_codes, ef, heap=True, stream=True)
    assert r["kernel"] == "scan_topk_kernel+slots"
    assert r["len"][0] > CAP, "the stream must overflow for the redo path to run (length %d)" % r["len"][0]
    assert r["len"][2] == 0
    assert_same((r["dist"], r["labels"]), fs.compose(refs, qs))
    assert not np.isin(r["labels"][0], sets[31][0]).any() and np.isin(r["labels"][1], sets[31][0]).any()
    assert (r["labels"][2] == -1).all()


# ---- 4. keys and streams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,heap", [(1, False), (10, False), (10, True)])
def test_keys_and_streams(gpu, k, heap):
    """Keys, candidate streams and resolve_keys_dev of every query equal those of an unfiltered handle that uploaded the
    poisoned corpus of the query's slot."""
    b = base(**BASE)
    g, f, sets = two_handles(gpu, b)
    q = b["queries"]
    qs = fs.query_slots(len(q))
    a = _dev_search(g, q, k, qs, NPROBE, MAX_CODES, EF, heap=heap, keys=True, stream=heap)
    assert a["kernel"].endswith("+slots")
    for s in sorted(set(fs.PATTERN)):
        _upload(f, fs.slot_corpus(b, sets, s), graph=False)
        c = _dev_search(f, q, k, None, NPROBE, MAX_CODES, EF, heap=heap, keys=True, stream=heap)
        assert not c["kernel"].endswith("+slots")
        m = qs == s
        assert np.array_equal(a["keys"][m], c["keys"][m]), s
        assert _same_search((a["resolved"][0][m], a["resolved"][1][m]), (c["resolved"][0][m], c["resolved"][1][m])), s
        assert _same_search((a["dist"][m], a["labels"][m]), (c["dist"][m], c["labels"][m])), s
        if heap:
            assert np.array_equal(a["len"][m], c["len"][m]), s
            for i in np.nonzero(m)[0]:
                assert np.array_equal(a["stream"][i], c["stream"][i]), (s, i)
    lab = a["resolved"][1][qs == 31]
    assert np.isin(lab[lab >= 0], sets[31][0]).all() and (lab >= 0).any()


# ---- 5. split batch -------------------------------------------------------------------------------------------------------
def test_split_batch(gpu):
    b = base(**BASE)
    g, f, sets = two_handles(gpu, b)
    nq = 10240
    q = fs.tiled(b["queries"], nq)
    qs = fs.query_slots(nq)
    r = _dev_search(g, q, 1, qs, NPROBE, MAX_CODES, EF)
    assert g.last_batch_parts()[1] > 0, "the batch did not take the two-part path"
    assert g.last_batch_parts()[0] % 7 != 0  # the second part's slot bytes start inside the pattern
    assert r["kernel"] == "scan_k1_kernel+slots"
    small = [g.search_slots(q[i:i + 128], 1, qs[i:i + 128], NPROBE, MAX_CODES, efSearch=EF) for i in range(0, nq, 128)]
    want = (np.concatenate([s[0] for s in small]), np.concatenate([s[1] for s in small]))
    assert_same((r["dist"], r["labels"]), want)


# ---- 6. chunking ----------------------------------------------------------------------------------------------------------
def test_host_call_beyond_one_chunk(gpu):
    """One host call of more queries than a chunk holds (kMaxBatchAll = 1 << 17, capi_internal.h): every chunk reads its own
    slice of the slot bytes."""
    b = base(**BASE)
    g, f, sets = two_handles(gpu, b)
    period = 128 * 7
    nq = (1 << 17) + 3 * 128 + 5
    assert (1 << 17) % 7 != 0
    q896 = fs.tiled(b["queries"], period)
    small = g.search_slots(q896, 1, fs.query_slots(period), NPROBE, MAX_CODES, efSearch=EF)
    q = fs.tiled(q896, nq)
    got = g.search_slots(q, 1, fs.query_slots(nq), NPROBE, MAX_CODES, efSearch=EF)
    idx = np.arange(nq) % period
    assert_same(got, (small[0][idx], small[1][idx]))


# ---- 7. range search ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,params", [(BASE, fs.IVF_PARAMS), (GROUPING[1], fs.GROUPING_PARAMS)], ids=["ivfadc", "grouping"])
def test_range_search(gpu, kw, params):
    b = base(**kw)
    g, f, sets = two_handles(gpu, b)
    nprobe, mc, ef = params
    q = fs.tiled(b["queries"], 128)
    qs = fs.query_slots(len(q))
    nearest = f.search(q, 1, nprobe, mc, efSearch=ef)[0][:, 0]
    radius = float(np.median(nearest))  # half of the queries have their nearest code inside: filtered ones often nothing
    lims, dist, lab = g.range_search_slots(q, radius, qs, nprobe, mc, efSearch=ef)
    assert g.last_scan_kernel().endswith("+slots")
    assert len(lims) == len(q) + 1 and lims[0] == 0 and lims[-1] == len(dist) == len(lab)
    assert lims[-1] > 0
    sizes = np.diff(lims.astype(np.int64))
    assert any((sizes[qs == s] == 0).any() for s in fs.SPECS), "a query of a set slot must return nothing at this radius"
    assert (sizes[qs == UNSET] == 0).all()
    for s in sorted(set(fs.PATTERN)):
        mine = np.nonzero(qs == s)[0]
        if s == UNSET:
            continue
        if s == NONE:
            f.clear_filter()
        else:
            f.set_filter(sets[s][0], deny=sets[s][1])
        rl, rd, rb = f.range_search(q[mine], radius, nprobe, mc, efSearch=ef)
        for j, i in enumerate(mine):
            a0, a1, r0, r1 = int(lims[i]), int(lims[i + 1]), int(rl[j]), int(rl[j + 1])
            assert np.array_equal(lab[a0:a1], rb[r0:r1]), (s, i)
            assert np.array_equal(dist[a0:a1].view(np.uint32), rd[r0:r1].view(np.uint32)), (s, i)
    assert sizes[qs == 0].sum() > 0


# ---- 8. life cycle --------------------------------------------------------------------------------------------------------
def _plane_bytes(n):
    return 8 * max((n + 63) // 64, 1)


def test_set_twice_clear_and_upload(gpu):
    b = base(**BASE)
    n = len(b["ids"])
    g = _upload(gpu(), b)
    q = b["queries"]
    qs = fs.query_slots(len(q))
    before = g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
    kernel = g.last_scan_kernel()
    sets = fs.slot_sets(b)
    other = fs.slot_sets(b, seed=1)
    # memory_bytes follows the planes (measured around the calls, with no search in between: workspaces grow too)
    mem0 = g.memory_bytes()
    g.set_filter_slot(1, other[0][0])  # replaced below
    mem1 = g.memory_bytes()
    assert mem1 >= mem0 + 2 * _plane_bytes(n) + int(other[0][0].max()) // 8
    fs.install(g, sets)
    mem31 = g.memory_bytes()
    assert mem31 >= mem1 + 30 * _plane_bytes(n)
    g.clear_filter_slot(31)  # the last plane: the planes shrink to slot 7's
    g.clear_filter_slot(31)  # not set: succeeds
    assert g.filter_slot_info(31) == (-1, 0, n)
    mem7 = g.memory_bytes()
    assert mem7 <= mem31 - 24 * _plane_bytes(n) - int(sets[31][0].max()) // 8
    g.set_filter_slot(31, sets[31][0])
    assert g.memory_bytes() >= mem7 + 24 * _plane_bytes(n)
    f = _upload(gpu(), b)
    hrefs = handle_per_slot(f, sets, len(q), 1, lambda h: h.search(q, 1, NPROBE, MAX_CODES, efSearch=EF))
    assert_same(g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF), fs.compose(hrefs, qs), "after replacing slot 1")
    for s in range(32):
        rows = fs.passing_rows(b, sets, s)
        assert g.filter_slot_info(s) == ((1 if sets[s][1] else 0) if s in sets else -1, int(rows.sum()), n)
    # without slot 31 its queries find nothing, the others what they found
    g.clear_filter_slot(31)
    less = {s: v for s, v in sets.items() if s != 31}
    hrefs = handle_per_slot(f, less, len(q), 1, lambda h: h.search(q, 1, NPROBE, MAX_CODES, efSearch=EF))
    got = g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF)
    assert_same(got, fs.compose(hrefs, qs), "after clearing slot 31")
    assert (got[1][qs == 31] == -1).all()
    # plain calls never read slots
    assert _same_search(g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF), before) and g.last_scan_kernel() == kernel
    mem_a = g.memory_bytes()
    g.clear_filter_slot()
    assert g.memory_bytes() <= mem_a - 8 * _plane_bytes(n)
    assert all(g.filter_slot_info(s) == (-1, 0, n) for s in range(32))
    got = g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF)
    assert (got[1][qs != NONE] == -1).all()
    assert _same_search((got[0][qs == NONE], got[1][qs == NONE]), (before[0][qs == NONE], before[1][qs == NONE]))
    fs.install(g, sets)
    mem_a = g.memory_bytes()
    _upload(g, b, graph=False)
    assert all(g.filter_slot_info(s)[0] == -1 for s in range(32)) and g.memory_bytes() <= mem_a - 32 * _plane_bytes(n)


def test_dev_form_and_edge_labels(gpu):
    """set_filter_slot_dev equals the host form; labels 0xffffffff and above 2^31."""
    import torch
    b0 = base(**BASE)
    ids = b0["ids"].astype(np.uint64) * 3 + 0x80000011
    top = int(np.argmax(ids))
    ids[top] = 0xffffffff
    b = _with_ids(b0, ids)
    assert (b["ids"] > 2 ** 31).all() and (b["ids"] == 0xffffffff).sum() == 1
    sets = fs.slot_sets(b)
    sets[31] = (np.unique(np.concatenate([sets[31][0], [0xffffffff]])).astype(np.uint32), False)
    sets[7] = (np.unique(np.concatenate([sets[7][0], [0xffffffff]])).astype(np.uint32), True)
    a, f, _ = two_handles(gpu, b, sets)
    d = _upload(gpu(), b)
    dev = torch.device("cuda", 0)
    for s, (labels, deny) in sets.items():
        t = torch.from_numpy(labels.view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        d.set_filter_slot_dev(s, len(labels), t, deny=deny)
    d.set_filter_slot_dev(3, 0, None, deny=True)  # the empty deny set: everything passes
    a.set_filter_slot(3, np.zeros(0, np.uint32), deny=True)
    assert a.filter_slot_info(3) == d.filter_slot_info(3) == (1, len(ids), len(ids))
    q = b["queries"]
    qs = fs.query_slots(len(q))
    qs[::9] = 3
    for s in range(32):
        assert a.filter_slot_info(s) == d.filter_slot_info(s)
    assert a.filter_slot_info(31)[1] == len(sets[31][0]) and a.filter_slot_info(7)[1] == len(ids) - len(sets[7][0])
    for k, heap in ((1, False), (10, True)):
        got = a.search_slots(q, k, qs, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
        assert _same_search(got, d.search_slots(q, k, qs, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap))
        hrefs = handle_per_slot(f, {**sets, 3: (np.zeros(0, np.uint32), True)}, len(q), k,
                                lambda h: h.search(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap),
                                slots=set(qs.tolist()))
        assert_same(got, fs.compose(hrefs, qs), k)
    assert (got[1] > 2 ** 31).any()
    # the row labelled 0xffffffff: found on slot 31, which lists it, by the query nearest to it -- and not on slot 7, which denies it
    one = np.repeat(b0["base"][[int(b0["ids"][top])]], 2, axis=0).astype(np.float32)
    d1, l1 = a.search_slots(one, 1, np.array([31, 7], np.uint8), NPROBE, 10 ** 9, efSearch=EF)
    plain = a.search(one[:1], 1, NPROBE, 10 ** 9, efSearch=EF)[1][0, 0]
    assert plain != 0xffffffff or (l1[0, 0] == 0xffffffff and l1[1, 0] != 0xffffffff)


def test_user_view_answers_as_its_parent(gpu):
    b = base(**BASE)
    g, f, sets = two_handles(gpu, b)
    q = b["queries"]
    qs = fs.query_slots(len(q))
    v = g.view()
    assert v.filter_slot_info(31) == g.filter_slot_info(31)
    for k in (1, 10):
        assert _same_search(v.search_slots(q, k, qs, NPROBE, MAX_CODES, efSearch=EF),
                            g.search_slots(q, k, qs, NPROBE, MAX_CODES, efSearch=EF))
        assert v.last_scan_kernel().endswith("+slots")
    v.close()


def _check_against_fresh(gpu, g, cur, sets, upload=_upload, params=fs.IVF_PARAMS, prunings=(False,)):
    """g equals a fresh handle that uploaded the updated corpus and then set the same slots."""
    f = fs.install(upload(gpu(), cur), sets)
    n = len(cur["ids"])
    for s in range(32):
        want = (-1, 0, n)
        if s in sets:
            want = (1 if sets[s][1] else 0, int(filter_ref.passing(cur["ids"], sets[s][0], sets[s][1]).sum()), n)
        assert g.filter_slot_info(s) == f.filter_slot_info(s) == want, s
    q = cur["queries"]
    qs = fs.query_slots(len(q))
    for pruning in prunings:
        for k, heap in ((1, False), (10, True)):
            got = g.search_slots(q, k, qs, params[0], params[1], efSearch=params[2], do_pruning=pruning, heap_order=heap)
            assert g.last_scan_kernel().endswith("+slots")
            assert _same_search(got, f.search_slots(q, k, qs, params[0], params[1], efSearch=params[2], do_pruning=pruning,
                                                    heap_order=heap)), (pruning, k)
            for s, (labels, deny) in sets.items():
                lab = got[1][qs == s]
                assert (np.isin(lab[lab >= 0], labels) != deny).all(), s
    return got


def test_updates_keep_the_slots_ivf(gpu, pkg):
    import remove_ref
    from test_gpu_append import _csr_append
    b = base(**BASE)
    rng = np.random.default_rng(12)
    nc, M = b["nc"], b["code_size"]
    n = 3000
    new_ids = (np.arange(n) + 10 ** 6).astype(np.uint32)
    sets = fs.slot_sets(b)
    # rows to come: allowed by slot 0, denied by slot 7
    sets[0] = (np.concatenate([sets[0][0], new_ids[::2]]).astype(np.uint32), False)
    sets[7] = (np.concatenate([sets[7][0], new_ids[::3]]).astype(np.uint32), True)
    g = fs.install(_upload(gpu(), b), sets)
    # a failing update leaves every slot as it was
    info = [g.filter_slot_info(s) for s in range(32)]
    li = rng.integers(0, nc, n).astype(np.uint32)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    ncodes = rng.integers(0, 255, n).astype(np.uint8)
    bad = li.copy()
    bad[n // 2] = nc
    with pytest.raises(pkg.IvfHnswError) as e:
        g.append_ivf(bad, new_ids, codes, ncodes)
    assert e.value.code == pkg.ERR_INVALID
    assert [g.filter_slot_info(s) for s in range(32)] == info
    _check_against_fresh(gpu, g, b, sets)
    # append_ivf
    g.append_ivf(li, new_ids, codes, ncodes)
    lists = _csr_append((b["offsets"], b["ids"], b["codes"], b["norm_codes"]), nc, li, new_ids, codes, ncodes)
    cur = dict(b, offsets=lists[0], ids=lists[1], codes=lists[2], norm_codes=lists[3])
    got = _check_against_fresh(gpu, g, cur, sets)
    assert g.filter_slot_info(0)[1] == info[0][1] + len(new_ids[::2])
    # remove_ids (passing and non-passing rows alike)
    gone = rng.choice(cur["ids"], 5000, replace=False)
    assert g.remove_ids(gone)[0] == 5000
    cur, _ = remove_ref.filtered_corpus(cur, gone)
    _check_against_fresh(gpu, g, cur, sets)


def test_updates_keep_the_slots_grouping(gpu):
    import remove_ref
    import grouping_append_ref as gar
    import test_gpu_add_groups as tg
    params = (tg.NPROBE, tg.MAX_CODES, tg.EF)
    # remove_ids on a Grouping index
    c = base(**GROUPING[1])
    sets = fs.slot_sets(c)
    g = fs.install(_upload(gpu(), c), sets)
    gone = np.random.default_rng(15).choice(c["ids"], len(c["ids"]) // 4, replace=False)
    g.remove_ids(gone)
    cur, _ = remove_ref.filtered_corpus(c, gone)
    _check_against_fresh(gpu, g, cur, sets, params=fs.GROUPING_PARAMS, prunings=(False, True))
    # add_groups
    c, g0, groups, gone, rng = tg._group_case(tg.SHAPES[1], 21)
    full = tg._assemble(c, g0, groups)
    part, _ = gar.without_groups(full, gone)
    part["subgroup_sizes"][gone] = 0
    g = tg._upload_for_add(gpu, c, g0, part)
    sets = fs.slot_sets(full)
    fs.install(g, sets)
    tg._add_groups(g, groups, rng.permutation(np.nonzero(gone)[0]))
    tg._assert_state(g, full)
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    _check_against_fresh(gpu, g, dict(full, queries=c["queries"]), sets, upload=tg._upload, params=params,
                         prunings=(False, True))


# ---- 9. latency path ------------------------------------------------------------------------------------------------------
def test_latency_path(gpu):
    b = base(**BASE)
    g, f, sets = two_handles(gpu, b)
    g.prepare_latency()
    q = b["queries"][:4]
    qs = np.array([0, 31, 7, 1], np.uint8)
    plain = g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel() == "ivf_tail_kernel"
    refs = fs.per_slot(fs.oracle_search(fs.IVF_PARAMS, 1), b, sets, q, 1, slots=qs)
    got = g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel() == "scan_k1_kernel+slots"
    assert_same(got, fs.compose(refs, qs))
    assert _same_search(g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF), plain)
    assert g.last_scan_kernel() == "ivf_tail_kernel"
