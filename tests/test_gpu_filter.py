"""Label filter of a handle (ivfhnsw_gpu_set_filter).

Expected values come from the poisoned corpus of filter_ref: (A) the oracle's search of it, (B) an unfiltered search of an
upload of it on a second handle.  Labels and distance bits are compared exactly; last_scan_kernel proves that the
filtered form of the expected scan kernel ran."""
import numpy as np
import pytest

from conftest import corpus
import filter_ref
import synth
from test_gpu_remove import BASE, CODE_SIZES, _upload, _same_search, _with_ids

pytestmark = pytest.mark.gpu

NPROBE, MAX_CODES, EF = 16, 2000, 40
FLT_MAX = np.finfo(np.float32).max
GROUPING = dict(seed=43, nc=256, d=96, M=16, n_base=20000, nq=64, nsubc=8)  # mean sub-group 9.8 codes: the bitmap scan

_CLIPPED = {}


def base(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _CLIPPED:
        _CLIPPED[key] = filter_ref.clipped(corpus(**kw))
    return _CLIPPED[key]


def allow_set(b, frac, seed=0):
    return np.random.default_rng(seed).choice(b["ids"], int(frac * len(b["ids"])), replace=False).astype(np.uint32)


def tiled(q, n):
    return np.ascontiguousarray(np.tile(q, ((n + len(q) - 1) // len(q), 1))[:n])


def same_bits(got, ref_d, ref_l):
    return np.array_equal(got[1], ref_l.reshape(got[1].shape)) and \
        np.array_equal(got[0].view(np.uint32), ref_d.reshape(got[0].shape).view(np.uint32))


def pair(gpu, b, labels, deny=False):
    """(filtered handle on b, unfiltered handle on the poisoned corpus, that corpus)."""
    rows = filter_ref.passing(b["ids"], labels, deny)
    p = filter_ref.poisoned(b, rows)
    g = _upload(gpu(), b)
    g.set_filter(labels, deny=deny)
    assert g.filter_info() == (1 if deny else 0, int(rows.sum()), len(rows))
    return g, _upload(gpu(), p), p


# ---- 1. code sizes, both k = 1 forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CODE_SIZES, ids=lambda kw: "M%d" % kw["M"])
@pytest.mark.parametrize("frac", [0.5, 0.1, 0.01, 0.0])
def test_k1_code_sizes(gpu, kw, frac):
    b = base(**kw)
    g, f, p = pair(gpu, b, allow_set(b, frac, seed=kw["M"]))
    q128 = tiled(b["queries"], 128)
    ox = synth.oracle_index(p)
    ox.set_params(NPROBE, MAX_CODES, EF)
    ref = ox.search_batch(q128, k=1)
    plain = "scan_k1_kernel" if kw["M"] in (8, 16, 32) else "scan_k1_kernel (run-time code size)"
    for rep in (1, 8):  # 128 queries: several workgroups per query; 1024: one, which resolves the label itself
        q = tiled(q128, 128 * rep)
        got = g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
        assert g.last_scan_kernel() == plain + "+filter"
        counts = g.last_scan_counts()
        assert same_bits(got, np.tile(ref[0], (rep, 1)), np.tile(ref[1], (rep, 1))), (rep, "oracle")
        assert _same_search(got, f.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)), (rep, "poisoned upload")
        assert f.last_scan_kernel() == plain
        assert counts == f.last_scan_counts() and counts[0] == ref[4].ncode * rep
    if frac == 0.0:
        assert (got[1] == -1).all() and (got[0] == FLT_MAX).all()
    else:
        assert (got[1] >= 0).any()


# ---- 2. deny ---------------------------------------------------------------------------------------------------------
def test_deny_complement_equals_allow(gpu):
    b = base(**BASE)
    allow = allow_set(b, 0.1, seed=2)
    rest = np.setdiff1d(b["ids"], allow).astype(np.uint32)
    a = _upload(gpu(), b)
    a.set_filter(allow)
    d = _upload(gpu(), b)
    d.set_filter(rest, deny=True)
    assert a.filter_info()[1:] == d.filter_info()[1:] == (len(allow), len(b["ids"]))
    for k, heap in ((1, False), (10, True)):
        assert _same_search(a.search(b["queries"], k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap),
                            d.search(b["queries"], k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap))
    # the empty sets: allow nothing, deny nothing
    a.set_filter(np.zeros(0, np.uint32))
    assert a.filter_info() == (0, 0, len(b["ids"]))
    assert (a.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF)[1] == -1).all()
    d.set_filter(np.zeros(0, np.uint32), deny=True)
    assert d.filter_info() == (1, len(b["ids"]), len(b["ids"]))
    got = d.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF)
    assert d.last_scan_kernel().endswith("+filter")
    d.clear_filter()
    assert _same_search(got, d.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF))


# ---- 3. Grouping -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pruning", [False, True], ids=["all", "pruned"])
@pytest.mark.parametrize("frac", [0.5, 0.1, 0.01, 0.0])
def test_grouping(gpu, pruning, frac):
    b = base(**GROUPING)
    g, f, p = pair(gpu, b, allow_set(b, frac, seed=3))
    ox = synth.oracle_index(p)
    ox.set_params(NPROBE, MAX_CODES, 64, do_pruning=pruning)
    q128 = tiled(b["queries"], 128)
    for k in (1, 10):
        ref = ox.search_batch(q128, k=k)
        for rep in ((1, 8) if k == 1 else (1,)):
            q = tiled(q128, 128 * rep)
            got = g.search(q, k, NPROBE, MAX_CODES, efSearch=64, do_pruning=pruning, heap_order=True)
            assert g.last_scan_kernel() == ("scan_k1_bitmap_kernel+filter" if k == 1 else "scan_topk_kernel+filter")
            counts = g.last_scan_counts()
            assert same_bits(got, np.tile(ref[0], (rep, 1)), np.tile(ref[1], (rep, 1))), (k, rep)
            assert _same_search(got, f.search(q, k, NPROBE, MAX_CODES, efSearch=64, do_pruning=pruning, heap_order=True))
            assert counts == f.last_scan_counts()
        if k == 10 and frac == 0.01:
            filled = (got[1] >= 0).sum(1)
            assert (filled < 10).any()  # short results are reached


# ---- 4. k > 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("frac", [0.5, 0.01])
def test_topk_both_orders(gpu, k, frac):
    b = base(**BASE)
    g, f, p = pair(gpu, b, allow_set(b, frac, seed=4))
    ox = synth.oracle_index(p)
    ox.set_params(NPROBE, MAX_CODES, EF)
    ref = ox.search_batch(b["queries"], k=k)
    got = g.search(b["queries"], k, NPROBE, MAX_CODES, efSearch=EF, heap_order=True)
    assert g.last_scan_kernel() == "scan_topk_kernel+filter"
    assert same_bits(got, ref[0], ref[1])  # faiss's heap array, element for element
    assert _same_search(got, f.search(b["queries"], k, NPROBE, MAX_CODES, efSearch=EF, heap_order=True))
    asc = g.search(b["queries"], k, NPROBE, MAX_CODES, efSearch=EF)
    assert _same_search(asc, f.search(b["queries"], k, NPROBE, MAX_CODES, efSearch=EF))
    # ascending: the same k results (test_gpu_topk's comparison); unfilled slots sort last on both sides
    assert np.array_equal(asc[0].view(np.uint32), np.sort(ref[0], axis=1).view(np.uint32))
    for i in range(len(asc[1])):
        assert sorted(asc[1][i]) == sorted(ref[1][i])
    if frac == 0.01:
        assert (asc[1] == -1).any() and (asc[0][asc[1] == -1] == FLT_MAX).all()


def test_heap_scan_k2000(gpu):
    b = base(**BASE)
    g, f, p = pair(gpu, b, allow_set(b, 0.5, seed=5))
    nprobe, ef, k, mc = 64, 80, 2000, 10 ** 9
    ox = synth.oracle_index(p)
    ox.set_params(nprobe, mc, ef)
    q = b["queries"][:32]
    ref = ox.search_batch(q, k=k)
    assert ((ref[1] >= 0).sum(1) == k).any(), "fixture: some query must admit more than k passing codes"
    got = g.search(q, k, nprobe, mc, efSearch=ef, heap_order=True)
    assert g.last_scan_kernel() == "heap_scan_kernel+filter"
    assert same_bits(got, ref[0], ref[1])
    assert _same_search(got, f.search(q, k, nprobe, mc, efSearch=ef, heap_order=True))
    assert f.last_scan_kernel() == "heap_scan_kernel"


def test_heap_redo_path(gpu):
    """A candidate stream that overflows with the filter installed: heap_scan_kernel's filtered form redoes the query."""
    from test_gpu_heap_unbounded import OVERFLOW, CAP, _descending, _stream_lengths
    nprobe, max_codes, ef, k = 8, 20000, 16, 10
    c = base(**OVERFLOW[1][0])
    ox = synth.oracle_index(c)
    ox.set_params(nprobe, 10 ** 9, ef)
    cid = ox.search_batch(c["queries"], k=1)[2]
    sizes = np.diff(c["offsets"].astype(np.int64))
    qi = int(np.argmax(sizes[cid[:, 0]]))
    lst = int(cid[qi, 0])
    lo, hi = int(c["offsets"][lst]), int(c["offsets"][lst + 1])
    deny = c["ids"][lo:hi][::37].copy()  # 2.7 % of the query's first list
    assert (hi - lo) - len(deny) > CAP + 200, "fixture: the passing rows of the first probed list must outgrow the stream"
    b = _descending(c, c["queries"][qi], lst)  # that list in descending order of distance: every passing row is admitted
    p = filter_ref.poisoned(b, filter_ref.passing(b["ids"], deny, deny=True))
    g = _upload(gpu(), b)
    g.set_filter(deny, deny=True)
    q = b["queries"][[qi]]
    ox = synth.oracle_index(p)
    ox.set_params(nprobe, max_codes, ef)
    ref = ox.search_batch(q, k=k)
    ln, dd, ll = _stream_lengths(g, q, k, nprobe, max_codes, ef, False)
    assert ln[0] > CAP, "the stream must overflow for the redo path to run (length %d)" % ln[0]
    assert same_bits((dd, ll), ref[0], ref[1])
    assert not np.isin(ll, deny).any()


# ---- 5. keys and streams ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,heap", [(1, False), (10, False), (10, True)])
def test_keys_and_streams(gpu, k, heap):
    import torch
    b = base(**BASE)
    g, f, p = pair(gpu, b, allow_set(b, 0.1, seed=6))
    dev = torch.device("cuda", 0)
    q = b["queries"]
    nq = len(q)
    d_q = torch.from_numpy(q).to(dev)
    out = []
    for h in (g, f):
        dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
        ll = torch.empty((nq, k), dtype=torch.int64, device=dev)
        kk = torch.empty((nq, k), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)  # the handle's stream is not torch's
        h.search_dev(nq, k, d_q, dd, ll, NPROBE, MAX_CODES, efSearch=EF, d_out_keys=kk, heap_order=heap)
        h.sync()
        r = dict(keys=kk.cpu().numpy(), kernel=h.last_scan_kernel())
        if heap:
            ln = torch.empty((nq,), dtype=torch.int32, device=dev)
            cap = h.last_stream_dev(nq, d_len=ln)
            h.sync()
            L = max(1, int(ln.max().item()))
            assert L <= cap
            st = torch.zeros((nq, L), dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            h.last_stream_dev(nq, L, d_keys=st)
            h.sync()
            r["len"] = ln.cpu().numpy()
            st = st.cpu().numpy()
            r["stream"] = [st[i, :r["len"][i]] for i in range(nq)]
        d2 = torch.empty((nq, k), dtype=torch.float32, device=dev)
        l2 = torch.empty((nq, k), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        h.resolve_keys_dev(nq, k, kk, d2, l2)
        h.sync()
        r["resolved"] = (d2.cpu().numpy(), l2.cpu().numpy())
        out.append(r)
    a, c = out
    assert a["kernel"].endswith("+filter") and not c["kernel"].endswith("+filter")
    assert np.array_equal(a["keys"], c["keys"])
    assert _same_search(a["resolved"], c["resolved"])
    lab = a["resolved"][1]
    assert np.isin(lab[lab >= 0], allow_set(b, 0.1, seed=6)).all()
    if heap:
        assert np.array_equal(a["len"], c["len"])
        for x, y in zip(a["stream"], c["stream"]):
            assert np.array_equal(x, y)


# ---- 6. split batch -------------------------------------------------------------------------------------------------------
def test_split_batch(gpu):
    import torch
    b = base(**BASE)
    g, f, p = pair(gpu, b, allow_set(b, 0.1, seed=7))
    small = g.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF)
    q = tiled(b["queries"], 8192)
    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(q).to(dev)
    dd = torch.empty((len(q), 1), dtype=torch.float32, device=dev)
    ll = torch.empty((len(q), 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    g.search_dev(len(q), 1, d_q, dd, ll, NPROBE, MAX_CODES, efSearch=EF)
    g.sync()
    assert g.last_batch_parts()[1] > 0, "the batch did not take the two-part path"
    assert g.last_scan_kernel() == "scan_k1_kernel+filter"
    rep = len(q) // len(b["queries"])
    assert same_bits((dd.cpu().numpy(), ll.cpu().numpy()), np.tile(small[0], (rep, 1)), np.tile(small[1], (rep, 1)))


# ---- 7. edge labels -------------------------------------------------------------------------------------------------------
def _edge_case(gpu, b, labels, deny=False):
    g, f, p = pair(gpu, b, labels, deny)  # filter_info against numpy's count is asserted in pair
    for k, heap in ((1, False), (10, True)):
        got = g.search(b["queries"], k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
        assert _same_search(got, f.search(b["queries"], k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap))
    return g, got


def test_ids_above_2_31(gpu):
    b0 = base(**BASE)
    b = _with_ids(b0, b0["ids"].astype(np.uint64) * 3 + 0x80000011)
    labels = np.random.default_rng(3).choice(b["ids"], 6000, replace=False)
    _, got = _edge_case(gpu, b, labels)
    assert (got[1] > 2 ** 31).any()
    _edge_case(gpu, b, labels, deny=True)


@pytest.mark.parametrize("listed", [True, False])
@pytest.mark.parametrize("deny", [False, True])
def test_id_0xffffffff(gpu, listed, deny):
    b0 = base(**BASE)
    ox = synth.oracle_index(b0)
    ox.set_params(NPROBE, MAX_CODES, EF)
    top = int(ox.search_batch(b0["queries"][:1], k=1)[1][0, 0])  # query 0's nearest: the nearest of any set that holds it
    assert top >= 0
    ids = b0["ids"].copy()
    ids[ids == top] = 0xffffffff
    b = _with_ids(b0, ids)
    labels = allow_set(b0, 0.2, seed=8)
    labels = np.concatenate([labels[labels != top], [0xffffffff] if listed else []]).astype(np.uint32)
    g, _ = _edge_case(gpu, b, labels, deny)
    d1, l1 = g.search(b["queries"][:1], 1, NPROBE, MAX_CODES, efSearch=EF)
    assert (l1[0, 0] == 0xffffffff) == (listed != deny)


def test_label_in_many_lists_repeated_and_absent(gpu):
    b0 = base(**BASE)
    b = _with_ids(b0, b0["ids"] % 700)
    pick = np.array([0, 5, 77, 699, 123456, 0xfffffff0], np.uint32)  # two labels no row holds
    labels = np.concatenate([pick, pick[::2], pick, np.arange(100, 400, dtype=np.uint32)])
    g, _ = _edge_case(gpu, b, labels)
    assert g.filter_info()[1] == int(np.isin(b["ids"], labels).sum()) > 300 * 40
    _edge_case(gpu, b, labels, deny=True)


def test_last_word_and_unaligned_list_ends(gpu):
    b = base(**BASE)
    off = b["offsets"].astype(np.int64)
    n = len(b["ids"])
    assert n % 64 != 0
    lens = np.diff(off)
    cand = np.nonzero((off[:-1] % 64 != 0) & (lens > 1))[0]
    ox = synth.oracle_index(b)
    ox.set_params(NPROBE, MAX_CODES, EF)
    cid = ox.search_batch(b["queries"], k=1)[2]
    lst = int([c for c in cid[:, 0] if c in cand][0])  # a probed list whose start is not 64-aligned
    rows = np.array([off[lst], off[lst + 1] - 1, n - 1])
    labels = b["ids"][rows]
    g, got = _edge_case(gpu, b, labels)
    assert g.filter_info()[1] == 3
    assert np.isin(labels[:2], got[1]).all()  # first and last row of that list are found
    # everything but those rows
    g2, got2 = _edge_case(gpu, b, labels, deny=True)
    assert not np.isin(got2[1], labels).any()
    # the last row alone passes: whoever probes its list finds it, nobody finds anything else
    g3, got3 = _edge_case(gpu, b, labels[2:])
    assert set(np.unique(got3[1])) <= {-1, int(labels[2])}


# ---- 8. lifecycle ---------------------------------------------------------------------------------------------------------
def test_set_twice_clear_and_upload(gpu):
    b = base(**BASE)
    g = _upload(gpu(), b)
    before = g.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF)
    kernel = g.last_scan_kernel()
    mem0 = g.memory_bytes()
    first, second = allow_set(b, 0.5, seed=9), allow_set(b, 0.1, seed=10)
    g.set_filter(first)
    g.set_filter(second)
    f = _upload(gpu(), filter_ref.poisoned(b, filter_ref.passing(b["ids"], second)))
    assert _same_search(g.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF),
                        f.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF))
    assert g.filter_info() == (0, len(second), len(b["ids"]))
    assert g.memory_bytes() >= mem0 + (len(b["ids"]) + 7) // 8 + int(second.max()) // 8
    g.clear_filter()
    g.clear_filter()  # no filter: succeeds
    assert g.filter_info() == (-1, len(b["ids"]), len(b["ids"]))
    assert _same_search(g.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF), before)
    assert g.last_scan_kernel() == kernel
    g.set_filter(first)
    _upload(g, b, graph=False)
    assert g.filter_info()[0] == -1
    assert _same_search(g.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF), before)


def test_dev_form_equals_host_form(gpu):
    import torch
    b = base(**BASE)
    labels = allow_set(b, 0.1, seed=11)
    a = _upload(gpu(), b)
    a.set_filter(labels, deny=True)
    d = _upload(gpu(), b)
    dev = torch.device("cuda", 0)
    d_lab = torch.from_numpy(labels.view(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    d.set_filter_dev(len(labels), d_lab, deny=True)
    assert a.filter_info() == d.filter_info()
    assert _same_search(a.search(b["queries"], 10, NPROBE, MAX_CODES, efSearch=EF),
                        d.search(b["queries"], 10, NPROBE, MAX_CODES, efSearch=EF))
    d.set_filter_dev(0, None)
    assert d.filter_info() == (0, 0, len(b["ids"]))


def _check_against_fresh(gpu, g, cur, deny, params=(NPROBE, MAX_CODES, EF), pruning=False):
    """g equals a fresh handle that uploaded the updated corpus and then set the same filter."""
    f = _upload(gpu(), cur)
    f.set_filter(deny, deny=True)
    assert g.filter_info() == f.filter_info() == (1, int((~np.isin(cur["ids"], deny)).sum()), len(cur["ids"]))
    for k, heap in ((1, False), (10, True)):
        got = g.search(cur["queries"], k, params[0], params[1], efSearch=params[2], do_pruning=pruning, heap_order=heap)
        assert g.last_scan_kernel().endswith("+filter")
        assert _same_search(got, f.search(cur["queries"], k, params[0], params[1], efSearch=params[2], do_pruning=pruning,
                                          heap_order=heap))
        assert not np.isin(got[1], deny).any()
    return f


def test_updates_keep_the_filter_ivf(gpu):
    import remove_ref
    from test_gpu_append import _csr_append
    b = base(**BASE)
    rng = np.random.default_rng(12)
    nc, M = b["nc"], b["code_size"]
    n = 3000
    new_ids = (np.arange(2 * n) + 10 ** 6).astype(np.uint32)
    deny = np.concatenate([allow_set(b, 0.3, seed=13), new_ids[::2]]).astype(np.uint32)  # half of the rows to come, too
    g = _upload(gpu(), b)
    g.upload_codebooks(b["d"], M, b["pq_centroids"], b["norm_table"])
    g.set_filter(deny, deny=True)
    # append_ivf
    li = rng.integers(0, nc, n).astype(np.uint32)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    ncodes = rng.integers(0, 255, n).astype(np.uint8)
    g.append_ivf(li, new_ids[:n], codes, ncodes)
    lists = _csr_append((b["offsets"], b["ids"], b["codes"], b["norm_codes"]), nc, li, new_ids[:n], codes, ncodes)
    cur = dict(b, offsets=lists[0], ids=lists[1], codes=lists[2], norm_codes=lists[3])
    _check_against_fresh(gpu, g, cur, deny)
    # remove_ids (denied and passing rows alike)
    gone = rng.choice(cur["ids"], 5000, replace=False)
    assert g.remove_ids(gone)[0] == 5000
    cur, _ = remove_ref.filtered_corpus(cur, gone)
    _check_against_fresh(gpu, g, cur, deny)
    # add
    x = b["base"][:n] + rng.normal(0, 3.0, (n, b["d"])).astype(np.float32)
    idx, codes, ncodes = g.add(x, new_ids[n:], efSearch=EF)
    lists = _csr_append((cur["offsets"], cur["ids"], cur["codes"], cur["norm_codes"]), nc, idx, new_ids[n:], codes, ncodes)
    cur = dict(cur, offsets=lists[0], ids=lists[1], codes=lists[2], norm_codes=lists[3])
    _check_against_fresh(gpu, g, cur, deny)


def test_updates_keep_the_filter_grouping(gpu):
    import grouping_append_ref as gar
    import test_gpu_add_groups as tg
    # append_grouping
    c = corpus(**tg.SHAPES[1])
    rng = np.random.default_rng(14)
    part, batch = gar.split_corpus(c, gar.tail_mask(c, rng))
    deny = rng.choice(c["ids"], len(c["ids"]) // 3, replace=False).astype(np.uint32)
    g = tg._upload(gpu(), part)
    g.set_filter(deny, deny=True)
    tg._append(g, batch)
    tg._assert_state(g, c)
    f = tg._upload(gpu(), c)
    f.set_filter(deny, deny=True)
    assert g.filter_info() == f.filter_info() == (1, int((~np.isin(c["ids"], deny)).sum()), len(c["ids"]))
    for pruning in (False, True):
        for k in (1, 10):
            got = g.search(c["queries"], k, tg.NPROBE, tg.MAX_CODES, efSearch=tg.EF, do_pruning=pruning, heap_order=True)
            assert g.last_scan_kernel().endswith("+filter")
            assert _same_search(got, f.search(c["queries"], k, tg.NPROBE, tg.MAX_CODES, efSearch=tg.EF, do_pruning=pruning,
                                              heap_order=True))
            assert not np.isin(got[1], deny).any()
    # add_groups
    c, g0, groups, gone, rng = tg._group_case(tg.SHAPES[1], 21)
    full = tg._assemble(c, g0, groups)
    part, _ = gar.without_groups(full, gone)
    part["subgroup_sizes"][gone] = 0
    g = tg._upload_for_add(gpu, c, g0, part)
    deny = rng.choice(full["ids"], len(full["ids"]) // 3, replace=False).astype(np.uint32)
    g.set_filter(deny, deny=True)
    tg._add_groups(g, groups, rng.permutation(np.nonzero(gone)[0]))
    tg._assert_state(g, full)
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    f = tg._upload(gpu(), full)
    f.set_filter(deny, deny=True)
    assert g.filter_info() == f.filter_info() == (1, int((~np.isin(full["ids"], deny)).sum()), len(full["ids"]))
    for pruning in (False, True):
        got = g.search(c["queries"], 10, tg.NPROBE, tg.MAX_CODES, efSearch=tg.EF, do_pruning=pruning)
        assert _same_search(got, f.search(c["queries"], 10, tg.NPROBE, tg.MAX_CODES, efSearch=tg.EF, do_pruning=pruning))
        assert not np.isin(got[1], deny).any()


# ---- 9. latency path ------------------------------------------------------------------------------------------------------
def test_latency_path(gpu):
    b = base(**BASE)
    labels = allow_set(b, 0.1, seed=15)
    p = filter_ref.poisoned(b, filter_ref.passing(b["ids"], labels))
    g = _upload(gpu(), b)
    g.prepare_latency()
    q = b["queries"][:4]
    plain = g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel() == "ivf_tail_kernel"
    g.set_filter(labels)
    ox = synth.oracle_index(p)
    ox.set_params(NPROBE, MAX_CODES, EF)
    ref = ox.search_batch(q, k=1)
    got = g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
    assert g.last_scan_kernel() == "scan_k1_kernel+filter"
    assert same_bits(got, ref[0], ref[1])
    g.clear_filter()
    assert _same_search(g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF), plain)
    assert g.last_scan_kernel() == "ivf_tail_kernel"


def test_user_view_filters_as_its_parent_did(gpu):
    b = base(**BASE)
    labels = allow_set(b, 0.1, seed=16)
    g = _upload(gpu(), b)
    g.set_filter(labels)
    v = g.view()
    assert v.filter_info() == g.filter_info()
    assert _same_search(v.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF),
                        g.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF))
    assert v.last_scan_kernel().endswith("+filter")
    v.close()
