"""Heap-order top-k without limits (heap_scan_kernel, kernels_heap.hip): any k, any number of admitted codes.

The reference returns the array faiss's max-heap leaves (IndexIVF_HNSW.cpp:265,285-288) for every k and however many
codes the heap admits.  A query whose candidate stream overflows its 8192 entries is redone from the plan and the
table; k > 1024 runs the heap scan alone (LDS heap, or a global one beyond what fits beside the table).  Labels and
distance bits are compared with the oracle's heap array, element for element.
"""
import numpy as np
import pytest
import torch

from conftest import corpus
import synth

pytestmark = pytest.mark.gpu

CAP = 8192  # candidate-stream entries per query of the heap-order replay (capi_internal.h kHeapStreamCap)
FLT_MAX = np.float32(3.4028234663852886e38)


def _upload(g, c):
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"], opq_A=c["opq_A"])
    if c["nsubc"]:
        g.upload_grouping(c["nsubc"], c["alphas"], c["nn_centroid_idxs"], c["subgroup_sizes"],
                          c["inter_centroid_dists"])
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)


def _assert_rows(dist, lab, ref_d, ref_l, what=""):
    for i in range(len(ref_l)):
        assert np.array_equal(lab[i], ref_l[i]), "%s query %d labels" % (what, i)
        assert np.array_equal(dist[i].view(np.uint32), ref_d[i].view(np.uint32)), "%s query %d distances" % (what, i)


def _adc_part(c, q, lo, hi):
    """The per-code part of the query's distance, norm - 2 <q, code> (approximately: only its order is used)."""
    M, d = c["code_size"], c["d"]
    x = q.astype(np.float64)
    if c["opq_A"] is not None:
        x = c["opq_A"].astype(np.float64) @ x
    tab = np.einsum("mjs,ms->mj", c["pq_centroids"].astype(np.float64), x.reshape(M, d // M))
    codes = c["codes"][lo:hi].reshape(hi - lo, M)
    ip = tab[np.arange(M)[None, :], codes].sum(1)
    return c["norm_table"][c["norm_codes"][lo:hi]].astype(np.float64) - 2.0 * ip


def _descending(c, q, lst):
    """Copy of the corpus with list `lst` rewritten (ids, codes, norm codes together) in descending order of the query's
    distance: scanned first, every one of its codes is admitted by the heap.  Grouping: the whole list becomes the one
    sub-group whose sub-centroid is nearest to the query (never pruned ahead of the others)."""
    c2 = dict(c)
    c2["ids"], c2["codes"], c2["norm_codes"] = c["ids"].copy(), c["codes"].copy(), c["norm_codes"].copy()
    lo, hi = int(c["offsets"][lst]), int(c["offsets"][lst + 1])
    order = lo + np.argsort(-_adc_part(c, q, lo, hi), kind="stable")
    for name in ("ids", "codes", "norm_codes"):
        c2[name][lo:hi] = c[name][order]
    if c["nsubc"]:
        cents = c["centroids"]
        sub = cents[lst][None, :] + c["alphas"][lst] * (cents[c["nn_centroid_idxs"][lst]] - cents[lst][None, :])
        s = int(((sub - q[None, :]) ** 2).sum(1).argmin())
        sg = c["subgroup_sizes"].copy()
        sg[lst] = 0
        sg[lst, s] = hi - lo
        c2["subgroup_sizes"] = sg
    return c2


def _overflow_corpus(kw, nprobe, ef):
    """(corpus, query index): the query whose first probed list is the largest, that list in descending order."""
    c = corpus(**kw)
    ox = synth.oracle_index(c)
    ox.set_params(nprobe, 10 ** 9, ef)
    _, _, cid, _, _ = ox.search_batch(c["queries"], k=1)
    sizes = np.diff(c["offsets"].astype(np.int64))
    qi = int(np.argmax(sizes[cid[:, 0]]))
    lst = int(cid[qi, 0])
    assert sizes[lst] > CAP + 500, "fixture: the first probed list must outgrow the stream"
    return _descending(c, c["queries"][qi], lst), qi


def _stream_lengths(g, q, k, nprobe, max_codes, ef, pruning, cid=None, cd=None):
    """search_dev in heap order on device buffers; the candidate-stream length of every query (last_stream_dev)."""
    dev = torch.device("cuda", 0)
    nq = len(q)
    d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    d_cid = None if cid is None else torch.from_numpy(cid.astype(np.int32)).to(dev)
    d_cd = None if cd is None else torch.from_numpy(cd).to(dev)
    dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ll = torch.empty((nq, k), dtype=torch.int64, device=dev)
    g.search_dev(nq, k, d_q, dd, ll, nprobe, max_codes, d_coarse_ids=d_cid, d_coarse_dists=d_cd,
                 efSearch=0 if cid is not None else ef, do_pruning=pruning, heap_order=True)
    ln = torch.empty((nq,), dtype=torch.int32, device=dev)
    cap = g.last_stream_dev(nq, d_len=ln)
    g.sync()
    assert cap == CAP
    return ln.cpu().numpy(), dd.cpu().numpy(), ll.cpu().numpy()


OVERFLOW = [  # (corpus, k, pruning)
    (dict(seed=301, nc=8, d=128, M=16, n_base=40000, nq=48, efConstruction=40), 2, False),
    (dict(seed=301, nc=8, d=128, M=16, n_base=40000, nq=48, efConstruction=40), 10, False),
    (dict(seed=301, nc=8, d=128, M=16, n_base=40000, nq=48, efConstruction=40), 1000, False),
    (dict(seed=302, nc=8, d=128, M=16, n_base=40000, nq=48, efConstruction=40, nsubc=4), 10, False),
    (dict(seed=302, nc=8, d=128, M=16, n_base=40000, nq=48, efConstruction=40, nsubc=4), 1000, True),
    (dict(seed=303, nc=8, d=128, M=16, n_base=40000, nq=48, efConstruction=40, opq=True), 10, False),
    (dict(seed=304, nc=8, d=128, M=64, n_base=40000, nq=48, efConstruction=40), 10, False),     # 64 KB table
    (dict(seed=305, nc=8, d=128, M=128, n_base=40000, nq=48, efConstruction=40), 1000, False),  # 128 KB table
    (dict(seed=306, nc=8, d=112, M=28, n_base=60000, nq=48, efConstruction=40), 100, False),    # run-time code size
]


def _ovf_id(case):
    kw, k, pruning = case
    kind = "grp" if kw.get("nsubc") else ("opq" if kw.get("opq") else "ivf")
    return "%s-M%d-k%d%s" % (kind, kw["M"], k, "-prune" if pruning else "")


@pytest.mark.parametrize("case", OVERFLOW, ids=_ovf_id)
def test_forced_overflow_equals_oracle_heap_array(gpu, case):
    """Every code of the query's first list is admitted: more than 8192 candidates.  Device walk and given coarse ids."""
    kw, k, pruning = case
    nprobe, max_codes, ef = 8, 20000, 16
    c, qi = _overflow_corpus(kw, nprobe, ef)
    ox = synth.oracle_index(c)
    ox.set_params(nprobe, max_codes, ef, do_pruning=pruning)
    q = c["queries"][[qi]]
    ref_d, ref_l, cid, cd, _ = ox.search_batch(q, k=k)
    g = gpu()
    _upload(g, c)
    ln, dd, ll = _stream_lengths(g, q, k, nprobe, max_codes, ef, pruning)
    assert ln[0] > CAP, "the stream must overflow for the redo path to run (length %d)" % ln[0]
    _assert_rows(dd, ll, ref_d, ref_l, "search_dev walk")
    d1, l1 = g.search(q, k, nprobe, max_codes, efSearch=ef, do_pruning=pruning, heap_order=True)
    _assert_rows(d1, l1, ref_d, ref_l, "walk")
    d2, l2 = g.search(q, k, nprobe, max_codes, coarse_ids=cid, coarse_dists=cd, do_pruning=pruning, heap_order=True)
    _assert_rows(d2, l2, ref_d, ref_l, "given coarse")


def test_mixed_batch_only_overflowing_queries_redone(gpu):
    kw = OVERFLOW[1][0]
    nprobe, max_codes, ef, k = 8, 20000, 16, 10
    c, qi = _overflow_corpus(kw, nprobe, ef)
    ox = synth.oracle_index(c)
    ox.set_params(nprobe, max_codes, ef)
    q = c["queries"]
    ref_d, ref_l, cid, cd, _ = ox.search_batch(q, k=k)
    g = gpu()
    _upload(g, c)
    ln, dd, ll = _stream_lengths(g, q, k, nprobe, max_codes, ef, False, cid, cd)
    over = ln > CAP
    assert over[qi] and over.sum() < len(q), "fixture: some queries overflow, the rest do not"
    _assert_rows(dd, ll, ref_d, ref_l, "mixed batch")
    # the rows that fit are what the unchanged path returns for a batch of those queries alone
    rest = np.nonzero(~over)[0]
    ln2, dd2, ll2 = _stream_lengths(g, q[rest], k, nprobe, max_codes, ef, False, cid[rest], cd[rest])
    assert (ln2 <= CAP).all()
    assert np.array_equal(ll2, ll[rest]) and np.array_equal(dd2.view(np.uint32), dd[rest].view(np.uint32))


BIG = [  # (corpus, k, queries): k > 1024; 17000 is beyond the LDS heap at PQ16 (the global tier)
    (dict(seed=11, nc=256, d=128, M=16, n_base=30000, nq=128), 1025, 48),
    (dict(seed=11, nc=256, d=128, M=16, n_base=30000, nq=128), 4096, 48),
    (dict(seed=11, nc=256, d=128, M=16, n_base=30000, nq=128), 17000, 4),
    (dict(seed=41, nc=256, d=128, M=16, n_base=30000, nq=96, nsubc=16), 1025, 48),
    (dict(seed=41, nc=256, d=128, M=16, n_base=30000, nq=96, nsubc=16), 4096, 48),
    (dict(seed=41, nc=256, d=128, M=16, n_base=30000, nq=96, nsubc=16), 17000, 4),
]


@pytest.mark.parametrize("case", BIG, ids=lambda cs: "%s-k%d" % ("grp" if cs[0].get("nsubc") else "ivf", cs[1]))
def test_k_above_1024_heap_order(gpu, case):
    kw, k, nq = case
    c = corpus(**kw)
    nprobe, max_codes, ef = 16, 6000, 40
    ox = synth.oracle_index(c)
    ox.set_params(nprobe, max_codes, ef, do_pruning=bool(c["nsubc"]))
    q = c["queries"][:nq]
    ref_d, ref_l, _, _, _ = ox.search_batch(q, k=k)
    g = gpu()
    _upload(g, c)
    dist, lab = g.search(q, k, nprobe, max_codes, efSearch=ef, do_pruning=bool(c["nsubc"]), heap_order=True)
    _assert_rows(dist, lab, ref_d, ref_l)
    if k == 17000:  # more slots than codes: the unfilled ones keep the heapify state
        assert (lab == -1).any()
        assert (dist[lab == -1] == FLT_MAX).all()
    with pytest.raises(RuntimeError):  # no candidate stream is left behind
        g.last_stream_dev(nq)


def test_k_above_1024_fewer_codes_than_k(gpu):
    c = corpus(seed=11, nc=256, d=128, M=16, n_base=30000, nq=128)
    sizes = np.diff(c["offsets"].astype(np.int64))
    small = int(np.argmin(np.where(sizes > 0, sizes, 10 ** 9)))
    g = gpu()
    _upload(g, c)
    cid = np.array([[small]], np.uint32)
    cd = np.array([[123.0]], np.float32)
    k = 1500
    ox = synth.oracle_index(c)
    ox.set_params(1, 10 ** 9, 16)
    ref_d, ref_l, _ = ox.search_coarse(c["queries"][0], cid, cd, k=k)
    dist, lab = g.search(c["queries"][:1], k, 1, 10 ** 9, coarse_ids=cid, coarse_dists=cd, heap_order=True)
    _assert_rows(dist, lab, ref_d.reshape(1, k), ref_l.reshape(1, k))
    n = int(sizes[small])
    assert (lab[0] == -1).sum() == k - n and (dist[0][lab[0] == -1] == FLT_MAX).all()


def test_k_above_1024_batch_slices(gpu):
    """More queries than one heap-order slice (2^14): three slices, rows at the boundaries and elsewhere exact."""
    c = corpus(seed=11, nc=256, d=128, M=16, n_base=30000, nq=128)
    rng = np.random.default_rng(5)
    nq, k = 2 * 16384 + 300, 1100
    src = rng.integers(0, len(c["queries"]), size=nq)
    q = (c["queries"][src] + rng.normal(0.0, 2.0, size=(nq, c["d"]))).astype(np.float32)
    nprobe, max_codes, ef = 4, 1500, 32
    g = gpu()
    _upload(g, c)
    dist, lab = g.search(q, k, nprobe, max_codes, efSearch=ef, heap_order=True)
    check = np.unique(np.concatenate([[0, 1, 16383, 16384, 16385, 32767, 32768, 32769, nq - 1],
                                      rng.integers(0, nq, size=40)]))
    ox = synth.oracle_index(c)
    ox.set_params(nprobe, max_codes, ef)
    ref_d, ref_l, _, _, _ = ox.search_batch(q[check], k=k, nthreads=8)
    _assert_rows(dist[check], lab[check], ref_d, ref_l, "sliced")


def test_reference_preset_orca_nprobe20(gpu):
    """examples/run_sift1b_orca_nprobe20.sh: k = 100, nprobe 20, max_codes 30000, efSearch 100, code size 64 (the
    run-time code-size scan); the 20 probed lists hold more than 30000 codes, so max_codes bites."""
    c = corpus(seed=307, nc=40, d=128, M=64, n_base=80000, nq=64, efConstruction=120)
    nprobe, max_codes, ef, k = 20, 30000, 100, 100
    ox = synth.oracle_index(c)
    ox.set_params(nprobe, max_codes, ef)
    ref_d, ref_l, cid, _, st = ox.search_batch(c["queries"], k=k)
    sizes = np.diff(c["offsets"].astype(np.int64))
    assert (sizes[cid.astype(np.int64)].sum(1) > max_codes).mean() > 0.9, "fixture: max_codes must bite"
    g = gpu()
    _upload(g, c)
    dist, lab = g.search(c["queries"], k, nprobe, max_codes, efSearch=ef, heap_order=True)
    _assert_rows(dist, lab, ref_d, ref_l)


@pytest.mark.parametrize("what", ["k2000", "overflow-k10"])
def test_class_surface_unbounded_heap(tmp_path, what):
    """search() one query per call and search_batch() through the classes (tests/cpp/hostlib_tool.bin)."""
    from test_host_library import _class_search
    if what == "k2000":
        c = synth.make_corpus(seed=71, nc=128, d=128, M=16, n_base=8000, nq=32, efConstruction=80)
        nprobe, max_codes, ef, k = 8, 1500, 32, 2000
    else:
        c, qi = _overflow_corpus(OVERFLOW[1][0], 8, 16)
        c = dict(c, queries=c["queries"][np.unique(np.r_[qi, np.arange(15)])])
        nprobe, max_codes, ef, k = 8, 20000, 16, 10
    ox = synth.oracle_index(c)
    ox.set_params(nprobe, max_codes, ef)
    ref_d, ref_l, _, _, _ = ox.search_batch(c["queries"], k=k)
    lab, dist = _class_search(tmp_path, c, nprobe, max_codes, ef, False, k=k)
    for mode in (0, 1):  # search() per query, search_batch()
        _assert_rows(dist[mode], lab[mode], ref_d, ref_l, "mode %d" % mode)
