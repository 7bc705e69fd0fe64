"""Range search of a handle (ivfhnsw_gpu_range_search): lims, label sequence and distance bits are
compared exactly with range_ref (the oracle's scored set, IVFADC scan order restated in numpy)."""
import ctypes as C

import numpy as np
import pytest

from conftest import corpus
import range_ref
import synth
from test_gpu_remove import BASE, CODE_SIZES, _upload, _with_ids
from test_gpu_filter import GROUPING, NPROBE, MAX_CODES, EF, tiled

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
QUANTILES = (0.0005, 0.01, 0.1)


def scored(kw, nprobe=NPROBE, max_codes=MAX_CODES, ef=EF, pruning=False, nq=None):
    c = corpus(**kw)
    q = c["queries"] if nq is None else c["queries"][:nq]
    key = (tuple(sorted(kw.items())), nprobe, max_codes, ef, pruning, nq)
    return c, range_ref.scored_batch(c, q, nprobe, max_codes, ef, pruning, key=key)


def radii(sc):
    return [range_ref.pooled_quantile(sc, x) for x in QUANTILES] + [INF]


def expand(res, idx):
    """The result of the batch whose query j is query idx[j] of `res`."""
    lims, dist, lab = res
    lims = np.asarray(lims, np.int64)
    per = (lims[1:] - lims[:-1])[idx]
    pos = np.concatenate([np.arange(lims[i], lims[i + 1]) for i in idx]) if len(idx) else np.zeros(0, np.int64)
    return np.concatenate([[0], np.cumsum(per)]).astype(np.uint64), dist[pos], lab[pos]


def rs(g, q, r, nprobe=NPROBE, max_codes=MAX_CODES, ef=EF, **kw):
    return g.range_search(q, r, nprobe, max_codes, efSearch=ef, **kw)


# ---- 1. code sizes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CODE_SIZES, ids=lambda kw: "M%d" % kw["M"])
def test_code_sizes(gpu, kw):
    c, sc = scored(kw)
    nqu = len(c["queries"])
    g = _upload(gpu(), c)
    name = "range_scan_kernel" if kw["M"] in (8, 16, 32) else "range_scan_kernel (run-time code size)"
    low = None
    for r in radii(sc):
        want = range_ref.expected_ivf(c, sc, MAX_CODES, r)
        for n in (128, 1024):  # several slices per query; one
            idx = np.arange(n) % nqu
            q = np.ascontiguousarray(c["queries"][idx])
            got = rs(g, q, r)
            assert g.last_scan_kernel() == name
            assert range_ref.same_range(got, expand(want, idx)), (float(r), n)
            if r == INF:
                assert np.array_equal(np.diff(got[0].astype(np.int64)), sc["ncode"][idx])
                counts = g.last_scan_counts()
                g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
                assert counts == g.last_scan_counts() and counts[0] == sc["ncode"][idx].sum()
        if low is None:
            low = np.diff(want[0].astype(np.int64))
    if kw is BASE:
        assert (low == 0).any() and (low > 0).any()  # the lowest quantile leaves empty and non-empty queries


# ---- 2. strictness -----------------------------------------------------------------------------------------------------
def test_strict_comparison(gpu):
    c, sc = scored(BASE)
    g = _upload(gpu(), c)
    q = c["queries"]
    want = range_ref.expected_ivf(c, sc, MAX_CODES, range_ref.pooled_quantile(sc, 0.01))
    i = int(np.argmax(np.diff(want[0].astype(np.int64))))
    a = int(want[0][i])
    r, label = want[1][a], want[2][a]

    def labels_of(res):
        return res[2][int(res[0][i]):int(res[0][i + 1])]
    got = rs(g, q, r)
    assert label not in labels_of(got) and range_ref.same_range(got, range_ref.expected_ivf(c, sc, MAX_CODES, r))
    up = np.nextafter(r, INF)
    got = rs(g, q, up)
    assert label in labels_of(got) and range_ref.same_range(got, range_ref.expected_ivf(c, sc, MAX_CODES, up))
    lowest = min(d.min() for d in sc["dists"])
    for r0 in (lowest, np.float32(-1e30), -INF):
        lims, dist, lab = rs(g, q, r0)
        assert not lims.any() and len(dist) == 0 and len(lab) == 0
        assert g.range_results_dev() == (0, 0, 0)
        g.range_results(0, 0)
    assert rs(g, q, np.nextafter(lowest, INF))[0][-1] >= 1


# ---- 3. ties -----------------------------------------------------------------------------------------------------------
def test_ties_keep_scan_order(gpu):
    c0, sc0 = scored(BASE)
    off = c0["offsets"].astype(np.int64)
    codes = np.array(c0["codes"]).reshape(len(c0["ids"]), -1).copy()
    ncodes = np.array(c0["norm_codes"]).copy()
    probed = [int(x) for x in np.unique(sc0["cid"][:, :4]) if off[int(x) + 1] - off[int(x)] >= 4][:50]
    assert len(probed) == 50
    pairs = []
    for lst in probed:  # row j's code on row j + 1: equal distances for whoever scans the list
        j = off[lst] + (off[lst + 1] - off[lst]) // 2
        codes[j + 1], ncodes[j + 1] = codes[j], ncodes[j]
        pairs.append((int(c0["ids"][j]), int(c0["ids"][j + 1])))
    # one row twice: the first row of query 0's first probed list again at the head of its second, under the same label
    la, lb = int(sc0["cid"][0, 0]), int(sc0["cid"][0, 1])
    assert off[la + 1] > off[la] and off[lb + 1] > off[lb] and la != lb
    ra, rb = off[la], off[lb]
    codes[rb], ncodes[rb] = codes[ra], ncodes[ra]
    tmp = int(c0["ids"].max()) + 1
    ids_unique = c0["ids"].copy()
    ids_unique[rb] = tmp
    ids_dup = c0["ids"].copy()
    ids_dup[rb] = c0["ids"][ra]
    cu = dict(_with_ids(c0, ids_unique), codes=codes.reshape(np.asarray(c0["codes"]).shape), norm_codes=ncodes)
    sc = range_ref.scored_batch(cu, cu["queries"], NPROBE, MAX_CODES, EF)
    g = _upload(gpu(), dict(cu, ids=ids_dup))
    for r in (range_ref.pooled_quantile(sc, 0.1), INF):
        lims, dist, lab = range_ref.expected_ivf(cu, sc, MAX_CODES, r)
        want = (lims, dist, np.where(lab == tmp, int(c0["ids"][ra]), lab))
        got = rs(g, cu["queries"], r)
        assert range_ref.same_range(got, want)
    # at +inf: every pair stands side by side with equal bits, the copied-from row first; query 0 holds its label twice
    lims, dist, lab = got
    seen = 0
    for i in range(len(cu["queries"])):
        l, d = lab[int(lims[i]):int(lims[i + 1])], dist[int(lims[i]):int(lims[i + 1])].view(np.uint32)
        for a, b in pairs:
            at = np.nonzero(l == a)[0]
            if len(at):
                assert l[at[0] + 1] == b and d[at[0] + 1] == d[at[0]]
                seen += 1
    assert seen >= 50
    l0 = lab[:int(lims[1])]
    assert (l0 == int(c0["ids"][ra])).sum() == 2 and l0[0] == int(c0["ids"][ra])


# ---- 4. Grouping -------------------------------------------------------------------------------------------------------
def _grouping_ties(c):
    """Row j's code and norm code on row j + 1 of the same sub-group, in 50 lists: exact ties inside sub-groups."""
    off = c["offsets"].astype(np.int64)
    sizes = np.asarray(c["subgroup_sizes"]).reshape(c["nc"], -1).astype(np.int64)
    codes = np.array(c["codes"]).reshape(len(c["ids"]), -1).copy()
    ncodes = np.array(c["norm_codes"]).copy()
    pairs = []
    for lst in range(c["nc"]):
        big = np.nonzero(sizes[lst] >= 2)[0]
        if len(big) == 0 or len(pairs) == 50:
            continue
        j = off[lst] + sizes[lst][:big[-1]].sum()  # first row of the last sub-group with two rows
        codes[j + 1], ncodes[j + 1] = codes[j], ncodes[j]
        pairs.append((int(c["ids"][j]), int(c["ids"][j + 1])))
    assert len(pairs) == 50
    return dict(c, codes=codes.reshape(np.asarray(c["codes"]).shape), norm_codes=ncodes), pairs


@pytest.mark.parametrize("pruning,max_codes", [(False, 500), (True, MAX_CODES)], ids=["all", "pruned"])
def test_grouping(gpu, pruning, max_codes):
    c, pairs = _grouping_ties(corpus(**GROUPING))
    q = c["queries"]
    sc = range_ref.scored_batch(c, q, NPROBE, max_codes, 64, pruning)
    assert sc["ncode"].max() <= 1024 and sc["ncode"].min() > 0  # order check (a) sees every scored code
    g = _upload(gpu(), c)
    top_d, top_l = g.search(q, 1024, NPROBE, max_codes, efSearch=64, do_pruning=pruning, heap_order=False)
    k_counts = g.last_scan_counts()
    rr = radii(sc)
    low = None
    for r in rr:
        lims, dist, lab = rs(g, q, r, max_codes=max_codes, ef=64, do_pruning=pruning)
        assert g.last_scan_kernel() == "range_scan_bitmap_kernel"  # the short-segment form
        assert g.last_scan_counts() == k_counts
        assert lims[0] == 0 and lims[-1] == len(dist) == len(lab)
        for i in range(len(q)):
            assert np.array_equal(range_ref.result_set(lims, dist, lab, i), range_ref.expected_set(sc, i, r)), (float(r), i)
            # (a) ascending by (distance, scan position) it is the k-search's own ascending result up to the radius
            a, b = int(lims[i]), int(lims[i + 1])
            order = np.argsort(dist[a:b], kind="stable")
            assert np.array_equal(lab[a:b][order], top_l[i, :b - a])
            assert np.array_equal(dist[a:b][order].view(np.uint32), top_d[i, :b - a].view(np.uint32))
        if low is None:
            low = np.diff(lims.astype(np.int64))
    assert (low == 0).any() and (low > 0).any()
    # (b) at +inf the engineered ties stand side by side, the copied-from row first
    seen = 0
    for i in range(len(q)):
        l, d = lab[int(lims[i]):int(lims[i + 1])], dist[int(lims[i]):int(lims[i + 1])].view(np.uint32)
        for a, b in pairs:
            at = np.nonzero(l == a)[0]
            if len(at):
                assert l[at[0] + 1] == b and d[at[0] + 1] == d[at[0]]
                seen += 1
    assert seen > 0


# ---- 5. filter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,params", [(BASE, dict()), (GROUPING, dict(ef=64, do_pruning=True))], ids=["ivf", "grouping"])
def test_filter(gpu, kw, params):
    c = corpus(**kw)
    q = c["queries"]
    g = _upload(gpu(), c)
    rng = np.random.default_rng(5)
    allow = rng.choice(c["ids"], len(c["ids"]) // 10, replace=False).astype(np.uint32)
    rest = np.setdiff1d(c["ids"], allow).astype(np.uint32)
    plain = {}
    for r in (np.float32(rs(g, q, INF, **params)[1].mean() / 2), INF):
        plain[r] = rs(g, q, r, **params)
    name, counts = g.last_scan_kernel(), g.last_scan_counts()
    assert not name.endswith("+filter")
    for labels, deny, passing in ((allow, False, allow), (np.zeros(0, np.uint32), False, np.zeros(0, np.uint32)),
                                  (rest, True, allow)):
        g.set_filter(labels, deny=deny)
        for r, res in plain.items():
            got = rs(g, q, r, **params)
            assert g.last_scan_kernel() == name + "+filter"
            assert g.last_scan_counts() == counts
            assert range_ref.same_range(got, range_ref.filtered(res, passing)), (len(labels), deny, float(r))
        assert (len(got[2]) == 0) == (len(passing) == 0)
    g.clear_filter()
    assert range_ref.same_range(rs(g, q, INF, **params), plain[INF]) and g.last_scan_kernel() == name


# ---- 6. coarse stage ---------------------------------------------------------------------------------------------------
def test_given_coarse_results(gpu):
    c, sc = scored(BASE, max_codes=10 ** 9)
    q = c["queries"]
    g = _upload(gpu(), c)
    r = range_ref.pooled_quantile(sc, 0.1)
    walk = rs(g, q, r, max_codes=10 ** 9)
    assert range_ref.same_range(walk, range_ref.expected_ivf(c, sc, 10 ** 9, r))
    cid, cd = g.coarse(q, NPROBE, EF)
    assert np.array_equal(cid, sc["cid"])
    assert range_ref.same_range(rs(g, q, r, max_codes=10 ** 9, coarse_ids=cid, coarse_dists=cd), walk)
    # padding slots: their lists leave the scan, everything else keeps its distance and its order
    holes = cid.copy()
    holes[:, 1::3] = 0xffffffff
    holes[5, :] = 0xffffffff
    got = rs(g, q, r, max_codes=10 ** 9, coarse_ids=holes, coarse_dists=cd)
    assert range_ref.same_range(got, range_ref.expected_ivf(c, sc, 10 ** 9, r, cid=holes, subset=True))
    assert got[0][6] == got[0][5] and 0 < got[0][-1] < walk[0][-1]


@pytest.mark.parametrize("nq", [8, 200])
def test_after_prepare_latency(gpu, nq):
    c, sc = scored(BASE)
    g = _upload(gpu(), c)
    g.prepare_latency()
    idx = np.arange(nq) % len(c["queries"])
    q = np.ascontiguousarray(c["queries"][idx])
    for r in (range_ref.pooled_quantile(sc, 0.01), INF):
        assert range_ref.same_range(rs(g, q, r), expand(range_ref.expected_ivf(c, sc, MAX_CODES, r), idx))


@pytest.mark.parametrize("nq", [1, 3])
def test_few_queries_many_slices(gpu, nq):
    c, sc = scored(BASE, nprobe=64, max_codes=30000, ef=80, nq=3)
    g = _upload(gpu(), c)
    want = expand(range_ref.expected_ivf(c, sc, 30000, INF), np.arange(nq))
    assert want[0][1] > 3000  # thousands of results from the 32 slices of one query
    assert range_ref.same_range(rs(g, c["queries"][:nq], INF, nprobe=64, max_codes=30000, ef=80), want)
    r = range_ref.pooled_quantile(sc, 0.01)
    want = expand(range_ref.expected_ivf(c, sc, 30000, r), np.arange(nq))
    assert range_ref.same_range(rs(g, c["queries"][:nq], r, nprobe=64, max_codes=30000, ef=80), want)


# ---- 7. forms and lifetime ---------------------------------------------------------------------------------------------
def test_dev_form_second_call_memory(gpu):
    import torch
    c, sc = scored(BASE)
    q = c["queries"]
    g = _upload(gpu(), c)
    r1, r2 = range_ref.pooled_quantile(sc, 0.1), range_ref.pooled_quantile(sc, 0.01)
    mem0 = g.memory_bytes()
    host = rs(g, q, r1)
    assert g.memory_bytes() >= mem0 + 12 * int(host[0][-1])
    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(q).to(dev)
    d_lims = torch.full((len(q) + 1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    for r in (r2, r1):  # the second call replaces the first's results
        total = g.range_search_dev(len(q), d_q, float(r), d_lims, NPROBE, MAX_CODES, efSearch=EF)
        pd, pl, t = g.range_results_dev()
        assert t == total and pd and pl
        lims = d_lims.cpu().numpy().view(np.uint64)
        dist, lab = g.range_results(0, total)
        assert range_ref.same_range((lims, dist, lab), range_ref.expected_ivf(c, sc, MAX_CODES, r))
    assert range_ref.same_range((lims, dist, lab), host)
    part_d, part_l = g.range_results(7, 5)
    assert np.array_equal(part_l, lab[7:12]) and np.array_equal(part_d.view(np.uint32), dist[7:12].view(np.uint32))
    # the plan a range search leaves is not the last search's: resolve_keys refuses it
    kk = torch.zeros((len(q), 1), dtype=torch.int64, device=dev)
    dd = torch.zeros((len(q), 1), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    with pytest.raises(Exception) as e:
        g.resolve_keys_dev(len(q), 1, kk, dd, kk)
    assert e.value.code == -3


def test_view_beside_its_parent(gpu):
    c, sc = scored(BASE)
    q = c["queries"]
    g = _upload(gpu(), c)
    v = g.view()
    r1, r2 = range_ref.pooled_quantile(sc, 0.1), range_ref.pooled_quantile(sc, 0.01)
    a = rs(g, q, r1)
    b = rs(v, q[:50], r2)
    # each holds its own results
    assert g.range_results_dev()[2] == a[0][-1] and v.range_results_dev()[2] == b[0][-1]
    da, la = g.range_results(0, int(a[0][-1]))
    assert range_ref.same_range((a[0], da, la), range_ref.expected_ivf(c, sc, MAX_CODES, r1))
    assert range_ref.same_range(b, expand(range_ref.expected_ivf(c, sc, MAX_CODES, r2), np.arange(50)))
    v.close()


def test_after_append_and_remove(gpu):
    import remove_ref
    from test_gpu_append import _csr_append
    c, sc = scored(BASE)
    q = c["queries"]
    rng = np.random.default_rng(21)
    n, nc, M = 3000, c["nc"], c["code_size"]
    g = _upload(gpu(), c)
    r = range_ref.pooled_quantile(sc, 0.1)
    li = rng.integers(0, nc, n).astype(np.uint32)
    new_ids = (np.arange(n) + 10 ** 6).astype(np.uint32)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    ncodes = rng.integers(0, 255, n).astype(np.uint8)
    g.append_ivf(li, new_ids, codes, ncodes)
    lists = _csr_append((c["offsets"], c["ids"], c["codes"], c["norm_codes"]), nc, li, new_ids, codes, ncodes)
    cur = dict(c, offsets=lists[0], ids=lists[1], codes=lists[2], norm_codes=lists[3])
    for step in range(2):
        f = _upload(gpu(), cur)
        for rad in (r, INF):
            got = rs(g, q, rad)
            assert range_ref.same_range(got, rs(f, q, rad)), step
        if step == 0:
            assert np.isin(got[2], new_ids).any()
            gone = rng.choice(cur["ids"], 5000, replace=False)
            assert g.remove_ids(gone)[0] == 5000
            cur, _ = remove_ref.filtered_corpus(cur, gone)
        else:
            assert not np.isin(got[2], gone).any()
            sc2 = range_ref.scored_batch(cur, q, NPROBE, MAX_CODES, EF)
            assert range_ref.same_range(got, range_ref.expected_ivf(cur, sc2, MAX_CODES, INF))


# ---- 8. errors ---------------------------------------------------------------------------------------------------------
def test_errors(gpu, pkg):
    c, sc = scored(BASE)
    q = c["queries"]
    L = pkg.lib()
    INVALID, STATE = pkg.ERR_INVALID, pkg.ERR_STATE

    def code(f, *a, **kw):
        with pytest.raises(pkg.IvfHnswError) as e:
            f(*a, **kw)
        return e.value.code

    empty = gpu()
    assert code(rs, empty, q, 1.0) == STATE                           # before upload_ivf
    g = _upload(gpu(), c)
    assert code(g.range_results, 0, 0) == STATE                       # before any range search
    assert code(g.range_results_dev) == STATE
    r = range_ref.pooled_quantile(sc, 0.01)
    held = rs(g, q, r)
    total = int(held[0][-1])
    assert code(rs, g, q, np.float32(np.nan)) == INVALID              # NaN radius
    p = pkg.SearchParams(NPROBE, MAX_CODES, EF, 0, 0)
    lims, tot = np.zeros(len(q) + 1, np.uint64), C.c_uint64(0)
    qp, lp = q.ctypes.data_as(C.c_void_p), lims.ctypes.data_as(C.c_void_p)
    assert L.ivfhnsw_gpu_range_search(g._h, len(q), qp, None, None, C.byref(p), 1.0, None, C.byref(tot)) == INVALID
    assert L.ivfhnsw_gpu_range_search(g._h, len(q), qp, None, None, C.byref(p), 1.0, lp, None) == INVALID
    assert L.ivfhnsw_gpu_range_search(g._h, len(q), None, None, None, C.byref(p), 1.0, lp, C.byref(tot)) == INVALID
    # whatever search_dev refuses for the same params, with its status
    assert code(rs, g, q, 1.0, ef=NPROBE - 1) == code(g.search, q, 1, NPROBE, MAX_CODES, efSearch=NPROBE - 1) == INVALID
    assert code(rs, g, q, 1.0, nprobe=0) == code(g.search, q, 1, 0, MAX_CODES, efSearch=EF) == INVALID
    assert code(g.range_results, total - 1, 2) == INVALID             # beyond the total
    assert code(g.range_results, total + 1, 0) == INVALID
    # every error above left the results of the last good call
    dist, lab = g.range_results(0, total)
    assert range_ref.same_range((held[0], dist, lab), held) and g.range_results_dev()[2] == total
    # nq = 0
    lims0, d0, l0 = rs(g, np.zeros((0, c["d"]), np.float32), 1.0)
    assert lims0.tolist() == [0] and len(d0) == 0 and len(l0) == 0
    # a sharded handle
    s = _upload(gpu(), c, shard_rank=0, shard_world=2)
    assert code(rs, s, q, 1.0) == STATE


def test_batch_total_of_2_32_results_is_refused(gpu):
    """131 072 queries that each score every code of a 90 000-code synthetic upload: 1.2e10 results."""
    c = corpus(**BASE)
    g = gpu()
    off = c["offsets"].astype(np.uint64) * np.uint64(3)
    g.upload_ivf_synthetic(c["d"], c["code_size"], off, c["centroid_norms"], c["pq_centroids"], c["norm_table"], 7)
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    small = rs(g, c["queries"], INF, nprobe=c["nc"], max_codes=10 ** 9, ef=c["nc"])
    assert small[0][1] > 2 ** 15  # one query alone returns more than 2^32 / 131072 results
    held = int(small[0][-1])
    q = tiled(c["queries"], 1 << 17)
    with pytest.raises(Exception) as e:
        rs(g, q, INF, nprobe=c["nc"], max_codes=10 ** 9, ef=c["nc"])
    assert e.value.code == -1 and "2^32" in str(e.value)
    assert g.range_results_dev()[2] == held  # the earlier results are still there
