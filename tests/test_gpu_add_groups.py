"""Additions to a device-resident Grouping index (ivfhnsw_gpu_append_grouping / ivfhnsw_gpu_add_groups).

The expected state is always assembled on the host (grouping_append_ref.merge_lists; the oracle's add_group_encode per
group): the handle must then hold, byte for byte, what upload_ivf + upload_grouping of the merged index hold, and
searches must equal the oracle on the full index and a fresh upload of it: labels, distance bits, last_scan_counts."""
import numpy as np
import pytest

from conftest import corpus
import grouping_append_ref as gar
import synth
from oracle import orc

pytestmark = pytest.mark.gpu

BASE = dict(seed=97, nc=128, n_base=9000, nq=48, efConstruction=80)
SHAPES = [dict(BASE, nsubc=64, opq=True), dict(BASE, nsubc=8), dict(BASE, d=96, M=8, nsubc=16, opq=True),
          dict(BASE, d=32, M=4, nsubc=5), dict(BASE, d=96, M=12, nsubc=8), dict(BASE, seed=85, nc=64, d=112, M=28,
                                                                              n_base=4000, nq=32, nsubc=6, opq=True)]
SEARCH_SHAPES = SHAPES[:4]
KEYS = ("offsets", "ids", "codes", "norm_codes")
TABLES = ("alphas", "nn_centroid_idxs", "subgroup_sizes", "inter_centroid_dists")
NPROBE, MAX_CODES, EF = 16, 2000, 40


def _id(kw):
    return "d%d_M%d_nsubc%d%s" % (kw.get("d", 128), kw.get("M", 16), kw["nsubc"], "_opq" if kw.get("opq") else "")


def _upload(g, c, graph=True, lists=None, **kw):
    off, ids, codes, ncodes = lists if lists is not None else (c["offsets"], c["ids"], c["codes"], c["norm_codes"])
    g.upload_ivf(c["d"], c["code_size"], off, ids, codes, ncodes, c["centroid_norms"], c["pq_centroids"], c["norm_table"],
                 opq_A=c["opq_A"], **kw)
    g.upload_grouping(c["nsubc"], c["alphas"], c["nn_centroid_idxs"], c["subgroup_sizes"], c["inter_centroid_dists"])
    if graph:
        gr = c["graph"]
        g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    return g


def _state(g):
    return g.download_ivf() + g.download_grouping_tables()


def _assert_state(g, want, lists=None):
    off, ids, codes, ncodes = g.download_ivf()
    w = lists if lists is not None else tuple(want[k] for k in KEYS)
    assert np.array_equal(off, np.asarray(w[0], np.uint64))
    assert np.array_equal(ids, w[1])
    assert np.array_equal(codes, np.asarray(w[2]).reshape(codes.shape))
    assert np.array_equal(ncodes, w[3])
    for got, k in zip(g.download_grouping_tables(), TABLES):
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32).reshape(got.shape)), k


def _same_search(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _append(g, batch, sel=slice(None), dev=False):
    args = [batch[k][sel] for k in ("list_idx", "sub_idx", "ids", "codes", "norm_codes")]
    if not dev:
        return g.append_grouping(*args)
    import torch
    dv = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).to(dv) for a in args]
    g.append_grouping_dev(len(args[0]), *t)


def _check_searches(gpu, g, full, added_lists):
    """g against the oracle on `full` and a fresh upload of it; conditions (c) and (d) of the issue asserted."""
    f = _upload(gpu(), full)
    lst, _ = gar.rows_of(full["offsets"], full["subgroup_sizes"])
    list_of_id = np.zeros(int(full["ids"].max()) + 1, np.int64)
    list_of_id[full["ids"]] = lst
    for k in (1, 10):
        for pruning in (False, True):
            ox = synth.oracle_index(full)
            ox.set_params(NPROBE, MAX_CODES, EF, do_pruning=pruning)
            ref = ox.search_batch(full["queries"], k=k)
            # heap_order: the very array the reference's heap leaves, element for element
            got = g.search(full["queries"], k, NPROBE, MAX_CODES, efSearch=EF, do_pruning=pruning, heap_order=True)
            counts = g.last_scan_counts()
            fresh = f.search(full["queries"], k, NPROBE, MAX_CODES, efSearch=EF, do_pruning=pruning, heap_order=True)
            assert _same_search(got, fresh) and counts == f.last_scan_counts()
            assert np.array_equal(got[1], ref[1].reshape(got[1].shape))
            assert np.array_equal(got[0].view(np.uint32), ref[0].reshape(got[0].shape).view(np.uint32))
            assert (got[1] >= 0).all()                                   # (c) no label -1
            best = got[1][np.arange(len(got[1])), got[0].argmin(1)]
            top1_added = added_lists[list_of_id[best]]
            assert top1_added.any() and (~top1_added).any()              # (d) top-1 answers on both sides
    return f


def _batch_conditions(part, batch, nc):
    """(a) the batch touches a sub-group that was empty and one that was not, (b) it leaves a list untouched."""
    before = part["subgroup_sizes"][batch["list_idx"], batch["sub_idx"]]
    assert (before == 0).any() and (before > 0).any()
    assert len(np.unique(batch["list_idx"])) < nc
    # ... and an empty sub-group of a NON-empty list, and an empty list
    lens = np.diff(part["offsets"].astype(np.int64))
    assert ((before == 0) & (lens[batch["list_idx"]] > 0)).any() and (lens[batch["list_idx"]] == 0).any()


# ---- 1. layout, primitive ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", SHAPES, ids=_id)
@pytest.mark.parametrize("nbatches", [1, 3, 10])
def test_append_grouping_layout(gpu, kw, nbatches):
    c = corpus(**kw)
    rng = np.random.default_rng(kw["nsubc"])
    part, batch = gar.split_corpus(c, gar.tail_mask(c, rng))
    _batch_conditions(part, batch, c["nc"])
    p = rng.permutation(len(batch["ids"]))
    # arrival order: a shuffle, so that the rows of one sub-group arrive between those of all the others
    shuffled = {k: v[p] for k, v in batch.items()}
    g = _upload(gpu(), part, graph=False)
    cur = part
    for sel in np.array_split(np.arange(len(p)), nbatches):
        _append(g, shuffled, sel)
        cur = dict(part, **gar.merge_lists(cur["offsets"], cur["ids"], cur["codes"], cur["norm_codes"], cur["subgroup_sizes"],
                                           *[shuffled[k][sel] for k in ("list_idx", "sub_idx", "ids", "codes", "norm_codes")]))
        _assert_state(g, cur)
    # the tails in their own order restore the corpus itself
    h = _upload(gpu(), part, graph=False)
    for sel in np.array_split(np.arange(len(p)), nbatches):
        _append(h, batch, sel)
    _assert_state(h, c)


@pytest.mark.parametrize("where", ["one_list", "every_list", "empty_lists"])
def test_append_grouping_targets_and_dev_form(gpu, where):
    c = corpus(**SHAPES[1])
    nc, nsubc, M = c["nc"], c["nsubc"], c["code_size"]
    rng = np.random.default_rng(3)
    lens = np.diff(c["offsets"].astype(np.int64))
    if where == "one_list":
        li = np.full(500, int(np.argmax(lens)), np.uint32)
    elif where == "every_list":
        li = np.concatenate([np.arange(nc), rng.integers(0, nc, 2000)]).astype(np.uint32)
    else:
        empty = np.nonzero(lens == 0)[0]
        assert len(empty) >= 2
        li = rng.choice(empty, 300).astype(np.uint32)
    n = len(li)
    batch = dict(list_idx=li, sub_idx=rng.integers(0, nsubc, n).astype(np.uint32),
                 ids=(10 ** 6 + np.arange(n)).astype(np.uint32), codes=rng.integers(0, 256, (n, M)).astype(np.uint8),
                 norm_codes=rng.integers(0, 256, n).astype(np.uint8))
    want = dict(c, **gar.merge_lists(c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["subgroup_sizes"],
                                     *[batch[k] for k in ("list_idx", "sub_idx", "ids", "codes", "norm_codes")]))
    g = _upload(gpu(), c, graph=False)
    _append(g, batch)
    _assert_state(g, want)
    h = _upload(gpu(), c, graph=False)
    _append(h, batch, dev=True)
    _assert_state(h, want)
    g.append_grouping(*[batch[k][:0] for k in ("list_idx", "sub_idx", "ids", "codes", "norm_codes")])   # n = 0: nothing
    _assert_state(g, want)


# ---- 2. layout, add_groups -----------------------------------------------------------------------------------------
def _assign(c):
    x, cen = c["base"].astype(np.float64), c["centroids"].astype(np.float64)
    d2 = (x ** 2).sum(1)[:, None] - 2.0 * x @ cen.T + (cen ** 2).sum(1)[None, :]
    return d2.argmin(1)


def _build_graph(c):
    """The quantizer as add_group sees it: before rotate_quantizer (the drivers rotate after the index is complete)."""
    gr = c["graph"]
    if c["opq_A"] is None:
        return gr
    return orc.Hnsw.from_arrays(gr.counts, gr.links, c["centroids"], 16, gr.enterpoint)


def _encoder(c, g0):
    nc, M = c["nc"], c["code_size"]
    ox = orc.Index(c["d"], M, g0, c["pq_centroids"], c["norm_table"], np.zeros(nc + 1, np.uint64), np.zeros(0, np.uint32),
                   np.zeros((0, M), np.uint8), np.zeros(0, np.uint8), np.zeros(nc, np.float32), opq_A=c["opq_A"])
    ox.set_params(1, 0, 80)
    return ox


def _assemble(c, g0, groups, inter=None):
    """The Grouping index add_group builds from groups = {centroid: (points, ids)} (IndexIVF_HNSW_Grouping.cpp:43-157
    through the oracle's add_group_encode), as a corpus dict.  Groups without points: neighbour row only."""
    nc, nsubc, M = c["nc"], c["nsubc"], c["code_size"]
    ox = _encoder(c, g0)
    nn = np.zeros((nc, nsubc), np.uint32)
    alphas = np.zeros(nc, np.float32)
    sg = np.zeros((nc, nsubc), np.uint32)
    ids, codes, ncodes = [], [], []
    for cc in range(nc):
        if cc not in groups:
            continue
        x, gid = groups[cc]
        rnn, ralpha, rsub, rcodes, rnc = ox.add_group_encode(nsubc, cc, x)
        nn[cc] = rnn
        if len(gid) == 0:
            continue
        alphas[cc] = ralpha
        order = np.argsort(rsub, kind="stable")
        sg[cc] = np.bincount(rsub, minlength=nsubc)
        ids.append(gid[order])
        codes.append(rcodes[order])
        ncodes.append(rnc[order])
    icd = g0.inter_centroid_dists(nn) if inter is None else inter.copy()
    icd[sg.sum(1) == 0] = 0
    off = np.concatenate([[0], np.cumsum(sg.sum(1, dtype=np.int64))]).astype(np.uint64)
    return dict(c, offsets=off, ids=np.concatenate(ids).astype(np.uint32), codes=np.ascontiguousarray(np.concatenate(codes)),
                norm_codes=np.concatenate(ncodes).astype(np.uint8), subgroup_sizes=sg, nn_centroid_idxs=nn, alphas=alphas,
                inter_centroid_dists=icd)


def _groups_of(c, points=None, ids=None):
    a = _assign(c)
    x = c["base"] if points is None else points
    gid = np.arange(len(x), dtype=np.uint32) if ids is None else ids
    return {cc: (np.ascontiguousarray(x[a == cc]), gid[a == cc]) for cc in range(c["nc"])}


def _add_groups(g, groups, which, inter=None, calls=3):
    """add_groups of the centroids `which`, in `calls` calls of shuffled groups."""
    for part in np.array_split(np.asarray(which), calls):
        if len(part) == 0:
            continue
        xs = [groups[int(cc)][0] for cc in part]
        off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)
        x = np.concatenate(xs) if off[-1] else np.zeros((0, g.d), np.float32)
        ids = np.concatenate([groups[int(cc)][1] for cc in part]).astype(np.uint32)
        g.add_groups(part.astype(np.uint32), off, x, ids, 80, inter_centroid_dists=None if inter is None else inter[part])


def _group_case(kw, seed):
    c = corpus(**kw)
    g0 = _build_graph(c)
    groups = _groups_of(c)
    rng = np.random.default_rng(seed)
    gone = rng.random(c["nc"]) < 0.5
    return c, g0, groups, gone, rng


def _upload_for_add(gpu, c, g0, part):
    g = _upload(gpu(), part, graph=False)
    g.upload_quantizer(g0.counts, g0.links, g0.vectors, g0.enterpoint)
    g.upload_codebooks(c["d"], c["code_size"], c["pq_centroids"], c["norm_table"], c["opq_A"])
    return g


@pytest.mark.parametrize("kw", SEARCH_SHAPES, ids=_id)
@pytest.mark.parametrize("given", [False, True], ids=["computed_icd", "given_icd"])
def test_add_groups_layout_and_search(gpu, kw, given):
    c, g0, groups, gone, rng = _group_case(kw, 21)
    inter = rng.random((c["nc"], c["nsubc"])).astype(np.float32) * 1000 if given else None
    full = _assemble(c, g0, groups, inter)
    part, _ = gar.without_groups(full, gone)
    part["subgroup_sizes"][gone] = 0
    which = rng.permutation(np.nonzero(gone)[0])
    npts = np.array([len(groups[int(cc)][1]) for cc in which])
    assert (npts == 0).any() and (npts > 0).any() and (~gone).any()
    g = _upload_for_add(gpu, c, g0, part)
    _add_groups(g, groups, which, inter)
    _assert_state(g, full)
    if not given:
        icd = g.download_grouping_tables()[3]
        ref = g0.inter_centroid_dists(full["nn_centroid_idxs"])
        live = gone & (full["subgroup_sizes"].sum(1) > 0)
        assert np.array_equal(icd[live].view(np.uint32), ref[live].view(np.uint32))
    # searches run on the rotated quantizer (the drivers rotate once the index is complete)
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    _check_searches(gpu, g, full, gone)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(view)).to(torch.device("cuda", 0))


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


@pytest.mark.parametrize("given", [False, True], ids=["computed_icd", "given_icd_no_norm_out"])
def test_add_groups_dev_equals_host_form(gpu, pkg, given):
    c, g0, groups, gone, rng = _group_case(SHAPES[1], 71)
    nc, nsubc, M = c["nc"], c["nsubc"], c["code_size"]
    inter = rng.random((nc, nsubc)).astype(np.float32) * 1000 if given else None
    full = _assemble(c, g0, groups, inter)
    part, _ = gar.without_groups(full, gone)
    which = rng.permutation(np.nonzero(gone)[0]).astype(np.uint32)
    xs = [groups[int(cc)][0] for cc in which]
    npts = np.array([len(x) for x in xs])
    assert (npts == 0).any() and (npts > 0).any()
    off = np.concatenate([[0], np.cumsum(npts)]).astype(np.uint64)
    x = np.ascontiguousarray(np.concatenate(xs))
    ids = np.concatenate([groups[int(cc)][1] for cc in which]).astype(np.uint32)
    n, G = len(ids), len(which)
    marker = np.full(G, 123.0, np.float32)
    a = _upload_for_add(gpu, c, g0, part)
    h_nn, h_al, h_sub, h_codes, h_nc = a.add_groups(which, off, x, ids, 80, alphas_in=marker,
                                                    inter_centroid_dists=None if inter is None else inter[which])
    _assert_state(a, full)
    assert (h_al[npts == 0] == 123.0).all() and (h_al[npts > 0] != 123.0).all()
    b = _upload_for_add(gpu, c, g0, part)
    before = _state(b)
    d_cidx, d_off, d_x, d_ids = _dev(which), _dev(off), _dev(x), _dev(ids)
    d_nn, d_al = _dev(np.zeros((G, nsubc), np.uint32)), _dev(marker)
    d_sub, d_codes = _dev(np.zeros(n, np.uint32)), _dev(np.zeros((n, M), np.uint8))
    d_nc = None if given else _dev(np.zeros(n, np.uint8))
    d_inter = None if inter is None else _dev(inter[which])

    def call(cidx=d_cidx, offs=d_off, ngroups=G):
        b.add_groups_dev(ngroups, cidx, offs, d_x, d_ids, 80, d_nn, d_al, d_sub, d_codes, d_out_norm_codes=d_nc,
                         d_inter_centroid_dists=d_inter)

    def refused(code, **kw):
        with pytest.raises(pkg.IvfHnswError) as e:
            call(**kw)
        assert e.value.code == code, str(e.value)
        for u, v in zip(_state(b), before):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
        return str(e.value)

    bad = which.copy()
    bad[1] = nc
    refused(pkg.ERR_INVALID, cidx=_dev(bad))
    bad[1] = bad[0]
    refused(pkg.ERR_INVALID, cidx=_dev(bad))
    live = int(np.nonzero(~gone & (full["subgroup_sizes"].sum(1) > 0))[0][0])
    bad[1] = live
    assert "list %d" % live in refused(pkg.ERR_STATE, cidx=_dev(bad))
    refused(pkg.ERR_INVALID, cidx=d_cidx.data_ptr() + 1)                # misaligned device pointers
    refused(pkg.ERR_INVALID, offs=d_off.data_ptr() + 4)
    call()
    _assert_state(b, full)
    assert np.array_equal(_host(d_nn, np.uint32), h_nn) and np.array_equal(_host(d_al, np.uint32), h_al.view(np.uint32))
    assert np.array_equal(_host(d_sub, np.uint32), h_sub) and np.array_equal(_host(d_codes, np.uint8), h_codes)
    if d_nc is not None:
        assert np.array_equal(_host(d_nc, np.uint8), h_nc)
    assert _same_search(a.search(c["queries"], 10, NPROBE, MAX_CODES, efSearch=EF, do_pruning=True),
                        b.search(c["queries"], 10, NPROBE, MAX_CODES, efSearch=EF, do_pruning=True))


def test_memory_bytes_counts_the_work_tables(gpu):
    """The handle keeps three [nc][nsubc] uint32 work tables after its first append_grouping, and accounts for them."""
    c = corpus(**SHAPES[1])
    part, batch = gar.split_corpus(c, gar.tail_mask(c, np.random.default_rng(9)))
    g = _upload(gpu(), part, graph=False)
    held = g.memory_bytes()
    _append(g, batch)
    grown = len(batch["ids"]) * c["code_size"]          # the lists themselves
    assert g.memory_bytes() - held >= 3 * c["nc"] * c["nsubc"] * 4 + grown


# ---- 3. search after the primitive, the tail kernel, the two-part split ----------------------------------------------
@pytest.mark.parametrize("kw", SEARCH_SHAPES, ids=_id)
def test_search_after_append_grouping(gpu, kw):
    c = corpus(**kw)
    rng = np.random.default_rng(31)
    gone = rng.random(c["nc"]) < 0.5
    lst, _ = gar.rows_of(c["offsets"], c["subgroup_sizes"])
    held = gar.tail_mask(c, rng) | gone[lst]              # whole groups and tails of the others
    held[np.isin(lst, np.nonzero(~gone)[0][:3])] = False  # some lists untouched
    part, batch = gar.split_corpus(c, held)
    _batch_conditions(part, batch, c["nc"])
    g = _upload(gpu(), part)
    for sel in np.array_split(np.arange(len(batch["ids"])), 3):
        _append(g, batch, sel)
    _assert_state(g, c)
    f = _check_searches(gpu, g, c, gone)
    # the tail kernel (one query per call after prepare_latency, which exists for d = 128 and 96)
    if c["d"] not in (128, 96):
        return
    g.prepare_latency()
    f.prepare_latency()
    for q in c["queries"][:12]:
        for k in (1, 10):
            assert _same_search(g.search(q[None, :], k, NPROBE, MAX_CODES, efSearch=EF, do_pruning=True),
                                f.search(q[None, :], k, NPROBE, MAX_CODES, efSearch=EF, do_pruning=True))


def test_large_batch_split_view_after_append_grouping(gpu):
    import torch
    c = corpus(**SHAPES[1])
    rng = np.random.default_rng(0)
    part, batch = gar.split_corpus(c, gar.tail_mask(c, rng))
    g = _upload(gpu(), part)
    q = np.repeat(c["queries"], 190, axis=0)[:9000]
    q = q + rng.normal(0, 2.0, q.shape).astype(np.float32)
    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)

    def run(h):
        d = torch.empty((len(q), 1), dtype=torch.float32, device=dev)
        lab = torch.empty((len(q), 1), dtype=torch.int64, device=dev)
        h.search_dev(len(q), 1, d_q, d, lab, NPROBE, MAX_CODES, efSearch=EF, do_pruning=True)
        h.sync()
        assert h.last_batch_parts()[1] > 0, "the batch did not take the two-part path"
        return d.cpu().numpy(), lab.cpu().numpy()

    run(g)  # the internal split view exists before the append
    _append(g, batch)
    _assert_state(g, c)
    assert _same_search(run(g), run(_upload(gpu(), c)))


# ---- 4. remove, then add --------------------------------------------------------------------------------------------
def test_remove_then_add_groups(gpu):
    c, g0, groups, gone, rng = _group_case(SHAPES[1], 41)
    full = _assemble(c, g0, groups)
    g = _upload_for_add(gpu, c, g0, full)
    sizes = full["subgroup_sizes"].sum(1)
    which = rng.permutation(np.nonzero(gone & (sizes > 0))[0])[:20]
    old_ids = np.concatenate([groups[int(cc)][1] for cc in which])
    n_rm, _ = g.remove_ids(old_ids)
    assert n_rm == len(old_ids)
    # other points for the same centroids: a perturbed half of the old ones under new labels
    new = dict(groups)
    for cc in which:
        x, gid = groups[int(cc)]
        keep = rng.random(len(gid)) < 0.5
        keep[0] = True
        new[int(cc)] = (np.ascontiguousarray(x[keep] + rng.normal(0, 3.0, x[keep].shape).astype(np.float32)),
                        (gid[keep] + np.uint32(10 ** 6)).astype(np.uint32))
    _add_groups(g, new, which, calls=2)
    want = _assemble(c, g0, new)
    _assert_state(g, want)
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    f = _upload(gpu(), want)
    for pruning in (False, True):
        assert _same_search(g.search(c["queries"], 10, NPROBE, MAX_CODES, efSearch=EF, do_pruning=pruning),
                            f.search(c["queries"], 10, NPROBE, MAX_CODES, efSearch=EF, do_pruning=pruning))
        assert g.last_scan_counts() == f.last_scan_counts()


# ---- 5. shards ------------------------------------------------------------------------------------------------------
def _shard_lists(c, rank, world):
    off = c["offsets"].astype(np.int64)
    owned = [cc for cc in range(c["nc"]) if cc % world == rank]
    sel = np.concatenate([np.arange(off[cc], off[cc + 1]) for cc in owned]).astype(np.int64)
    codes = np.asarray(c["codes"]).reshape(len(c["ids"]), -1)
    return c["offsets"], c["ids"][sel], codes[sel], c["norm_codes"][sel]


@pytest.mark.parametrize("pruning", [False, True])
def test_sharded_append_grouping(gpu, pkg, pruning):
    c = corpus(**SHAPES[1])
    rng = np.random.default_rng(51)
    part, batch = gar.split_corpus(c, gar.tail_mask(c, rng))
    world = 3
    shards = []
    for r in range(world):
        g = _upload(gpu(), part, lists=_shard_lists(part, r, world), shard_rank=r, shard_world=world)
        for sel in np.array_split(np.arange(len(batch["ids"])), 2):
            _append(g, batch, sel)
        _assert_state(g, c, lists=_shard_lists(c, r, world))
        shards.append(g)
    ox = synth.oracle_index(c)
    ox.set_params(NPROBE, MAX_CODES, EF, do_pruning=pruning)
    ref_d, ref_l, cid, cd, _ = ox.search_batch(c["queries"], k=10)
    one = _upload(gpu(), c)
    d1, l1 = one.search(c["queries"], 10, NPROBE, MAX_CODES, coarse_ids=cid, coarse_dists=cd, do_pruning=pruning)
    d, lab = pkg.search_sharded(shards, c["queries"], 10, NPROBE, MAX_CODES, cid, cd, do_pruning=pruning)
    assert _same_search((d, lab), (d1, l1))
    # against the oracle's heap array as sets per query (the sharded step answers in ascending order)
    assert np.array_equal(np.sort(lab, 1), np.sort(ref_l.reshape(lab.shape), 1))
    assert np.array_equal(np.sort(d, 1).view(np.uint32), np.sort(ref_d.reshape(d.shape), 1).view(np.uint32))


def test_sharded_add_groups(gpu, pkg):
    c, g0, groups, gone, rng = _group_case(SHAPES[1], 53)
    full = _assemble(c, g0, groups)
    part, _ = gar.without_groups(full, gone)
    which = rng.permutation(np.nonzero(gone)[0])
    world = 3
    shards = []
    for r in range(world):
        g = _upload(gpu(), part, graph=False, lists=_shard_lists(part, r, world), shard_rank=r, shard_world=world)
        g.upload_quantizer(g0.counts, g0.links, g0.vectors, g0.enterpoint)
        g.upload_codebooks(c["d"], c["code_size"], c["pq_centroids"], c["norm_table"], c["opq_A"])
        _add_groups(g, groups, which)                    # every shard is given every group
        _assert_state(g, full, lists=_shard_lists(full, r, world))
        shards.append(g)
    ox = synth.oracle_index(full)
    ox.set_params(NPROBE, MAX_CODES, EF, do_pruning=True)
    ref_d, ref_l, cid, cd, _ = ox.search_batch(c["queries"], k=10)
    one = _upload(gpu(), full)
    d1, l1 = one.search(c["queries"], 10, NPROBE, MAX_CODES, coarse_ids=cid, coarse_dists=cd, do_pruning=True)
    d, lab = pkg.search_sharded(shards, c["queries"], 10, NPROBE, MAX_CODES, cid, cd, do_pruning=True)
    assert _same_search((d, lab), (d1, l1))
    assert np.array_equal(np.sort(lab, 1), np.sort(ref_l.reshape(lab.shape), 1))


# ---- 6. errors leave the tables ---------------------------------------------------------------------------------------
def test_errors_leave_the_tables(gpu, pkg):
    import torch
    c, g0, groups, gone, rng = _group_case(SHAPES[1], 61)
    full = _assemble(c, g0, groups)
    part, _ = gar.without_groups(full, gone)
    part["subgroup_sizes"][gone] = 0
    nc, nsubc, M = c["nc"], c["nsubc"], c["code_size"]
    g = _upload_for_add(gpu, c, g0, part)
    before = _state(g)
    ref = g.search(c["queries"], 10, NPROBE, MAX_CODES, efSearch=EF, do_pruning=True)

    def unchanged():
        for x, y in zip(_state(g), before):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert _same_search(g.search(c["queries"], 10, NPROBE, MAX_CODES, efSearch=EF, do_pruning=True), ref)

    def raises(code, fn, *a, **k):
        with pytest.raises(pkg.IvfHnswError) as e:
            fn(*a, **k)
        assert e.value.code == code, str(e.value)
        unchanged()
        return str(e.value)

    one = lambda li, si: (np.array([0, li], np.uint32), np.array([0, si], np.uint32), np.array([7, 8], np.uint32),
                          np.zeros((2, M), np.uint8), np.zeros(2, np.uint8))
    raises(pkg.ERR_INVALID, g.append_grouping, *one(nc, 0))
    raises(pkg.ERR_INVALID, g.append_grouping, *one(0, nsubc))
    dv = torch.device("cuda", 0)
    for bad in (one(nc, 0), one(0, nsubc)):
        t = [torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).to(dv) for a in bad]
        raises(pkg.ERR_INVALID, g.append_grouping_dev, 2, *t)
    assert pkg.lib().ivfhnsw_gpu_append_grouping(g._h, 2, None, None, None, None, None) == pkg.ERR_INVALID
    unchanged()
    # n_local + n reaches 2^32 - 1: refused by its size alone (nothing of the batch is read)
    big = torch.zeros(16, dtype=torch.int32, device=dv)
    raises(pkg.ERR_INVALID, g.append_grouping_dev, 2 ** 32 - 2, big, big, big, big, big)
    v = g.view()
    raises(pkg.ERR_STATE, v.append_grouping, *one(1, 0))
    v.close()
    empty = np.nonzero(gone)[0]
    live = np.nonzero(~gone & (full["subgroup_sizes"].sum(1) > 0))[0]
    x2 = np.ascontiguousarray(c["base"][:2])
    off2 = np.array([0, 1, 2], np.uint64)
    ids2 = np.array([1, 2], np.uint32)
    raises(pkg.ERR_INVALID, g.add_groups, np.array([empty[0], nc], np.uint32), off2, x2, ids2, 80)
    raises(pkg.ERR_INVALID, g.add_groups, np.array([empty[0], empty[0]], np.uint32), off2, x2, ids2, 80)
    msg = raises(pkg.ERR_STATE, g.add_groups, np.array([empty[0], live[0]], np.uint32), off2, x2, ids2, 80)
    assert "list %d" % live[0] in msg
    # code books that do not match the index
    g.upload_codebooks(c["d"], 8, c["pq_centroids"].reshape(8, 256, -1), c["norm_table"])
    raises(pkg.ERR_INVALID, g.add_groups, np.array([empty[0], empty[1]], np.uint32), off2, x2, ids2, 80)
    g.upload_codebooks(c["d"], M, c["pq_centroids"], c["norm_table"], c["opq_A"])
    # handles in the wrong state
    h = gpu()
    with pytest.raises(pkg.IvfHnswError) as e:
        h.append_grouping(*one(1, 0))
    assert e.value.code == pkg.ERR_STATE
    h.upload_ivf(c["d"], M, part["offsets"], part["ids"], part["codes"], part["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"])
    lists = h.download_ivf()
    for fn, args in ((h.append_grouping, one(1, 0)), (h.download_grouping_tables, ())):
        with pytest.raises(pkg.IvfHnswError) as e:
            fn(*args)
        assert e.value.code == pkg.ERR_STATE
    for x, y in zip(h.download_ivf(), lists):
        assert np.array_equal(x, y)
    # after all that the handle still takes the groups
    _add_groups(g, groups, empty)
    _assert_state(g, full)


def test_upload_centroid_norms(gpu):
    c = corpus(**SHAPES[1])
    other = dict(c, centroid_norms=(c["centroid_norms"] * np.float32(1.03)).astype(np.float32))
    g = _upload(gpu(), c)
    f = _upload(gpu(), other)
    a = g.search(c["queries"], 10, NPROBE, MAX_CODES, efSearch=EF)
    g.upload_centroid_norms(other["centroid_norms"])
    b = g.search(c["queries"], 10, NPROBE, MAX_CODES, efSearch=EF)
    assert _same_search(b, f.search(c["queries"], 10, NPROBE, MAX_CODES, efSearch=EF)) and not _same_search(a, b)


# ---- 7. scale -------------------------------------------------------------------------------------------------------
def test_scale_synthetic_2_24_codes(gpu):
    import torch
    nc, M, nsubc = 65536, 16, 64
    tb = synth.make_throughput_tables(5, nc, 128, M, 1 << 24)
    off = tb["offsets"]
    n_old = int(off[-1])
    rng = np.random.default_rng(4)
    sizes = np.diff(off.astype(np.int64))
    cuts = np.sort(rng.integers(0, sizes[:, None] + 1, size=(nc, nsubc - 1)), axis=1)
    sg = np.diff(np.concatenate([np.zeros((nc, 1), np.int64), cuts, sizes[:, None]], axis=1), axis=1).astype(np.uint32)
    nn = rng.integers(0, nc, (nc, nsubc)).astype(np.uint32)
    g = gpu()
    g.upload_ivf_synthetic(128, M, off, np.zeros(nc, np.float32), tb["pq_centroids"], tb["norm_table"], seed=77)
    g.upload_grouping(nsubc, np.zeros(nc, np.float32), nn, sg, np.zeros((nc, nsubc), np.float32))
    n = 1 << 20
    touched = rng.random(nc) < 0.7                      # many lists stay untouched
    li = rng.choice(np.nonzero(touched)[0], n).astype(np.uint32)
    si = rng.integers(0, nsubc, n).astype(np.uint32)
    ids = (n_old + np.arange(n)).astype(np.uint32)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    ncodes = rng.integers(0, 256, n).astype(np.uint8)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in (li, si, ids, codes, ncodes)]
    g.append_grouping_dev(n, *t)
    o2, ids2, codes2, nc2 = g.download_ivf()
    sg2 = g.download_grouping_tables()[2]
    cnt = np.bincount(li.astype(np.int64) * nsubc + si, minlength=nc * nsubc).reshape(nc, nsubc)
    assert np.array_equal(sg2, (sg + cnt).astype(np.uint32))
    assert np.array_equal(o2, np.concatenate([[0], np.cumsum(sizes + cnt.sum(1))]).astype(np.uint64))
    assert len(ids2) == n_old + n and np.array_equal(np.sort(ids2), np.arange(n_old + n, dtype=np.uint32))
    sample = np.unique(np.concatenate([rng.choice(nc, 48, replace=False), np.nonzero(~touched)[0][:8]]))
    gidx, sc, sn = synth.synthetic_codes_lists(77, off, M, sample)
    pos = 0
    for cc in sample:
        m = int(sizes[cc])
        mine = np.nonzero(li == cc)[0]
        w = gar.merge_lists(np.array([0, m]), gidx[pos:pos + m], sc[pos:pos + m], sn[pos:pos + m], sg[cc][None, :],
                            np.zeros(len(mine), np.uint32), si[mine], ids[mine], codes[mine], ncodes[mine])
        a, b = int(o2[cc]), int(o2[cc + 1])
        assert np.array_equal(ids2[a:b], w["ids"]) and np.array_equal(codes2[a:b], w["codes"]), cc
        assert np.array_equal(nc2[a:b], w["norm_codes"]), cc
        pos += m
