"""Appends to the lists a handle holds (ivfhnsw_gpu_append_ivf / _dev, ivfhnsw_gpu_add / _dev).

Every case uploads a prefix of each list (some lists empty, some held back whole) and appends the rest in batches that
interleave the lists while keeping each list's order, as IndexIVF_HNSW::add_batch appends (IndexIVF_HNSW.cpp:122-131).
The contract: the handle then holds, byte for byte, what upload_ivf of the whole corpus holds, and searches equal the
oracle on the whole corpus and a fresh upload, labels and distance bits and last_scan_counts."""
import numpy as np
import pytest

from conftest import corpus
import synth

pytestmark = pytest.mark.gpu

BASE = dict(seed=11, nc=256, d=128, M=16, n_base=30000, nq=128)


def _split(c, seed, nbatch=1, only=None):
    """(prefix CSR, [batches of (list_idx, ids, codes, norm_codes)]) of corpus c.  only: the lists that receive appends
    (the others are uploaded whole)."""
    rng = np.random.default_rng(seed)
    off = c["offsets"].astype(np.int64)
    nc = len(off) - 1
    lens = np.diff(off)
    keep = rng.integers(0, lens + 1)
    keep[rng.random(nc) < 0.2] = 0          # held back whole
    whole = rng.random(nc) < 0.1
    keep[whole] = lens[whole]               # nothing appended
    if only is not None:
        keep = lens.copy()
        keep[only] = lens[only] // 3
    rows = np.concatenate([np.arange(off[cc], off[cc] + keep[cc]) for cc in range(nc)]).astype(np.int64)
    pre_off = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint64)
    prefix = (pre_off, c["ids"][rows], c["codes"][rows], c["norm_codes"][rows])
    # the rest: list order kept, lists interleaved at random, cut into nbatch consecutive batches
    rest = np.concatenate([np.arange(off[cc] + keep[cc], off[cc + 1]) for cc in range(nc)]).astype(np.int64)
    lid = np.repeat(np.arange(nc), lens - keep)
    key = rng.random(len(rest))
    for cc in np.unique(lid):
        m = lid == cc
        key[m] = np.sort(key[m])
    order = np.argsort(key, kind="stable")
    rest, lid = rest[order], lid[order]
    cuts = np.sort(rng.integers(0, len(rest) + 1, nbatch - 1))
    batches = []
    for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(rest)]])):
        r = rest[a:b]
        batches.append((lid[a:b].astype(np.uint32), c["ids"][r], c["codes"][r], c["norm_codes"][r]))
    return prefix, batches


def _upload(g, c, lists, graph=True, **kw):
    off, ids, codes, ncodes = lists
    g.upload_ivf(c["d"], c["code_size"], off, ids, codes, ncodes, c["centroid_norms"], c["pq_centroids"],
                 c["norm_table"], opq_A=c["opq_A"], **kw)
    if graph:
        gr = c["graph"]
        g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)


def _full(c):
    return (c["offsets"], c["ids"], c["codes"], c["norm_codes"])


def _assert_layout(g, want):
    off, ids, codes, ncodes = g.download_ivf()
    assert np.array_equal(off, np.asarray(want[0], np.uint64))
    assert np.array_equal(ids, want[1])
    assert np.array_equal(codes, np.asarray(want[2]).reshape(len(ids), -1))
    assert np.array_equal(ncodes, want[3])


def _appended(gpu, c, seed, nbatch=1, only=None):
    prefix, batches = _split(c, seed, nbatch, only)
    g = gpu()
    _upload(g, c, prefix)
    for b in batches:
        g.append_ivf(*b)
    return g


def _same_search(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


@pytest.mark.parametrize("kw", [dict(BASE, M=8), BASE, dict(BASE, M=32),
                                dict(seed=81, nc=128, d=96, M=12, n_base=9000, nq=48, efConstruction=60),
                                dict(seed=85, nc=64, d=112, M=28, n_base=4000, nq=32, efConstruction=60, opq=True)],
                         ids=lambda kw: "M%d" % kw["M"])
def test_layout_equals_full_upload(gpu, kw):
    c = corpus(**kw)
    for nbatch in (1, 3):
        _assert_layout(_appended(gpu, c, seed=kw["M"] + nbatch, nbatch=nbatch), _full(c))


@pytest.mark.parametrize("only", ["first", "last", "all"])
def test_layout_single_list_and_every_list(gpu, only):
    c = corpus(**BASE)
    nc = len(c["offsets"]) - 1
    lists = {"first": [0], "last": [nc - 1], "all": list(range(nc))}[only]
    _assert_layout(_appended(gpu, c, seed=5, nbatch=2, only=lists), _full(c))


def test_ten_small_appends_and_empty(gpu):
    c = corpus(**BASE)
    g = _appended(gpu, c, seed=9, nbatch=10)
    g.append_ivf(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, c["code_size"]), np.uint8),
                 np.zeros(0, np.uint8))
    _assert_layout(g, _full(c))


@pytest.mark.parametrize("kw", [BASE, dict(seed=85, nc=64, d=112, M=28, n_base=4000, nq=32, efConstruction=60,
                                                opq=True)], ids=["pq16", "opq_M28"])
def test_search_equals_oracle_and_fresh_upload(gpu, kw):
    c = corpus(**kw)
    g = _appended(gpu, c, seed=3, nbatch=4)
    f = gpu()
    _upload(f, c, _full(c))
    ox = synth.oracle_index(c)
    nprobe, ef = 16, 40
    for k, max_codes, heap in ((1, 300, False), (1, 3000, False), (10, 2000, True)):
        ox.set_params(nprobe, max_codes, ef)
        ref = ox.search_batch(c["queries"], k=k)
        got = g.search(c["queries"], k, nprobe, max_codes, efSearch=ef, heap_order=heap)
        assert _same_search(got, ref[:2]), (k, max_codes)
        if k == 1:
            assert g.last_scan_counts()[0] == ref[4].ncode
        fr = f.search(c["queries"], k, nprobe, max_codes, efSearch=ef, heap_order=heap)
        assert _same_search(got, fr)
        assert g.last_scan_counts() == f.last_scan_counts()
    # a view made after the append sees the new lists
    v = g.view()
    ox.set_params(nprobe, 300, ef)
    ref = ox.search_batch(c["queries"], k=1)
    assert _same_search(v.search(c["queries"], 1, nprobe, 300, efSearch=ef), ref[:2])
    v.close()


def test_large_batch_split_view_after_append(gpu):
    import torch
    c = corpus(**BASE)
    g = _appended(gpu, c, seed=4, nbatch=2)
    f = gpu()
    _upload(f, c, _full(c))
    rng = np.random.default_rng(0)
    q = np.repeat(c["queries"], 72, axis=0)[:9000]
    q = q + rng.normal(0, 2.0, q.shape).astype(np.float32)
    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    out = []
    for h in (g, f):
        d = torch.empty((len(q), 1), dtype=torch.float32, device=dev)
        lab = torch.empty((len(q), 1), dtype=torch.int64, device=dev)
        h.search_dev(len(q), 1, d_q, d, lab, 16, 2000, efSearch=40)
        h.sync()
        out.append((d.cpu().numpy(), lab.cpu().numpy()))
        assert h.last_batch_parts()[1] > 0, "the batch did not take the two-part path"
    assert _same_search(out[0], out[1])


def _shard_arrays(c, rank, world, owner, lists):
    off = np.asarray(lists[0], np.int64)
    owned = [cc for cc in range(len(off) - 1) if (cc % world if owner is None else owner[cc]) == rank]
    sel = np.concatenate([np.arange(off[cc], off[cc + 1]) for cc in owned]).astype(np.int64)
    return lists[0], lists[1][sel], lists[2][sel], lists[3][sel]


@pytest.mark.parametrize("partition", ["mod", "owner"])
def test_sharded_append(gpu, pkg, partition):
    c = corpus(**BASE)
    world = 3
    nc = len(c["offsets"]) - 1
    owner = None if partition == "mod" else np.random.default_rng(2).integers(0, world, nc).astype(np.uint32)
    prefix, batches = _split(c, 13, 3)
    shards = []
    for r in range(world):
        g = gpu()
        _upload(g, c, _shard_arrays(c, r, world, owner, prefix), shard_rank=r, shard_world=world, list_owner=owner)
        for b in batches:
            g.append_ivf(*b)
        _assert_layout(g, _shard_arrays(c, r, world, owner, _full(c)))
        shards.append(g)
    ox = synth.oracle_index(c)
    ox.set_params(16, 2500, 40)
    ref_d, ref_l, cid, cd, _ = ox.search_batch(c["queries"], k=1)
    d, lab = pkg.search_sharded(shards, c["queries"], 1, 16, 2500, cid, cd)
    assert np.array_equal(lab, ref_l) and np.array_equal(d.view(np.uint32), ref_d.view(np.uint32))


def _csr_append(lists, nc, idx, ids, codes, ncodes):
    """The lists after add_batch's append loop, restated on the host."""
    off = np.asarray(lists[0], np.int64)
    lens = np.diff(off)
    cnt = np.bincount(idx, minlength=nc)
    noff = np.concatenate([[0], np.cumsum(lens + cnt)])
    M = codes.shape[1]
    out = (noff.astype(np.uint64), np.empty(noff[-1], np.uint32), np.empty((noff[-1], M), np.uint8),
           np.empty(noff[-1], np.uint8))
    lid = np.repeat(np.arange(nc), lens)
    dst = noff[lid] + np.arange(len(lid)) - off[lid]
    out[1][dst], out[2][dst], out[3][dst] = lists[1], np.asarray(lists[2]).reshape(-1, M), lists[3]
    order = np.argsort(idx, kind="stable")
    nstart = np.concatenate([[0], np.cumsum(cnt)])
    si = idx[order]
    dst = noff[si] + lens[si] + np.arange(len(si)) - nstart[si]
    out[1][dst], out[2][dst], out[3][dst] = ids[order], codes[order], ncodes[order]
    return out


@pytest.mark.parametrize("opq", [False, True])
def test_add_equals_encode_then_upload(gpu, opq):
    import torch
    c = corpus(seed=61, nc=128, d=128, M=16, n_base=12000, nq=64, opq=opq)
    nc = len(c["offsets"]) - 1
    g = gpu()
    _upload(g, c, _full(c))
    g.upload_codebooks(c["d"], c["code_size"], c["pq_centroids"], c["norm_table"], c["opq_A"])
    x = c["base"][:3000] + np.float32(0.5)
    ids = np.arange(10 ** 6, 10 ** 6 + len(x), dtype=np.uint32)
    e_idx, e_codes, e_nc = g.encode(x, efSearch=40)
    a_idx, a_codes, a_nc = g.add(x, ids, efSearch=40)
    assert np.array_equal(a_idx, e_idx) and np.array_equal(a_codes, e_codes) and np.array_equal(a_nc, e_nc)
    want = _csr_append(_full(c), nc, e_idx, ids, e_codes, e_nc)
    _assert_layout(g, want)
    # add_dev with precomputed ids, on top
    dev = torch.device("cuda", 0)
    x2 = c["base"][3000:5000]
    p2 = np.random.default_rng(1).integers(0, nc, len(x2)).astype(np.uint32)
    ids2 = np.arange(2 * 10 ** 6, 2 * 10 ** 6 + len(x2), dtype=np.uint32)
    e2 = g.encode(x2, precomputed_idx=p2)
    d_codes = torch.empty((len(x2), c["code_size"]), dtype=torch.uint8, device=dev)
    g.add_dev(len(x2), torch.from_numpy(x2.copy()).to(dev), torch.from_numpy(ids2.view(np.int32)).to(dev),
              d_precomputed_idx=torch.from_numpy(p2.view(np.int32)).to(dev), d_out_codes=d_codes)
    assert np.array_equal(d_codes.cpu().numpy(), e2[1])
    want = _csr_append(want, nc, p2, ids2, e2[1], e2[2])
    _assert_layout(g, want)
    f = gpu()
    _upload(f, c, want)
    assert _same_search(g.search(c["queries"], 1, 16, 2000, efSearch=40), f.search(c["queries"], 1, 16, 2000, efSearch=40))


def test_append_dev_equals_host_form(gpu):
    import torch
    c = corpus(**BASE)
    prefix, batches = _split(c, 21, 2)
    g = gpu()
    _upload(g, c, prefix)
    dev = torch.device("cuda", 0)
    for li, ids, codes, ncodes in batches:
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (li.view(np.int32), ids.view(np.int32), codes,
                                                                         ncodes)]
        g.append_ivf_dev(len(li), *t)
    _assert_layout(g, _full(c))


def test_errors_leave_the_tables(gpu, pkg):
    import torch
    c = corpus(**BASE)
    nc = len(c["offsets"]) - 1
    prefix, batches = _split(c, 7, 1)
    li, ids, codes, ncodes = batches[0]
    g = gpu()
    _upload(g, c, prefix)
    before = g.download_ivf()

    def unchanged():
        for a, b in zip(g.download_ivf(), before):
            assert np.array_equal(a, b)

    bad = li.copy()
    bad[len(bad) // 2] = nc
    with pytest.raises(pkg.IvfHnswError) as e:
        g.append_ivf(bad, ids, codes, ncodes)
    assert e.value.code == pkg.ERR_INVALID
    unchanged()
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (bad.view(np.int32), ids.view(np.int32), codes, ncodes)]
    with pytest.raises(pkg.IvfHnswError) as e:
        g.append_ivf_dev(len(bad), *t)
    assert e.value.code == pkg.ERR_INVALID
    unchanged()
    # on a view
    v = g.view()
    with pytest.raises(pkg.IvfHnswError) as e:
        v.append_ivf(li, ids, codes, ncodes)
    assert e.value.code == pkg.ERR_STATE
    v.close()
    unchanged()
    # code books that do not match the index (code size)
    g.upload_codebooks(c["d"], 8, np.zeros(256 * c["d"], np.float32), c["norm_table"])
    with pytest.raises(pkg.IvfHnswError) as e:
        g.add(c["base"][:10], np.arange(10, dtype=np.uint32), efSearch=40)
    assert e.value.code == pkg.ERR_INVALID
    unchanged()
    # OPQ in the code books only
    g.upload_codebooks(c["d"], c["code_size"], c["pq_centroids"], c["norm_table"], np.eye(c["d"], dtype=np.float32))
    with pytest.raises(pkg.IvfHnswError) as e:
        g.add(c["base"][:10], np.arange(10, dtype=np.uint32), efSearch=40)
    assert e.value.code == pkg.ERR_INVALID
    unchanged()
    # before upload_ivf
    h = gpu()
    with pytest.raises(pkg.IvfHnswError) as e:
        h.append_ivf(li, ids, codes, ncodes)
    assert e.value.code == pkg.ERR_STATE


def test_append_refused_on_grouping_handle(gpu, pkg):
    c = corpus(seed=41, nc=256, d=128, M=16, n_base=30000, nq=96, nsubc=16)
    g = gpu()
    _upload(g, c, _full(c))
    g.upload_grouping(c["nsubc"], c["alphas"], c["nn_centroid_idxs"], c["subgroup_sizes"], c["inter_centroid_dists"])
    before = g.download_ivf()
    with pytest.raises(pkg.IvfHnswError) as e:
        g.append_ivf(np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros((1, 16), np.uint8), np.zeros(1, np.uint8))
    assert e.value.code == pkg.ERR_STATE
    for a, b in zip(g.download_ivf(), before):
        assert np.array_equal(a, b)
