"""Removals by label from the lists a handle holds (ivfhnsw_gpu_remove_ids / _dev).

The expected state is always a numpy-filtered copy of the corpus (remove_ref.filter_lists): the handle must then hold,
byte for byte, what upload_ivf (and upload_grouping with the reduced sub-group sizes) of the remaining lists holds, and
searches must equal the oracle on the filtered corpus and a fresh upload of it: labels, distance bits, last_scan_counts."""
import numpy as np
import pytest

from conftest import corpus
import remove_ref
import synth

pytestmark = pytest.mark.gpu

BASE = dict(seed=11, nc=256, d=128, M=16, n_base=30000, nq=128)
CODE_SIZES = [dict(BASE, M=8), BASE, dict(BASE, M=32),
              dict(seed=81, nc=128, d=96, M=12, n_base=9000, nq=48, efConstruction=60, opq=True),
              dict(seed=85, nc=64, d=112, M=28, n_base=4000, nq=32, efConstruction=60, opq=True)]


def _upload(g, c, graph=True, grouping=True, **kw):
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"], opq_A=c["opq_A"], **kw)
    if grouping and c.get("nsubc"):
        g.upload_grouping(c["nsubc"], c["alphas"], c["nn_centroid_idxs"], c["subgroup_sizes"], c["inter_centroid_dists"])
    if graph:
        gr = c["graph"]
        g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    return g


def _assert_layout(g, want):
    off, ids, codes, ncodes = g.download_ivf()
    assert np.array_equal(off, np.asarray(want["offsets"], np.uint64))
    assert np.array_equal(ids, want["ids"])
    assert np.array_equal(codes, np.asarray(want["codes"]).reshape(codes.shape))
    assert np.array_equal(ncodes, want["norm_codes"])


def _same_search(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _labels(c, kind, seed=0):
    rng = np.random.default_rng(seed)
    ids = c["ids"]
    off = c["offsets"].astype(np.int64)
    if kind == "one":
        return ids[len(ids) // 3:len(ids) // 3 + 1].copy()
    if kind == "random30":
        return rng.choice(ids, int(0.3 * len(ids)), replace=False)
    if kind == "list":
        big = int(np.argmax(np.diff(off)))
        return ids[off[big]:off[big + 1]].copy()
    if kind == "all":
        return rng.permutation(ids)
    if kind == "absent":
        return (np.arange(200, dtype=np.uint32) + np.uint32(ids.max()) + np.uint32(1)).astype(np.uint32)
    if kind == "repeated":
        pick = rng.choice(ids, 500, replace=False)
        return np.concatenate([pick, pick[::2], pick[:7], pick[:7]]).astype(np.uint32)
    raise ValueError(kind)


def _remove_and_check(g, c, labels):
    want = remove_ref.filter_lists(c["offsets"], c["ids"], c["codes"], c["norm_codes"], labels,
                                   c.get("subgroup_sizes") if c.get("nsubc") else None)
    n, per = g.remove_ids(labels)
    assert n == int(want["removed"].sum())
    assert np.array_equal(per, want["removed"])
    _assert_layout(g, want)
    return want


@pytest.mark.parametrize("kw", CODE_SIZES, ids=lambda kw: "M%d" % kw["M"])
@pytest.mark.parametrize("kind", ["one", "random30", "list", "all", "absent", "repeated"])
def test_layout_equals_filtered_upload(gpu, kw, kind):
    c = corpus(**kw)
    g = _upload(gpu(), c, graph=False)
    want = _remove_and_check(g, c, _labels(c, kind, seed=kw["M"]))
    if kind == "absent":
        assert want["removed"].sum() == 0
    if kind == "all":
        assert len(want["ids"]) == 0


def _with_ids(c, ids):
    return dict(c, ids=np.ascontiguousarray(ids, np.uint32))


def test_label_held_in_several_lists(gpu):
    c0 = corpus(**BASE)
    c = _with_ids(c0, c0["ids"] % 700)          # every label in ~40 codes spread over many lists
    labels = np.array([0, 5, 77, 699, 123456], np.uint32)
    g = _upload(gpu(), c, graph=False)
    want = _remove_and_check(g, c, labels)
    assert (want["removed"] > 0).sum() > 20


def test_ids_above_2_31_layout_and_search(gpu):
    c0 = corpus(**BASE)
    c = _with_ids(c0, c0["ids"].astype(np.uint64) * 3 + 0x80000011)
    labels = np.random.default_rng(3).choice(c["ids"], 6000, replace=False)
    g = _upload(gpu(), c)
    _remove_and_check(g, c, labels)
    fc, _ = remove_ref.filtered_corpus(c, labels)
    f = _upload(gpu(), fc)
    ox = synth.oracle_index(fc)
    ox.set_params(16, 2000, 40)
    ref = ox.search_batch(c["queries"], k=1)
    got = g.search(c["queries"], 1, 16, 2000, efSearch=40)
    assert _same_search(got, ref[:2])
    assert _same_search(got, f.search(c["queries"], 1, 16, 2000, efSearch=40))
    assert g.last_scan_counts()[0] == ref[4].ncode


@pytest.mark.parametrize("removed", [True, False])
def test_id_0xffffffff(gpu, removed):
    c0 = corpus(**BASE)
    ids = c0["ids"].copy()
    ids[4321] = 0xffffffff
    c = _with_ids(c0, ids)
    labels = np.array([1, 2, 3, 20000] + ([0xffffffff] if removed else []), np.uint32)
    g = _upload(gpu(), c, graph=False)
    want = _remove_and_check(g, c, labels)
    assert (0xffffffff in want["ids"]) != removed


@pytest.mark.parametrize("kw", [BASE, CODE_SIZES[4]], ids=["pq16", "opq_M28"])
def test_search_equals_oracle_and_fresh_upload(gpu, kw):
    c = corpus(**kw)
    labels = _labels(c, "random30", seed=2)
    g = _upload(gpu(), c)
    _remove_and_check(g, c, labels)
    fc, _ = remove_ref.filtered_corpus(c, labels)
    f = _upload(gpu(), fc)
    ox = synth.oracle_index(fc)
    nprobe, ef = 16, 40
    # 250 codes: the max_codes cut falls inside shortened lists
    for k, max_codes, heap in ((1, 250, False), (1, 3000, False), (10, 2000, False), (10, 2000, True)):
        ox.set_params(nprobe, max_codes, ef)
        ref = ox.search_batch(c["queries"], k=k)
        got = g.search(c["queries"], k, nprobe, max_codes, efSearch=ef, heap_order=heap)
        if heap or k == 1:  # the oracle returns faiss's heap array
            assert _same_search(got, ref[:2]), (k, max_codes, heap)
        else:               # ascending order: the same k results
            assert np.array_equal(np.sort(got[1], axis=1), np.sort(ref[1], axis=1))
            assert np.array_equal(got[0].view(np.uint32), np.sort(ref[0], axis=1).view(np.uint32))
        if k == 1:
            assert g.last_scan_counts()[0] == ref[4].ncode
        fr = f.search(c["queries"], k, nprobe, max_codes, efSearch=ef, heap_order=heap)
        assert _same_search(got, fr)
        assert g.last_scan_counts() == f.last_scan_counts()


def test_every_code_removed_search_is_empty(gpu):
    c = corpus(**BASE)
    g = _upload(gpu(), c)
    _remove_and_check(g, c, _labels(c, "all"))
    d, lab = g.search(c["queries"], 1, 16, 2000, efSearch=40)
    assert (lab == -1).all() and (d == np.finfo(np.float32).max).all()
    assert g.last_scan_counts()[0] == 0
    d, lab = g.search(c["queries"], 10, 16, 2000, efSearch=40, heap_order=True)
    assert (lab == -1).all() and (d == np.finfo(np.float32).max).all()


def test_tail_kernel_after_prepare_latency(gpu):
    c = corpus(**BASE)
    labels = _labels(c, "random30", seed=5)
    g = _upload(gpu(), c)
    g.prepare_latency()
    g.search(c["queries"][:4], 1, 16, 2000, efSearch=40)   # the latency records exist before the removal
    _remove_and_check(g, c, labels)
    fc, _ = remove_ref.filtered_corpus(c, labels)
    ox = synth.oracle_index(fc)
    ox.set_params(16, 2000, 40)
    ref = ox.search_batch(c["queries"], k=1)
    for i in range(0, 32, 8):
        got = g.search(c["queries"][i:i + 8], 1, 16, 2000, efSearch=40)
        assert g.last_scan_kernel() == "ivf_tail_kernel"
        assert np.array_equal(got[1], ref[1][i:i + 8])
        assert np.array_equal(got[0].view(np.uint32), ref[0][i:i + 8].view(np.uint32))
    for x, rl, rd in zip(c["queries"][:6], ref[1], ref[0]):
        d1, l1 = g.search(x, 1, 16, 2000, efSearch=40)
        assert l1[0, 0] == rl[0] and d1[0, 0].view(np.uint32) == rd[0].view(np.uint32)


def test_large_batch_split_view_after_remove(gpu):
    import torch
    c = corpus(**BASE)
    labels = _labels(c, "random30", seed=6)
    g = _upload(gpu(), c)
    rng = np.random.default_rng(0)
    q = np.repeat(c["queries"], 72, axis=0)[:9000]
    q = q + rng.normal(0, 2.0, q.shape).astype(np.float32)
    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(np.ascontiguousarray(q)).to(dev)

    def run(h):
        d = torch.empty((len(q), 1), dtype=torch.float32, device=dev)
        lab = torch.empty((len(q), 1), dtype=torch.int64, device=dev)
        h.search_dev(len(q), 1, d_q, d, lab, 16, 2000, efSearch=40)
        h.sync()
        assert h.last_batch_parts()[1] > 0, "the batch did not take the two-part path"
        return d.cpu().numpy(), lab.cpu().numpy()

    run(g)  # the internal split view exists before the removal
    _remove_and_check(g, c, labels)
    fc, _ = remove_ref.filtered_corpus(c, labels)
    f = _upload(gpu(), fc)
    assert _same_search(run(g), run(f))


def test_remove_append_remove_sequence(gpu):
    c = corpus(**BASE)
    rng = np.random.default_rng(8)
    g = _upload(gpu(), c)
    l1 = rng.choice(c["ids"], 4000, replace=False)
    want = _remove_and_check(g, c, l1)
    # append 3000 new codes (new ids) to random lists, in add_batch's order
    nc = c["nc"]
    n = 3000
    li = rng.integers(0, nc, n).astype(np.uint32)
    ids = (np.arange(n) + 10 ** 6).astype(np.uint32)
    codes = rng.integers(0, 256, (n, c["code_size"])).astype(np.uint8)
    ncodes = rng.integers(0, 256, n).astype(np.uint8)
    g.append_ivf(li, ids, codes, ncodes)
    from test_gpu_append import _csr_append
    cur = _csr_append((want["offsets"], want["ids"], want["codes"], want["norm_codes"]), nc, li, ids, codes, ncodes)
    cc = dict(c, offsets=cur[0], ids=cur[1], codes=cur[2], norm_codes=cur[3])
    l2 = np.concatenate([rng.choice(cur[1], 5000, replace=False), ids[:50]])
    final = _remove_and_check(g, cc, l2)
    fc = dict(c, offsets=final["offsets"], ids=final["ids"], codes=final["codes"], norm_codes=final["norm_codes"])
    f = _upload(gpu(), fc)
    ox = synth.oracle_index(fc)
    ox.set_params(16, 2000, 40)
    ref = ox.search_batch(c["queries"], k=1)
    got = g.search(c["queries"], 1, 16, 2000, efSearch=40)
    assert _same_search(got, ref[:2])
    assert _same_search(got, f.search(c["queries"], 1, 16, 2000, efSearch=40))
    assert g.last_scan_counts() == f.last_scan_counts()


def test_remove_dev_equals_host_form(gpu):
    import torch
    c = corpus(**BASE)
    labels = _labels(c, "random30", seed=9)
    a = _upload(gpu(), c, graph=False)
    b = _upload(gpu(), c, graph=False)
    n_a, per_a = a.remove_ids(labels)
    dev = torch.device("cuda", 0)
    d_lab = torch.from_numpy(labels.astype(np.uint32).view(np.int32)).to(dev)
    d_per = torch.full((c["nc"],), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    n_b = b.remove_ids_dev(len(labels), d_lab, d_per)
    assert n_a == n_b
    assert np.array_equal(per_a, d_per.cpu().numpy().view(np.uint32))
    for x, y in zip(a.download_ivf(), b.download_ivf()):
        assert np.array_equal(x, y)
    # nothing to remove: zero counts, no change
    d_per.fill_(-1)
    torch.cuda.synchronize(dev)
    assert b.remove_ids_dev(0, None, d_per) == 0
    assert (d_per.cpu().numpy() == 0).all()


GROUPING = [dict(seed=42, nc=128, d=128, M=16, n_base=20000, nq=64, nsubc=64),
            dict(seed=43, nc=256, d=96, M=16, n_base=20000, nq=64, nsubc=8),
            dict(seed=45, nc=128, d=128, M=16, n_base=12000, nq=64, nsubc=32, opq=True),
            dict(seed=46, nc=128, d=128, M=16, n_base=12000, nq=64, nsubc=8, opq=True)]


def _grouping_labels(c, seed):
    """30 % at random, plus every code of one group and of a few whole sub-groups."""
    rng = np.random.default_rng(seed)
    off = c["offsets"].astype(np.int64)
    sg = c["subgroup_sizes"].astype(np.int64)
    lab = [rng.choice(c["ids"], int(0.3 * len(c["ids"])), replace=False)]
    big = int(np.argmax(np.diff(off)))
    lab.append(c["ids"][off[big]:off[big + 1]])
    for cc in rng.choice(np.nonzero(np.diff(off) > 0)[0], 6, replace=False):
        j = int(np.argmax(sg[cc]))
        a = off[cc] + sg[cc, :j].sum()
        lab.append(c["ids"][a:a + sg[cc, j]])
    return np.concatenate(lab).astype(np.uint32), big


@pytest.mark.parametrize("kw", GROUPING, ids=lambda kw: "nsubc%d%s" % (kw["nsubc"], "_opq" if kw.get("opq") else ""))
def test_grouping_remove(gpu, kw):
    c = corpus(**kw)
    labels, big = _grouping_labels(c, kw["seed"])
    g = _upload(gpu(), c)
    want = _remove_and_check(g, c, labels)
    sizes = g.download_grouping()
    assert np.array_equal(sizes, want["subgroup_sizes"])
    assert sizes[big].sum() == 0
    assert (sizes < c["subgroup_sizes"]).any() and ((sizes == 0) & (c["subgroup_sizes"] > 0)).any()
    fc, _ = remove_ref.filtered_corpus(c, labels)
    f = _upload(gpu(), fc)
    assert np.array_equal(f.download_grouping(), sizes)
    ox = synth.oracle_index(fc)
    for pruning in (False, True):
        for max_codes in (600, 10 ** 9):
            ox.set_params(16, max_codes, 64, do_pruning=pruning)
            ref = ox.search_batch(c["queries"], k=1)
            got = g.search(c["queries"], 1, 16, max_codes, efSearch=64, do_pruning=pruning)
            assert _same_search(got, ref[:2]), (pruning, max_codes)
            assert g.last_scan_counts()[0] == ref[4].ncode
            fr = f.search(c["queries"], 1, 16, max_codes, efSearch=64, do_pruning=pruning)
            assert _same_search(got, fr)
            assert g.last_scan_counts() == f.last_scan_counts()


def test_grouping_remove_every_code(gpu):
    c = corpus(**GROUPING[0])
    g = _upload(gpu(), c)
    _remove_and_check(g, c, c["ids"])
    assert (g.download_grouping() == 0).all()
    d, lab = g.search(c["queries"], 1, 8, 600, efSearch=80, do_pruning=True)
    assert (lab == -1).all() and g.last_scan_counts()[0] == 0


def test_errors_leave_the_tables(gpu, pkg):
    c = corpus(**BASE)
    labels = _labels(c, "random30", seed=1)
    g = _upload(gpu(), c)
    before = g.download_ivf()
    ref = g.search(c["queries"], 1, 16, 2000, efSearch=40)

    def unchanged(h=g, b=before, r=ref):
        for x, y in zip(h.download_ivf(), b):
            assert np.array_equal(x, y)
        assert _same_search(h.search(c["queries"], 1, 16, 2000, efSearch=40), r)

    v = g.view()
    with pytest.raises(pkg.IvfHnswError) as e:
        v.remove_ids(labels)
    assert e.value.code == pkg.ERR_STATE
    v.close()
    unchanged()
    rc = pkg.lib().ivfhnsw_gpu_remove_ids(g._h, 5, None, None, None)
    assert rc == pkg.ERR_INVALID
    unchanged()
    with pytest.raises(pkg.IvfHnswError) as e:
        g.remove_ids_dev(5, None)
    assert e.value.code == pkg.ERR_INVALID
    unchanged()
    with pytest.raises(pkg.IvfHnswError) as e:
        g.download_grouping()
    assert e.value.code == pkg.ERR_STATE
    h = gpu()
    with pytest.raises(pkg.IvfHnswError) as e:
        h.remove_ids(labels)
    assert e.value.code == pkg.ERR_STATE
    # a shard of three
    world = 3
    off = c["offsets"].astype(np.int64)
    sel = np.concatenate([np.arange(off[cc], off[cc + 1]) for cc in range(0, c["nc"], world)]).astype(np.int64)
    s = gpu()
    s.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"][sel], c["codes"][sel], c["norm_codes"][sel],
                 c["centroid_norms"], c["pq_centroids"], c["norm_table"], shard_rank=0, shard_world=world)
    s_before = s.download_ivf()
    with pytest.raises(pkg.IvfHnswError) as e:
        s.remove_ids(labels)
    assert e.value.code == pkg.ERR_STATE and "shard" in str(e.value)
    for x, y in zip(s.download_ivf(), s_before):
        assert np.array_equal(x, y)


def test_scale_synthetic_2_24_codes(gpu):
    import torch
    nc, M = 65536, 16
    tb = synth.make_throughput_tables(5, nc, 128, M, 1 << 24)
    off = tb["offsets"]
    n = int(off[-1])
    g = gpu()
    g.upload_ivf_synthetic(128, M, off, np.zeros(nc, np.float32), tb["pq_centroids"], tb["norm_table"], seed=77)
    rng = np.random.default_rng(4)
    labels = rng.choice(n, n // 100, replace=False).astype(np.uint32)
    dev = torch.device("cuda", 0)
    n_rm = g.remove_ids_dev(len(labels), torch.from_numpy(labels.view(np.int32)).to(dev))
    assert n_rm == len(labels)
    o2, ids, codes, ncodes = g.download_ivf()
    assert np.array_equal(ids, np.setdiff1d(np.arange(n, dtype=np.uint32), labels))
    sizes = np.diff(off.astype(np.int64))
    lid = np.repeat(np.arange(nc), sizes)
    rem = np.bincount(lid[labels.astype(np.int64)], minlength=nc)
    assert np.array_equal(o2, np.concatenate([[0], np.cumsum(sizes - rem)]).astype(np.uint64))
    sample = np.sort(rng.choice(nc, 64, replace=False))
    gidx, sc, sn = synth.synthetic_codes_lists(77, off, M, sample)
    keep = ~np.isin(gidx, labels)
    rows = np.concatenate([np.arange(o2[cc], o2[cc + 1]) for cc in sample]).astype(np.int64)
    assert np.array_equal(ids[rows], gidx[keep])
    assert np.array_equal(codes[rows], sc[keep])
    assert np.array_equal(ncodes[rows], sn[keep])
