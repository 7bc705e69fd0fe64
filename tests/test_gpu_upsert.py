"""Upserts on the lists a handle holds (ivfhnsw_gpu_upsert_ivf / _dev, ivfhnsw_gpu_upsert / _dev).

The expected state is always upsert_ref.upsert_lists -- remove_ref.filter_lists of the batch's labels, then a stable append
per list: the handle must hold it byte for byte, report the reference's removal counts, and hold the same bytes as a second
handle that ran remove_ids followed by append_ivf.  Searches equal the oracle on the numpy-updated corpus and a fresh upload
of it (labels, distance bits, last_scan_counts); filter, filter slots and row tags, all keyed by label, stand as they do on
the second handle."""
import numpy as np
import pytest

from conftest import corpus
import remove_ref
import synth
import upsert_ref
from test_gpu_remove import BASE, CODE_SIZES, _assert_layout, _same_search, _upload, _with_ids

pytestmark = pytest.mark.gpu

KINDS = ["one", "present_same_list", "present_moved", "absent", "mixed", "whole_list", "all"]
OPQ12 = CODE_SIZES[3]


def _row_lists(c):
    off = c["offsets"].astype(np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def _with_an_empty_list(c):
    """c with its shortest list emptied (numpy): (corpus, that list)."""
    off = c["offsets"].astype(np.int64)
    short = int(np.argmin(np.diff(off)))
    fc, _ = remove_ref.filtered_corpus(c, c["ids"][off[short]:off[short + 1]])
    return fc, short


def _payload(rng, n, M):
    return rng.integers(0, 256, (n, M)).astype(np.uint8), rng.integers(0, 255, n).astype(np.uint8)


def _batch(c, kind, seed=0, empty=None):
    """(list_idx, ids, codes, norm_codes) of one upsert on corpus c (unique ids)."""
    rng = np.random.default_rng(seed)
    ids, nc, M = c["ids"], c["nc"], c["code_size"]
    lid = _row_lists(c)
    off = c["offsets"].astype(np.int64)
    fresh = np.uint32(int(ids.max()) + 1)
    if kind == "one":
        r = np.array([len(ids) // 3])
        lab, li = ids[r], lid[r]
    elif kind in ("present_same_list", "present_moved"):
        r = rng.choice(len(ids), len(ids) // 5, replace=False)
        lab, li = ids[r], lid[r]
        if kind == "present_moved":
            li = (li + rng.integers(1, nc, len(r))) % nc
            assert (li != lid[r]).all()
    elif kind == "absent":
        lab = (np.arange(1500, dtype=np.uint32) + fresh).astype(np.uint32)
        li = rng.integers(0, nc, len(lab))
    elif kind == "mixed":
        r = rng.choice(len(ids), 1500, replace=False)
        lab = rng.permutation(np.concatenate([ids[r], np.arange(1500, dtype=np.uint32) + fresh]).astype(np.uint32))
        li = rng.integers(0, nc, len(lab))
    elif kind == "whole_list":
        big = int(np.argmax(np.diff(off)))
        lab = ids[off[big]:off[big + 1]].copy()
        assert empty is not None and off[empty + 1] == off[empty] and empty != 0
        li = np.where(np.arange(len(lab)) % 2 == 0, 0, empty)
    elif kind == "all":
        lab = rng.permutation(ids)
        li = rng.integers(0, nc, len(lab))
    else:
        raise ValueError(kind)
    assert len(np.unique(lab)) == len(lab)
    return (np.asarray(li, np.uint32), np.asarray(lab, np.uint32)) + _payload(rng, len(lab), M)


def _upsert_and_check(g, c, batch, twin=None):
    """upsert_ivf on g against the reference; twin: a handle on the same lists that runs remove_ids + append_ivf."""
    fc, want = upsert_ref.upserted_corpus(c, *batch)
    n, per = g.upsert_ivf(*batch)
    assert n == int(want["removed"].sum())
    assert np.array_equal(per, want["removed"])
    _assert_layout(g, want)
    if twin is not None:
        twin.remove_ids(batch[1])
        twin.append_ivf(*batch)
        for x, y in zip(g.download_ivf(), twin.download_ivf()):
            assert np.array_equal(x, y)
    return fc, want


# ---- 1. layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CODE_SIZES, ids=lambda kw: "M%d" % kw["M"])
@pytest.mark.parametrize("kind", KINDS)
def test_layout_equals_remove_then_append(gpu, kw, kind):
    c, empty = corpus(**kw), None
    if kind == "whole_list":
        c, empty = _with_an_empty_list(c)
    batch = _batch(c, kind, seed=kw["M"], empty=empty)
    g, t = _upload(gpu(), c, graph=False), _upload(gpu(), c, graph=False)
    _, want = _upsert_and_check(g, c, batch, twin=t)
    if kind == "absent":
        assert want["removed"].sum() == 0
    if kind in ("all", "present_moved"):
        assert want["removed"].sum() == len(batch[1])
    if kind == "whole_list":
        off = want["offsets"].astype(np.int64)
        assert off[empty + 1] - off[empty] == len(batch[1]) // 2


# ---- 2. tile edges --------------------------------------------------------------------------------------------------------
def _first_rows(c, n):
    off = np.minimum(c["offsets"].astype(np.int64), n).astype(np.uint64)
    return dict(c, offsets=off, ids=c["ids"][:n].copy(), codes=np.asarray(c["codes"]).reshape(len(c["ids"]), -1)[:n].copy(),
                norm_codes=c["norm_codes"][:n].copy())


@pytest.mark.parametrize("kw", [BASE, OPQ12], ids=["M16", "M12"])
@pytest.mark.parametrize("rows", [4096, 4097])
def test_tile_edges(gpu, kw, rows):
    c = _first_rows(corpus(**kw), rows)       # the last source tile is full / holds one row
    assert len(c["ids"]) == rows
    rng = np.random.default_rng(rows)
    r = rng.choice(rows, 1001, replace=False)
    lab = np.concatenate([c["ids"][r], np.arange(3, dtype=np.uint32) + np.uint32(10 ** 6)]).astype(np.uint32)
    li = rng.integers(0, c["nc"], len(lab)).astype(np.uint32)
    batch = (li, lab) + _payload(rng, len(lab), c["code_size"])
    g, t = _upload(gpu(), c, graph=False), _upload(gpu(), c, graph=False)
    _, want = _upsert_and_check(g, c, batch, twin=t)
    starts = want["offsets"][:-1].astype(np.int64)
    assert (starts % 4 != 0).sum() > 10, "the new list starts do not leave the 16-byte groups"


# ---- 3. labels ------------------------------------------------------------------------------------------------------------
def test_label_held_in_several_lists(gpu):
    c0 = corpus(**BASE)
    c = _with_ids(c0, c0["ids"] % 700)          # every label in ~40 codes spread over many lists
    rng = np.random.default_rng(1)
    lab = np.array([0, 5, 77, 699, 123456], np.uint32)
    batch = (rng.integers(0, c["nc"], len(lab)).astype(np.uint32), lab) + _payload(rng, len(lab), c["code_size"])
    g, t = _upload(gpu(), c, graph=False), _upload(gpu(), c, graph=False)
    _, want = _upsert_and_check(g, c, batch, twin=t)
    assert (want["removed"] > 0).sum() > 20 and want["removed"].sum() > 100
    for l in lab:
        assert (want["ids"] == l).sum() == 1     # all of them went, one came


def test_ids_above_2_31(gpu):
    c0 = corpus(**BASE)
    c = _with_ids(c0, c0["ids"].astype(np.uint64) * 3 + 0x80000011)
    g, t = _upload(gpu(), c, graph=False), _upload(gpu(), c, graph=False)
    _upsert_and_check(g, c, _batch(c, "mixed", seed=3), twin=t)


@pytest.mark.parametrize("resident", [True, False])
def test_label_0xffffffff(gpu, resident):
    c0 = corpus(**BASE)
    ids = c0["ids"].copy()
    if resident:
        ids[4321] = 0xffffffff
    c = _with_ids(c0, ids)
    rng = np.random.default_rng(4)
    lab = np.array([1, 2, 0xffffffff, 3, 20000], np.uint32)
    batch = (rng.integers(0, c["nc"], len(lab)).astype(np.uint32), lab) + _payload(rng, len(lab), c["code_size"])
    g, t = _upload(gpu(), c, graph=False), _upload(gpu(), c, graph=False)
    _, want = _upsert_and_check(g, c, batch, twin=t)
    assert (want["ids"] == 0xffffffff).sum() == 1


# ---- 4. the empty index ---------------------------------------------------------------------------------------------------
def test_upsert_into_an_empty_index_is_an_append(gpu):
    c = corpus(**BASE)
    g, t = _upload(gpu(), c, graph=False), _upload(gpu(), c, graph=False)
    for h in (g, t):
        assert h.remove_ids(c["ids"])[0] == len(c["ids"])
    ec, _ = remove_ref.filtered_corpus(c, c["ids"])
    batch = _batch(c, "mixed", seed=5)
    n, per = g.upsert_ivf(*batch)
    assert n == 0 and not per.any()
    t.append_ivf(*batch)
    for x, y in zip(g.download_ivf(), t.download_ivf()):
        assert np.array_equal(x, y)
    _assert_layout(g, upsert_ref.upsert_lists(ec["offsets"], ec["ids"], ec["codes"], ec["norm_codes"], *batch))


# ---- 5. searches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [BASE, OPQ12], ids=["pq16", "opq_M12"])
def test_search_equals_oracle_and_fresh_upload(gpu, kw):
    c = corpus(**kw)
    g = _upload(gpu(), c)
    fc, _ = _upsert_and_check(g, c, _batch(c, "mixed", seed=2))
    f = _upload(gpu(), fc)
    ox = synth.oracle_index(fc)
    nprobe, max_codes, ef = 16, 2000, 40
    ox.set_params(nprobe, max_codes, ef)
    for k, heap in ((1, False), (10, True)):
        ref = ox.search_batch(c["queries"], k=k)
        got = g.search(c["queries"], k, nprobe, max_codes, efSearch=ef, heap_order=heap)
        assert _same_search(got, ref[:2]), k
        if k == 1:
            assert g.last_scan_counts()[0] == ref[4].ncode
        assert _same_search(got, f.search(c["queries"], k, nprobe, max_codes, efSearch=ef, heap_order=heap))
        assert g.last_scan_counts() == f.last_scan_counts()
    radius = float(np.median(f.search(c["queries"], 10, nprobe, max_codes, efSearch=ef)[0][:, 9]))
    a = g.range_search(c["queries"], radius, nprobe, max_codes, efSearch=ef)
    b = f.range_search(c["queries"], radius, nprobe, max_codes, efSearch=ef)
    assert int(a[0][-1]) > 0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ---- 6. upsert of vectors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [BASE, OPQ12], ids=["pq16", "opq_M12"])
@pytest.mark.parametrize("precomputed", [False, True], ids=["assign", "precomputed_idx"])
def test_upsert_vectors_equals_encode_then_upsert_ivf(gpu, kw, precomputed):
    c = corpus(**kw)
    rng = np.random.default_rng(6)
    n = 1200
    x = (c["base"][rng.integers(0, len(c["base"]), n)] + rng.normal(0, 3.0, (n, c["d"]))).astype(np.float32)
    lab = np.concatenate([rng.choice(c["ids"], n // 2, replace=False), np.arange(n - n // 2, dtype=np.uint32) + np.uint32(10 ** 6)])
    lab = rng.permutation(lab.astype(np.uint32))
    pidx = rng.integers(0, c["nc"], n).astype(np.uint32) if precomputed else None
    a, b = _upload(gpu(), c), _upload(gpu(), c)
    for h in (a, b):
        h.upload_codebooks(c["d"], c["code_size"], c["pq_centroids"], c["norm_table"], c["opq_A"])
    idx, codes, ncodes = b.encode(x, precomputed_idx=pidx, efSearch=40)
    n_b, _ = b.upsert_ivf(idx, lab, codes, ncodes)
    got = a.upsert(x, lab, precomputed_idx=pidx, efSearch=40)
    assert np.array_equal(got[0], idx) and np.array_equal(got[1], codes) and np.array_equal(got[2], ncodes)
    assert got[3] == n_b == n // 2
    if precomputed:
        assert np.array_equal(idx, pidx)
    for u, v in zip(a.download_ivf(), b.download_ivf()):
        assert np.array_equal(u, v)
    _assert_layout(a, upsert_ref.upsert_lists(c["offsets"], c["ids"], c["codes"], c["norm_codes"], idx, lab, codes, ncodes))


# ---- 7. the _dev forms ----------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(view)).to(torch.device("cuda", 0))


def test_dev_forms_equal_host_forms(gpu):
    import torch
    c = corpus(**BASE)
    dev = torch.device("cuda", 0)
    batch = _batch(c, "mixed", seed=7)
    a, b = _upload(gpu(), c), _upload(gpu(), c)
    n_a, per_a = a.upsert_ivf(*batch)
    d_per = torch.full((c["nc"],), -1, dtype=torch.int32, device=dev)
    d_batch = [_dev(x) for x in batch]
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    n_b = b.upsert_ivf_dev(len(batch[1]), *d_batch, d_removed_per_list=d_per)
    assert n_a == n_b == 1500
    assert np.array_equal(per_a, d_per.cpu().numpy().view(np.uint32))
    for x, y in zip(a.download_ivf(), b.download_ivf()):
        assert np.array_equal(x, y)
    # n = 0: zero counts, no change
    d_per.fill_(-1)
    torch.cuda.synchronize(dev)
    assert b.upsert_ivf_dev(0, None, None, None, None, d_removed_per_list=d_per) == 0
    assert (d_per.cpu().numpy() == 0).all()
    for x, y in zip(a.download_ivf(), b.download_ivf()):
        assert np.array_equal(x, y)
    # upsert_dev against upsert
    rng = np.random.default_rng(8)
    n = 700
    x = (c["base"][rng.integers(0, len(c["base"]), n)] + rng.normal(0, 3.0, (n, c["d"]))).astype(np.float32)
    now = a.download_ivf()[1]
    lab = rng.permutation(np.concatenate([rng.choice(now, n // 2, replace=False),
                                          np.arange(n - n // 2, dtype=np.uint32) + np.uint32(2 * 10 ** 6)]).astype(np.uint32))
    for h in (a, b):
        h.upload_codebooks(c["d"], c["code_size"], c["pq_centroids"], c["norm_table"], c["opq_A"])
    idx, codes, ncodes, n_a = a.upsert(x, lab, efSearch=40)
    d_idx = torch.empty((n,), dtype=torch.int32, device=dev)
    d_codes = torch.empty((n, c["code_size"]), dtype=torch.uint8, device=dev)
    d_nc = torch.empty((n,), dtype=torch.uint8, device=dev)
    d_x, d_lab = _dev(x), _dev(lab)
    torch.cuda.synchronize(dev)
    n_b = b.upsert_dev(n, d_x, d_lab, efSearch=40, d_out_idx=d_idx, d_out_codes=d_codes, d_out_norm_codes=d_nc)
    assert n_a == n_b == n // 2
    assert np.array_equal(d_idx.cpu().numpy().view(np.uint32), idx) and np.array_equal(d_codes.cpu().numpy(), codes)
    assert np.array_equal(d_nc.cpu().numpy(), ncodes)
    for u, v in zip(a.download_ivf(), b.download_ivf()):
        assert np.array_equal(u, v)


# ---- 8. state keyed by label ----------------------------------------------------------------------------------------------
def test_filter_slots_and_tags_stand(gpu, pkg):
    c = corpus(**BASE)
    rng = np.random.default_rng(9)
    q = c["queries"]
    batch = _batch(c, "mixed", seed=9)
    new = batch[1][batch[1] > c["ids"].max()]
    uniq = np.unique(c["ids"])
    allow = np.concatenate([rng.choice(uniq, len(uniq) // 2, replace=False), new[::2]]).astype(np.uint32)
    slots = {0: (rng.choice(uniq, len(uniq) // 3, replace=False), False), 5: (np.concatenate([uniq[::7], new[::3]]), True),
             31: (np.concatenate([uniq[::50], new]), False)}
    tl = np.concatenate([uniq, new]).astype(np.uint32)
    tags = (tl % 5).astype(np.uint16)
    qs = np.array([(0, 5, 31, pkg.SLOT_NONE)[i % 4] for i in range(len(q))], np.uint8)
    qt = np.array([(0, 1, 4, pkg.TAG_NONE)[i % 4] for i in range(len(q))], np.uint16)
    g, t = _upload(gpu(), c), _upload(gpu(), c)
    for h in (g, t):
        for s, (labels, deny) in slots.items():
            h.set_filter_slot(s, labels, deny=deny)
        h.set_tags(tl, tags)
    for deny in (False, True):
        for h in (g, t):
            h.set_filter(allow, deny=deny)
        b = batch if not deny else _batch(dict(c, ids=g.download_ivf()[1], offsets=g.download_ivf()[0]), "present_moved", seed=10)
        before = (g.filter_info()[0], [g.filter_slot_info(s)[0] for s in slots], g.tags_info()[2])
        g.upsert_ivf(*b)
        t.remove_ids(b[1])
        t.append_ivf(*b)
        ids_now = g.download_ivf()[1]
        assert np.array_equal(ids_now, t.download_ivf()[1])
        assert (g.filter_info()[0], [g.filter_slot_info(s)[0] for s in slots], g.tags_info()[2]) == before
        assert g.filter_info() == t.filter_info() == (int(deny), int((np.isin(ids_now, allow) != deny).sum()), len(ids_now))
        for s, (labels, sdeny) in slots.items():
            assert g.filter_slot_info(s) == t.filter_slot_info(s) == (int(sdeny), int((np.isin(ids_now, labels) != sdeny).sum()),
                                                                      len(ids_now))
        assert g.tags_info() == t.tags_info()
        for tag in range(5):
            assert g.tag_rows(tag) == t.tag_rows(tag) == int((ids_now % 5 == tag).sum())
        for k, heap in ((1, False), (10, True)):
            kw = dict(efSearch=40, heap_order=heap)
            assert _same_search(g.search(q, k, 16, 2000, **kw), t.search(q, k, 16, 2000, **kw))
            assert g.last_scan_kernel().endswith("+filter")
        for h in (g, t):   # a call is filtered by set_filter or by slots / tags, not both
            h.clear_filter()
        for k, heap in ((1, False), (10, True)):
            kw = dict(efSearch=40, heap_order=heap)
            assert _same_search(g.search_slots(q, k, qs, 16, 2000, **kw), t.search_slots(q, k, qs, 16, 2000, **kw))
            assert _same_search(g.search_tags(q, k, qt, 16, 2000, **kw), t.search_tags(q, k, qt, 16, 2000, **kw))
            lab = g.search_tags(q, k, qt, 16, 2000, **kw)[1]
            want = np.broadcast_to(qt[:, None], lab.shape)
            found = (lab >= 0) & (want != pkg.TAG_NONE)
            assert found.any() and (lab[found] % 5 == want[found]).all()
