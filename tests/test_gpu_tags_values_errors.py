"""Every refusal of the tag-AND-value entry points, one by one, with its code; after each, a correct call
still answers right, earlier range results are kept and memory_bytes has not moved.  The refusals are argument and state
checks the library makes on the host before anything is launched: none dereferences a bad pointer."""
import ctypes as C

import numpy as np
import pytest

from conftest import corpus
import filter_ref
import tags_values_ref as tv
from test_gpu_remove import BASE, _upload, _same_search

pytestmark = pytest.mark.gpu

NPROBE, MAX_CODES, EF = tv.IVF_PARAMS


def _raises(pkg, code, call, word=None):
    with pytest.raises(pkg.IvfHnswError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if word:
        assert word in str(e.value)


def _same_range(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_refusals_leave_everything(gpu, pkg):
    import torch
    b = filter_ref.clipped(corpus(**BASE))
    asg = tv.assignment(b)
    g = tv.install(_upload(gpu(), b), asg)
    q = b["queries"]
    nq = len(q)
    qt, qr = tv.query_tags(nq), tv.query_ranges(nq)
    rows = {tv.key(p): g.tag_value_rows(tv.key(p)[0], *tv.key(p)[1]) for p in tv.PATTERN}
    assert rows == {tv.key(p): int(tv.passing_rows(b, asg, p).sum()) for p in tv.PATTERN}
    refs = tv.per_pair(tv.oracle_search(tv.IVF_PARAMS, 1), b, asg, q, 1)
    ref = tv.compose(refs, qt, qr)
    radius = float(np.median(g.search(q, 10, NPROBE, MAX_CODES, efSearch=EF)[0][:, 9]))
    rref = g.range_search_tags_values(q, radius, qt, qr, NPROBE, MAX_CODES, efSearch=EF)
    assert rref[0][-1] > 0
    assert _same_search(g.search_tags_values(q, 1, qt, qr, NPROBE, MAX_CODES, efSearch=EF), ref)
    g.range_search_tags_values(q, radius, qt, qr, NPROBE, MAX_CODES, efSearch=EF)
    mem = g.memory_bytes()

    def in_force(range_results_kept=True):
        if range_results_kept:  # an error leaves the earlier range results as they were
            d, l = g.range_results(0, int(rref[0][-1]))
            assert np.array_equal(l, rref[2]) and np.array_equal(d.view(np.uint32), rref[1].view(np.uint32))
        assert {k: g.tag_value_rows(k[0], *k[1]) for k in rows} == rows
        assert _same_search(g.search_tags_values(q, 1, qt, qr, NPROBE, MAX_CODES, efSearch=EF), ref)
        assert g.last_scan_kernel() == "scan_k1_kernel+tags+values"
        assert _same_range(g.range_search_tags_values(q, radius, qt, qr, NPROBE, MAX_CODES, efSearch=EF), rref)
        assert g.memory_bytes() == mem

    in_force()
    L = pkg.lib()
    dev = torch.device("cuda", 0)
    total = C.c_uint64(0)
    # tag_value_rows: a tag beyond 16 bits, a null result, a null handle
    _raises(pkg, pkg.ERR_INVALID, lambda: g.tag_value_rows(0x10000, 0, 1), "tag_value_rows")
    assert L.ivfhnsw_gpu_tag_value_rows(g._h, 0, 0, 5, None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_tag_value_rows(None, 0, 0, 5, C.byref(total)) == pkg.ERR_INVALID
    in_force()
    # misaligned device pointers (constructed, never dereferenced): query tags 2-byte, query ranges 8-byte
    d_q = torch.from_numpy(q).to(dev)
    dd = torch.empty((nq, 1), dtype=torch.float32, device=dev)
    ll = torch.empty((nq, 1), dtype=torch.int64, device=dev)
    d_qt = torch.from_numpy(np.concatenate([qt, qt[:1]]).view(np.int16)).to(dev)
    d_qr = torch.from_numpy(np.concatenate([qr, qr[:1]]).view(np.int32)).to(dev)
    d_lims = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    p = pkg.SearchParams(NPROBE, MAX_CODES, EF, 0, 0)
    for t_off, r_off, word in ((0, 4, "8-byte aligned"), (1, 0, "2-byte aligned")):
        assert L.ivfhnsw_gpu_search_tags_values_dev(g._h, nq, 1, d_q.data_ptr(), None, None, C.byref(p), d_qt.data_ptr() + t_off,
                                                    d_qr.data_ptr() + r_off, dd.data_ptr(), ll.data_ptr(), None) == pkg.ERR_INVALID
        msg = L.ivfhnsw_gpu_last_error().decode()
        assert word in msg and "search_tags_values_dev" in msg
        assert L.ivfhnsw_gpu_range_search_tags_values_dev(g._h, nq, d_q.data_ptr(), None, None, C.byref(p),
                                                          d_qt.data_ptr() + t_off, d_qr.data_ptr() + r_off, C.c_float(radius),
                                                          d_lims.data_ptr(), C.byref(total)) == pkg.ERR_INVALID
        msg = L.ivfhnsw_gpu_last_error().decode()
        assert word in msg and "range_search_tags_values_dev" in msg
    in_force()
    # null handle
    assert L.ivfhnsw_gpu_search_tags_values(None, 0, 1, None, None, None, C.byref(p), None, None, None, None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_range_search_tags_values(None, 0, None, None, None, C.byref(p), None, None, C.c_float(1.0), None,
                                                  C.byref(total)) == pkg.ERR_INVALID
    # what the plain call refuses is refused with its status
    _raises(pkg, pkg.ERR_INVALID, lambda: g.search_tags_values(q, 0, qt, qr, NPROBE, MAX_CODES, efSearch=EF))
    _raises(pkg, pkg.ERR_INVALID, lambda: g.search_tags_values(q, 1, qt, qr, 0, MAX_CODES, efSearch=EF))
    _raises(pkg, pkg.ERR_INVALID, lambda: g.range_search_tags_values(q, float("nan"), qt, qr, NPROBE, MAX_CODES, efSearch=EF))
    in_force()
    # a view searches with its parent's tables
    v = g.view()
    assert _same_search(v.search_tags_values(q, 1, qt, qr, NPROBE, MAX_CODES, efSearch=EF), ref)
    v.close()
    in_force()


def test_not_combined_with_the_handles_filter(gpu, pkg):
    b = filter_ref.clipped(corpus(**BASE))
    asg = tv.assignment(b)
    g = tv.install(_upload(gpu(), b), asg)
    q = b["queries"]
    qt, qr = tv.query_tags(len(q)), tv.query_ranges(len(q))
    pair = (0, tv.BAND31)
    ref = g.search_tags_values(q, 1, qt, qr, NPROBE, MAX_CODES, efSearch=EF)
    rref = g.range_search_tags_values(q, 1e30, qt, qr, NPROBE, MAX_CODES, efSearch=EF)
    g.set_filter(tv.labels_in(asg, pair))
    filtered = g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)  # plain calls go on, and read neither table
    assert g.last_scan_kernel() == "scan_k1_kernel+filter"
    _raises(pkg, pkg.ERR_STATE, lambda: g.search_tags_values(q, 1, qt, qr, NPROBE, MAX_CODES, efSearch=EF), "set_filter")
    _raises(pkg, pkg.ERR_STATE, lambda: g.range_search_tags_values(q, 1.0, qt, qr, NPROBE, MAX_CODES, efSearch=EF), "set_filter")
    d, l = g.range_results(0, int(rref[0][-1]))  # the refused range call left the earlier results
    assert np.array_equal(l, rref[2])
    assert _same_search(g.search_tags_values(q, 1, None, None, NPROBE, MAX_CODES, efSearch=EF), filtered)  # NULL, NULL: the plain call
    g.clear_filter()
    assert _same_search(g.search_tags_values(q, 1, qt, qr, NPROBE, MAX_CODES, efSearch=EF), ref)
    m = tv.mine(qt, qr, pair)
    assert m.any() and _same_search((ref[0][m], ref[1][m]), (filtered[0][m], filtered[1][m]))


def test_before_upload_and_on_a_shard(gpu, pkg):
    c = corpus(**BASE)
    nq = len(c["queries"])
    full = np.tile(np.array(tv.FULL, np.uint32), (nq, 1))
    none = np.full(nq, tv.TAG_NONE, np.uint16)
    h = gpu()
    _raises(pkg, pkg.ERR_STATE, lambda: h.search_tags_values(c["queries"], 1, none, full, 16, 2000, efSearch=40))
    # a shard of two
    world = 2
    off = c["offsets"].astype(np.int64)
    sel = np.concatenate([np.arange(off[cc], off[cc + 1]) for cc in range(0, c["nc"], world)]).astype(np.int64)
    s = gpu()
    s.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"][sel], c["codes"][sel], c["norm_codes"][sel],
                 c["centroid_norms"], c["pq_centroids"], c["norm_table"], shard_rank=0, shard_world=world)
    gr = c["graph"]
    s.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    _raises(pkg, pkg.ERR_STATE, lambda: s.search_tags_values(c["queries"], 1, none, full, 16, 2000, efSearch=40), "shard")
    _raises(pkg, pkg.ERR_STATE, lambda: s.range_search_tags_values(c["queries"], 1.0, none, full, 16, 2000, efSearch=40), "shard")
    # a handle that is no shard answers the same call
    g = _upload(gpu(), filter_ref.clipped(c))
    plain = g.search(c["queries"], 1, 16, 2000, efSearch=40)
    assert _same_search(g.search_tags_values(c["queries"], 1, none, full, 16, 2000, efSearch=40), plain)
