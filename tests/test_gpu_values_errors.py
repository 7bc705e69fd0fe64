"""Every refusal of the row-value entry points, with its code; after each, the values answer as before,
shown by a search and a range search, and memory_bytes follows the contract's formula.  The refusals are argument checks
the library makes on the host, or on the device over valid buffers before anything changes: none launches a kernel on a
bad pointer.  (IVFHNSW_ERR_NOMEM needs an allocation to fail, which a test cannot arrange without exhausting the device;
the path is the one set_tags has: the new table and the new row values are allocated and filled before the installed ones
are touched.)"""
import ctypes as C

import numpy as np
import pytest

from conftest import corpus
import filter_ref
import values_ref as vr
from test_gpu_remove import BASE, _upload, _same_search

pytestmark = pytest.mark.gpu

NPROBE, MAX_CODES, EF = vr.IVF_PARAMS
NONE = vr.NONE


def _raises(pkg, code, call, word=None):
    with pytest.raises(pkg.IvfHnswError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if word:
        assert word in str(e.value)


def _same_range(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_refusals_leave_the_values(gpu, pkg):
    import torch
    b = filter_ref.clipped(corpus(**BASE))
    asg = vr.assignment(b)
    g = vr.install(_upload(gpu(), b), asg)
    q = b["queries"]
    qr = vr.query_ranges(len(q))
    info = g.values_info()
    rows = {r: g.value_rows(*r) for r in vr.PATTERN}
    ref = g.search_values(q, 1, qr, NPROBE, MAX_CODES, efSearch=EF)
    radius = float(np.median(g.search(q, 10, NPROBE, MAX_CODES, efSearch=EF)[0][:, 9]))
    rref = g.range_search_values(q, radius, qr, NPROBE, MAX_CODES, efSearch=EF)
    assert rref[0][-1] > 0
    mem = g.memory_bytes()

    def in_force(range_results_kept=True):
        if range_results_kept:  # an error leaves the earlier range results as they were
            d, l = g.range_results(0, int(rref[0][-1]))
            assert np.array_equal(l, rref[2]) and np.array_equal(d.view(np.uint32), rref[1].view(np.uint32))
        assert g.values_info() == info and {r: g.value_rows(*r) for r in rows} == rows
        assert _same_search(g.search_values(q, 1, qr, NPROBE, MAX_CODES, efSearch=EF), ref)
        assert g.last_scan_kernel() == "scan_k1_kernel+values"
        assert _same_range(g.range_search_values(q, radius, qr, NPROBE, MAX_CODES, efSearch=EF), rref)
        assert g.memory_bytes() == mem

    in_force()
    L = pkg.lib()
    labels, values = vr.valued(asg)
    dev = torch.device("cuda", 0)
    # conflicting repeats: one label, two different values -- among thousands of valid entries, host and device form
    lab2 = np.concatenate([labels[:4000], labels[17:18]]).astype(np.uint32)
    val2 = np.concatenate([np.full(4000, 7, np.uint32), np.array([0x80000007], np.uint32)])
    _raises(pkg, pkg.ERR_INVALID, lambda: g.set_values(lab2, val2), "two different values")
    in_force()
    d_lab = torch.from_numpy(np.concatenate([lab2, lab2[:1]]).view(np.int32)).to(dev)
    d_val = torch.from_numpy(np.concatenate([val2, val2[:1]]).view(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    _raises(pkg, pkg.ERR_INVALID, lambda: g.set_values_dev(len(lab2), d_lab, d_val), "two different values")
    in_force()
    # NULL pointers with n > 0
    assert L.ivfhnsw_gpu_set_values(g._h, 5, None, val2.ctypes.data) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_set_values(g._h, 5, lab2.ctypes.data, None) == pkg.ERR_INVALID
    assert "null values" in L.ivfhnsw_gpu_last_error().decode()
    assert L.ivfhnsw_gpu_set_values_dev(g._h, 5, None, d_val.data_ptr()) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_set_values_dev(g._h, 5, d_lab.data_ptr(), None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_value_rows(g._h, 0, 5, None) == pkg.ERR_INVALID
    in_force()
    # misaligned device pointers (constructed, never dereferenced): labels and values 4-byte, query ranges 8-byte
    assert L.ivfhnsw_gpu_set_values_dev(g._h, 100, d_lab.data_ptr() + 2, d_val.data_ptr()) == pkg.ERR_INVALID
    assert "aligned" in L.ivfhnsw_gpu_last_error().decode()
    assert L.ivfhnsw_gpu_set_values_dev(g._h, 100, d_lab.data_ptr(), d_val.data_ptr() + 2) == pkg.ERR_INVALID
    assert "aligned" in L.ivfhnsw_gpu_last_error().decode()
    d_q = torch.from_numpy(q).to(dev)
    dd = torch.empty((len(q), 1), dtype=torch.float32, device=dev)
    ll = torch.empty((len(q), 1), dtype=torch.int64, device=dev)
    d_qr = torch.from_numpy(np.concatenate([qr, qr[:1]]).view(np.int32)).to(dev)
    d_lims = torch.zeros(len(q) + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    p = pkg.SearchParams(NPROBE, MAX_CODES, EF, 0, 0)
    total = C.c_uint64(0)
    assert L.ivfhnsw_gpu_search_values_dev(g._h, len(q), 1, d_q.data_ptr(), None, None, C.byref(p), d_qr.data_ptr() + 4,
                                           dd.data_ptr(), ll.data_ptr(), None) == pkg.ERR_INVALID
    assert "8-byte aligned" in L.ivfhnsw_gpu_last_error().decode()
    assert L.ivfhnsw_gpu_range_search_values_dev(g._h, len(q), d_q.data_ptr(), None, None, C.byref(p), d_qr.data_ptr() + 4,
                                                 C.c_float(radius), d_lims.data_ptr(), C.byref(total)) == pkg.ERR_INVALID
    assert "8-byte aligned" in L.ivfhnsw_gpu_last_error().decode()
    in_force()
    # null handle
    assert L.ivfhnsw_gpu_set_values(None, 0, None, None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_clear_values(None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_values_info(None, None, None, None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_value_rows(None, 0, 1, C.byref(total)) == pkg.ERR_INVALID
    # views: neither set nor clear; they search with the parent's values
    v = g.view()
    _raises(pkg, pkg.ERR_STATE, lambda: v.set_values(lab2[:10], val2[:10]))
    _raises(pkg, pkg.ERR_STATE, lambda: v.set_values_dev(0, None, None))
    _raises(pkg, pkg.ERR_STATE, lambda: v.clear_values())
    assert _same_search(v.search_values(q, 1, qr, NPROBE, MAX_CODES, efSearch=EF), ref)
    v.close()
    in_force()
    # what the plain call refuses is refused with its status
    _raises(pkg, pkg.ERR_INVALID, lambda: g.search_values(q, 0, qr, NPROBE, MAX_CODES, efSearch=EF))
    _raises(pkg, pkg.ERR_INVALID, lambda: g.search_values(q, 1, qr, 0, MAX_CODES, efSearch=EF))
    _raises(pkg, pkg.ERR_INVALID, lambda: g.range_search_values(q, float("nan"), qr, NPROBE, MAX_CODES, efSearch=EF))
    in_force()
    # a repeated label with the same value counts once; n = 0 changes nothing
    g.set_values(np.array([labels[0], labels[0]], np.uint32), np.array([values[0], values[0]], np.uint32))
    g.set_values(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    g.set_values_dev(0, None, None)
    in_force()


def test_values_and_the_handles_filter_are_not_combined(gpu, pkg):
    b = filter_ref.clipped(corpus(**BASE))
    asg = vr.assignment(b)
    g = vr.install(_upload(gpu(), b), asg)
    q = b["queries"]
    qr = vr.query_ranges(len(q))
    band = vr.PATTERN[3]
    ref = g.search_values(q, 1, qr, NPROBE, MAX_CODES, efSearch=EF)
    g.set_filter(vr.labels_in(asg, band))
    filtered = g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)  # plain calls go on, and never read values
    assert g.last_scan_kernel() == "scan_k1_kernel+filter"
    _raises(pkg, pkg.ERR_STATE, lambda: g.search_values(q, 1, qr, NPROBE, MAX_CODES, efSearch=EF), "set_filter")
    _raises(pkg, pkg.ERR_STATE, lambda: g.range_search_values(q, 1.0, qr, NPROBE, MAX_CODES, efSearch=EF), "set_filter")
    assert _same_search(g.search_values(q, 1, None, NPROBE, MAX_CODES, efSearch=EF), filtered)  # NULL: the plain call
    g.clear_filter()
    assert _same_search(g.search_values(q, 1, qr, NPROBE, MAX_CODES, efSearch=EF), ref)
    m = vr.mine(qr, band)
    assert _same_search((ref[0][m], ref[1][m]), (filtered[0][m], filtered[1][m]))


def test_before_upload_and_on_a_shard(gpu, pkg):
    c = corpus(**BASE)
    labels = c["ids"][:100].copy()
    values = np.full(100, 3, np.uint32)
    full = np.tile(np.array(vr.FULL, np.uint32), (len(c["queries"]), 1))
    h = gpu()
    for call in (lambda: h.set_values(labels, values), lambda: h.set_values_dev(0, None, None)):
        _raises(pkg, pkg.ERR_STATE, call, "upload_ivf")
    h.clear_values()  # nothing to clear
    assert h.values_info() == (0, 0, 0)
    _raises(pkg, pkg.ERR_STATE, lambda: h.search_values(c["queries"], 1, full, 16, 2000, efSearch=40))
    # a shard of two
    world = 2
    off = c["offsets"].astype(np.int64)
    sel = np.concatenate([np.arange(off[cc], off[cc + 1]) for cc in range(0, c["nc"], world)]).astype(np.int64)
    s = gpu()
    s.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"][sel], c["codes"][sel], c["norm_codes"][sel],
                 c["centroid_norms"], c["pq_centroids"], c["norm_table"], shard_rank=0, shard_world=world)
    _raises(pkg, pkg.ERR_STATE, lambda: s.set_values(labels, values), "shard")
    _raises(pkg, pkg.ERR_STATE, lambda: s.clear_values(), "shard")
    assert s.values_info() == (0, len(sel), 0)
    gr = c["graph"]
    s.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    _raises(pkg, pkg.ERR_STATE, lambda: s.search_values(c["queries"], 1, full, 16, 2000, efSearch=40), "shard")
    _raises(pkg, pkg.ERR_STATE, lambda: s.range_search_values(c["queries"], 1.0, full, 16, 2000, efSearch=40), "shard")


def test_memory_bytes_follows_the_formula(gpu):
    """4 * (largest valued label + 1) bytes of table and 4 * max(rows, 1) bytes of row values, measured around the calls
    with no search in between (workspaces grow too)."""
    import torch
    b = filter_ref.clipped(corpus(**BASE))
    n = len(b["ids"])
    g = _upload(gpu(), b)
    mem0 = g.memory_bytes()
    g.set_values(np.array([10, 20], np.uint32), np.array([1, 0x80000000], np.uint32))
    assert g.memory_bytes() - mem0 == 4 * 21 + 4 * n
    g.set_values(np.array([5], np.uint32), np.array([1], np.uint32))  # below the largest label: the table keeps its size
    assert g.memory_bytes() - mem0 == 4 * 21 + 4 * n
    dev = torch.device("cuda", 0)
    d_lab = torch.from_numpy(np.array([99999, 7], np.uint32).view(np.int32)).to(dev)
    d_val = torch.from_numpy(np.array([4, 4], np.uint32).view(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    g.set_values_dev(2, d_lab, d_val)
    assert g.memory_bytes() - mem0 == 4 * 100000 + 4 * n
    assert g.values_info() == (int(np.isin(b["ids"], [5, 7, 10, 20, 99999]).sum()), n, 100000)
    assert g.value_rows(0x80000000, 0x80000000) == int((b["ids"] == 20).sum())
    g.set_values(np.array([99999], np.uint32), np.array([NONE], np.uint32))  # un-valued, and still the table's last entry
    assert g.memory_bytes() - mem0 == 4 * 100000 + 4 * n
    g.clear_values()
    assert g.memory_bytes() == mem0
    # no resident row: one element of row values
    e = _upload(gpu(), b, graph=False)
    assert e.remove_ids(np.unique(b["ids"]))[0] == n
    mem0 = e.memory_bytes()
    e.set_values(np.array([3], np.uint32), np.array([9], np.uint32))
    assert e.memory_bytes() - mem0 == 4 * 4 + 4 and e.values_info() == (0, 0, 4) and e.value_rows(NONE, NONE) == 0
