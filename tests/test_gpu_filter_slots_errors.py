"""Every refusal of the filter-slot entry points, with its code; after each, every slot answers as before, shown by a search.
(IVFHNSW_ERR_NOMEM needs an allocation to fail, which a test cannot arrange without exhausting the device; the path is
the one set_filter has: label bitmap, mask and larger planes are allocated before the installed ones are touched.)"""
import ctypes as C

import numpy as np
import pytest

from conftest import corpus
import filter_ref
import filter_slots_ref as fs
from test_gpu_remove import BASE, _upload, _same_search

pytestmark = pytest.mark.gpu

NPROBE, MAX_CODES, EF = fs.IVF_PARAMS


def _raises(pkg, code, call, word=None):
    with pytest.raises(pkg.IvfHnswError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if word:
        assert word in str(e.value)


def test_refusals_leave_the_slots(gpu, pkg):
    b = filter_ref.clipped(corpus(**BASE))
    sets = fs.slot_sets(b)
    g = fs.install(_upload(gpu(), b), sets)
    q = b["queries"]
    qs = fs.query_slots(len(q))
    info = [g.filter_slot_info(s) for s in range(32)]
    ref = g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF)
    other = fs.slot_sets(b, seed=3)[0][0]

    def in_force():
        assert [g.filter_slot_info(s) for s in range(32)] == info
        assert _same_search(g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF), ref)
        assert g.last_scan_kernel() == "scan_k1_kernel+slots"

    L = pkg.lib()
    # slot out of range
    _raises(pkg, pkg.ERR_INVALID, lambda: g.set_filter_slot(32, other), "slot")
    _raises(pkg, pkg.ERR_INVALID, lambda: g.set_filter_slot_dev(32, 0, None), "slot")
    _raises(pkg, pkg.ERR_INVALID, lambda: g.clear_filter_slot(32))
    _raises(pkg, pkg.ERR_INVALID, lambda: g.clear_filter_slot(-2))
    _raises(pkg, pkg.ERR_INVALID, lambda: g.filter_slot_info(32))
    in_force()
    # null labels with n > 0, host and device form
    assert L.ivfhnsw_gpu_set_filter_slot(g._h, 0, 5, None, pkg.FILTER_ALLOW) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_set_filter_slot_dev(g._h, 0, 5, None, pkg.FILTER_DENY) == pkg.ERR_INVALID
    in_force()
    # an unknown mode
    for mode in (2, -1):
        assert L.ivfhnsw_gpu_set_filter_slot(g._h, 0, other.size, other.ctypes.data, mode) == pkg.ERR_INVALID
        assert "mode" in L.ivfhnsw_gpu_last_error().decode()
    in_force()
    # a misaligned device pointer
    import torch
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(np.concatenate([other, other[:1]]).view(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    assert L.ivfhnsw_gpu_set_filter_slot_dev(g._h, 0, other.size, t.data_ptr() + 2, pkg.FILTER_ALLOW) == pkg.ERR_INVALID
    assert "aligned" in L.ivfhnsw_gpu_last_error().decode()
    in_force()
    # views: neither set nor clear; they search with the parent's slots
    v = g.view()
    _raises(pkg, pkg.ERR_STATE, lambda: v.set_filter_slot(0, other))
    _raises(pkg, pkg.ERR_STATE, lambda: v.set_filter_slot_dev(0, 0, None))
    _raises(pkg, pkg.ERR_STATE, lambda: v.clear_filter_slot(0))
    _raises(pkg, pkg.ERR_STATE, lambda: v.clear_filter_slot())
    assert _same_search(v.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF), ref)
    v.close()
    in_force()
    # null handle
    assert L.ivfhnsw_gpu_set_filter_slot(None, 0, 0, None, 0) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_clear_filter_slot(None, -1) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_filter_slot_info(None, 0, None, None, None) == pkg.ERR_INVALID
    # what the plain call refuses is refused with its status
    _raises(pkg, pkg.ERR_INVALID, lambda: g.search_slots(q, 0, qs, NPROBE, MAX_CODES, efSearch=EF))
    _raises(pkg, pkg.ERR_INVALID, lambda: g.search_slots(q, 1, qs, 0, MAX_CODES, efSearch=EF))
    _raises(pkg, pkg.ERR_INVALID, lambda: g.range_search_slots(q, float("nan"), qs, NPROBE, MAX_CODES, efSearch=EF))
    in_force()


def test_slot_bytes_of_the_host_forms(gpu, pkg):
    """A byte in 32..254 is refused before anything is launched or written; NULL bytes are the plain call."""
    b = filter_ref.clipped(corpus(**BASE))
    g = fs.install(_upload(gpu(), b), fs.slot_sets(b))
    L = pkg.lib()
    for nq in (64, 1024):  # the pinned and the staged host path
        q = fs.tiled(b["queries"], nq)
        qs = fs.query_slots(nq)
        good = g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF)
        kernel = g.last_scan_kernel()
        bad = qs.copy()
        bad[nq - 3] = 200
        dist = np.full((nq, 1), 7.0, np.float32)
        lab = np.full((nq, 1), 7, np.int64)
        p = pkg.SearchParams(NPROBE, MAX_CODES, EF, 0, 0)
        rc = L.ivfhnsw_gpu_search_slots(g._h, nq, 1, q.ctypes.data, None, None, C.byref(p), bad.ctypes.data,
                                        dist.ctypes.data, lab.ctypes.data)
        assert rc == pkg.ERR_INVALID and "slot 200" in L.ivfhnsw_gpu_last_error().decode()
        assert (dist == 7.0).all() and (lab == 7).all()
        for byte in (32, 254):
            bad[0] = byte
            _raises(pkg, pkg.ERR_INVALID, lambda: g.search_slots(q, 1, bad, NPROBE, MAX_CODES, efSearch=EF))
        lims = np.full(nq + 1, 7, np.uint64)
        total = C.c_uint64(7)
        rc = L.ivfhnsw_gpu_range_search_slots(g._h, nq, q.ctypes.data, None, None, C.byref(p), bad.ctypes.data,
                                              C.c_float(1.0), lims.ctypes.data, C.byref(total))
        assert rc == pkg.ERR_INVALID and (lims == 7).all() and total.value == 7
        assert _same_search(g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF), good)
        assert g.last_scan_kernel() == kernel
        # NULL: the plain call, name included
        plain = g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)
        name = g.last_scan_kernel()
        assert not name.endswith("+slots")
        assert _same_search(g.search_slots(q, 1, None, NPROBE, MAX_CODES, efSearch=EF), plain)
        assert g.last_scan_kernel() == name
        none = g.search_slots(q, 1, np.full(nq, fs.NONE, np.uint8), NPROBE, MAX_CODES, efSearch=EF)
        assert _same_search(none, plain) and g.last_scan_kernel().endswith("+slots")
    r0 = g.range_search(q[:64], 1e9, NPROBE, 200, efSearch=EF)
    r1 = g.range_search_slots(q[:64], 1e9, None, NPROBE, 200, efSearch=EF)
    assert not g.last_scan_kernel().endswith("+slots")
    assert all(np.array_equal(x, y) for x, y in zip(r0, r1))


def test_slot_bytes_of_the_dev_form(gpu):
    """The _dev form reads nothing back: a byte that names no installed slot -- beyond the planes held, or 32..254 -- passes
    nothing."""
    from test_gpu_filter_slots import _dev_search
    b = filter_ref.clipped(corpus(**BASE))
    sets = {s: v for s, v in fs.slot_sets(b).items() if s != 31}  # planes 0..7
    g = fs.install(_upload(gpu(), b), sets)
    q = b["queries"]
    qs = fs.query_slots(len(q))
    want = g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF)
    assert (want[1][qs == 31] == -1).all()  # slot 31 is in range for the host form, and not set
    odd = qs.copy()
    odd[qs == 31] = np.resize(np.array([8, 31, 32, 100, 254], np.uint8), int((qs == 31).sum()))
    r = _dev_search(g, q, 1, odd, NPROBE, MAX_CODES, EF)
    assert _same_search((r["dist"], r["labels"]), want)
    r = _dev_search(g, q, 10, odd, NPROBE, MAX_CODES, EF, heap=True)
    assert (r["labels"][qs == 31] == -1).all() and (r["labels"][qs == 0] >= 0).any()


def test_slots_and_the_handles_filter_are_not_combined(gpu, pkg):
    b = filter_ref.clipped(corpus(**BASE))
    sets = fs.slot_sets(b)
    g = fs.install(_upload(gpu(), b), sets)
    q = b["queries"]
    qs = fs.query_slots(len(q))
    ref = g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF)
    g.set_filter(sets[0][0])
    filtered = g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)  # plain calls go on, and never read slots
    assert g.last_scan_kernel() == "scan_k1_kernel+filter"
    _raises(pkg, pkg.ERR_STATE, lambda: g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF), "set_filter")
    _raises(pkg, pkg.ERR_STATE, lambda: g.range_search_slots(q, 1.0, qs, NPROBE, MAX_CODES, efSearch=EF), "set_filter")
    assert _same_search(g.search_slots(q, 1, None, NPROBE, MAX_CODES, efSearch=EF), filtered)  # NULL: the plain call
    g.clear_filter()
    assert _same_search(g.search_slots(q, 1, qs, NPROBE, MAX_CODES, efSearch=EF), ref)
    m = qs == 0
    assert _same_search((ref[0][m], ref[1][m]), (filtered[0][m], filtered[1][m]))


def test_before_upload_and_on_a_shard(gpu, pkg):
    c = corpus(**BASE)
    labels = c["ids"][:100].copy()
    h = gpu()
    for call in (lambda: h.set_filter_slot(0, labels), lambda: h.set_filter_slot_dev(0, 0, None),
                 lambda: h.clear_filter_slot(0), lambda: h.clear_filter_slot()):
        _raises(pkg, pkg.ERR_STATE, call, "upload_ivf")
    assert h.filter_slot_info(0) == (-1, 0, 0)
    _raises(pkg, pkg.ERR_STATE, lambda: h.search_slots(c["queries"], 1, fs.query_slots(len(c["queries"])), 16, 2000,
                                                       efSearch=40))
    # a shard of three
    world = 3
    off = c["offsets"].astype(np.int64)
    sel = np.concatenate([np.arange(off[cc], off[cc + 1]) for cc in range(0, c["nc"], world)]).astype(np.int64)
    s = gpu()
    s.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"][sel], c["codes"][sel], c["norm_codes"][sel],
                 c["centroid_norms"], c["pq_centroids"], c["norm_table"], shard_rank=0, shard_world=world)
    for deny in (False, True):
        _raises(pkg, pkg.ERR_STATE, lambda: s.set_filter_slot(0, labels, deny=deny), "shard")
    _raises(pkg, pkg.ERR_STATE, lambda: s.clear_filter_slot(), "shard")
    assert s.filter_slot_info(0) == (-1, 0, len(sel))
    gr = c["graph"]
    s.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    nq = len(c["queries"])
    _raises(pkg, pkg.ERR_STATE, lambda: s.search_slots(c["queries"], 1, np.full(nq, fs.NONE, np.uint8), 16, 2000,
                                                       efSearch=40), "shard")
