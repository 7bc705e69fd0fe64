"""Every refusal of the row-tag entry points, with its code; after each, the tags answer as before, shown by a search, and
memory_bytes follows the contract's formula.  (IVFHNSW_ERR_NOMEM needs an allocation to fail, which a test cannot arrange
without exhausting the device; the path is the one set_filter has: the new table and the new row tags are allocated and
filled before the installed ones are touched.)"""
import ctypes as C

import numpy as np
import pytest

from conftest import corpus
import filter_ref
import tags_ref as tr
from test_gpu_remove import BASE, _upload, _same_search

pytestmark = pytest.mark.gpu

NPROBE, MAX_CODES, EF = tr.IVF_PARAMS
NONE = tr.NONE


def _raises(pkg, code, call, word=None):
    with pytest.raises(pkg.IvfHnswError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if word:
        assert word in str(e.value)


def test_refusals_leave_the_tags(gpu, pkg):
    import torch
    b = filter_ref.clipped(corpus(**BASE))
    asg = tr.assignment(b)
    g = tr.install(_upload(gpu(), b), asg)
    q = b["queries"]
    qt = tr.query_tags(len(q))
    info = g.tags_info()
    rows = {t: g.tag_rows(t) for t in set(tr.PATTERN)}
    ref = g.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF)
    mem = g.memory_bytes()

    def in_force():
        assert g.tags_info() == info and {t: g.tag_rows(t) for t in rows} == rows
        assert _same_search(g.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF), ref)
        assert g.last_scan_kernel() == "scan_k1_kernel+tags"
        assert g.memory_bytes() == mem

    L = pkg.lib()
    labels, tags = tr.tagged(asg)
    dev = torch.device("cuda", 0)
    # conflicting repeats: one label, two different tags -- among thousands of valid entries, host and device form
    lab2 = np.concatenate([labels[:4000], labels[17:18]]).astype(np.uint32)
    tag2 = np.concatenate([np.full(4000, 7, np.uint16), np.array([8], np.uint16)])
    _raises(pkg, pkg.ERR_INVALID, lambda: g.set_tags(lab2, tag2), "two different tags")
    in_force()
    d_lab = torch.from_numpy(np.concatenate([lab2, lab2[:1]]).view(np.int32)).to(dev)
    d_tag = torch.from_numpy(np.concatenate([tag2, tag2[:1]]).view(np.int16)).to(dev)
    torch.cuda.synchronize(dev)
    _raises(pkg, pkg.ERR_INVALID, lambda: g.set_tags_dev(len(lab2), d_lab, d_tag), "two different tags")
    in_force()
    # NULL pointers with n > 0
    assert L.ivfhnsw_gpu_set_tags(g._h, 5, None, tag2.ctypes.data) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_set_tags(g._h, 5, lab2.ctypes.data, None) == pkg.ERR_INVALID
    assert "null tags" in L.ivfhnsw_gpu_last_error().decode()
    assert L.ivfhnsw_gpu_set_tags_dev(g._h, 5, None, d_tag.data_ptr()) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_set_tags_dev(g._h, 5, d_lab.data_ptr(), None) == pkg.ERR_INVALID
    in_force()
    # misaligned device pointers (constructed, never dereferenced on the host): labels 4-byte, tags 2-byte
    assert L.ivfhnsw_gpu_set_tags_dev(g._h, 100, d_lab.data_ptr() + 2, d_tag.data_ptr()) == pkg.ERR_INVALID
    assert "aligned" in L.ivfhnsw_gpu_last_error().decode()
    assert L.ivfhnsw_gpu_set_tags_dev(g._h, 100, d_lab.data_ptr(), d_tag.data_ptr() + 1) == pkg.ERR_INVALID
    assert "aligned" in L.ivfhnsw_gpu_last_error().decode()
    d_q = torch.from_numpy(q).to(dev)
    dd = torch.empty((len(q), 1), dtype=torch.float32, device=dev)
    ll = torch.empty((len(q), 1), dtype=torch.int64, device=dev)
    d_qt = torch.from_numpy(np.concatenate([qt, qt[:1]]).view(np.int16)).to(dev)
    torch.cuda.synchronize(dev)
    p = pkg.SearchParams(NPROBE, MAX_CODES, EF, 0, 0)
    assert L.ivfhnsw_gpu_search_tags_dev(g._h, len(q), 1, d_q.data_ptr(), None, None, C.byref(p), d_qt.data_ptr() + 1,
                                         dd.data_ptr(), ll.data_ptr(), None) == pkg.ERR_INVALID
    in_force()
    # tag_rows of something that is no tag; null handle
    _raises(pkg, pkg.ERR_INVALID, lambda: g.tag_rows(0x10000))
    assert L.ivfhnsw_gpu_set_tags(None, 0, None, None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_clear_tags(None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_tags_info(None, None, None, None) == pkg.ERR_INVALID
    # views: neither set nor clear; they search with the parent's tags
    v = g.view()
    _raises(pkg, pkg.ERR_STATE, lambda: v.set_tags(lab2[:10], tag2[:10]))
    _raises(pkg, pkg.ERR_STATE, lambda: v.set_tags_dev(0, None, None))
    _raises(pkg, pkg.ERR_STATE, lambda: v.clear_tags())
    assert _same_search(v.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF), ref)
    v.close()
    in_force()
    # what the plain call refuses is refused with its status
    _raises(pkg, pkg.ERR_INVALID, lambda: g.search_tags(q, 0, qt, NPROBE, MAX_CODES, efSearch=EF))
    _raises(pkg, pkg.ERR_INVALID, lambda: g.search_tags(q, 1, qt, 0, MAX_CODES, efSearch=EF))
    _raises(pkg, pkg.ERR_INVALID, lambda: g.range_search_tags(q, float("nan"), qt, NPROBE, MAX_CODES, efSearch=EF))
    in_force()
    # a repeated label with the same tag counts once; n = 0 changes nothing
    g.set_tags(np.array([labels[0], labels[0]], np.uint32), np.array([tags[0], tags[0]], np.uint16))
    g.set_tags(np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    g.set_tags_dev(0, None, None)
    in_force()


def test_tags_and_the_handles_filter_are_not_combined(gpu, pkg):
    b = filter_ref.clipped(corpus(**BASE))
    asg = tr.assignment(b)
    g = tr.install(_upload(gpu(), b), asg)
    q = b["queries"]
    qt = tr.query_tags(len(q))
    ref = g.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF)
    g.set_filter(tr.labels_of(asg, 0))
    filtered = g.search(q, 1, NPROBE, MAX_CODES, efSearch=EF)  # plain calls go on, and never read tags
    assert g.last_scan_kernel() == "scan_k1_kernel+filter"
    _raises(pkg, pkg.ERR_STATE, lambda: g.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF), "set_filter")
    _raises(pkg, pkg.ERR_STATE, lambda: g.range_search_tags(q, 1.0, qt, NPROBE, MAX_CODES, efSearch=EF), "set_filter")
    assert _same_search(g.search_tags(q, 1, None, NPROBE, MAX_CODES, efSearch=EF), filtered)  # NULL: the plain call
    g.clear_filter()
    assert _same_search(g.search_tags(q, 1, qt, NPROBE, MAX_CODES, efSearch=EF), ref)
    m = qt == 0
    assert _same_search((ref[0][m], ref[1][m]), (filtered[0][m], filtered[1][m]))


def test_before_upload_and_on_a_shard(gpu, pkg):
    c = corpus(**BASE)
    labels = c["ids"][:100].copy()
    tags = np.full(100, 3, np.uint16)
    h = gpu()
    for call in (lambda: h.set_tags(labels, tags), lambda: h.set_tags_dev(0, None, None)):
        _raises(pkg, pkg.ERR_STATE, call, "upload_ivf")
    h.clear_tags()  # nothing to clear
    assert h.tags_info() == (0, 0, 0)
    _raises(pkg, pkg.ERR_STATE, lambda: h.search_tags(c["queries"], 1, tr.query_tags(len(c["queries"])), 16, 2000, efSearch=40))
    # a shard of two
    world = 2
    off = c["offsets"].astype(np.int64)
    sel = np.concatenate([np.arange(off[cc], off[cc + 1]) for cc in range(0, c["nc"], world)]).astype(np.int64)
    s = gpu()
    s.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"][sel], c["codes"][sel], c["norm_codes"][sel],
                 c["centroid_norms"], c["pq_centroids"], c["norm_table"], shard_rank=0, shard_world=world)
    _raises(pkg, pkg.ERR_STATE, lambda: s.set_tags(labels, tags), "shard")
    _raises(pkg, pkg.ERR_STATE, lambda: s.clear_tags(), "shard")
    assert s.tags_info() == (0, len(sel), 0)
    gr = c["graph"]
    s.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    nq = len(c["queries"])
    _raises(pkg, pkg.ERR_STATE, lambda: s.search_tags(c["queries"], 1, np.full(nq, NONE, np.uint16), 16, 2000, efSearch=40),
            "shard")
    _raises(pkg, pkg.ERR_STATE, lambda: s.range_search_tags(c["queries"], 1.0, np.full(nq, NONE, np.uint16), 16, 2000,
                                                            efSearch=40), "shard")


def test_memory_bytes_follows_the_formula(gpu):
    """2 * (largest tagged label + 1) bytes of table and 2 * max(rows, 1) bytes of row tags, measured around the calls with
    no search in between (workspaces grow too)."""
    import torch
    b = filter_ref.clipped(corpus(**BASE))
    n = len(b["ids"])
    g = _upload(gpu(), b)
    mem0 = g.memory_bytes()
    g.set_tags(np.array([10, 20], np.uint32), np.array([1, 2], np.uint16))
    assert g.memory_bytes() - mem0 == 2 * 21 + 2 * n
    g.set_tags(np.array([5], np.uint32), np.array([1], np.uint16))  # below the largest label: the table keeps its size
    assert g.memory_bytes() - mem0 == 2 * 21 + 2 * n
    dev = torch.device("cuda", 0)
    d_lab = torch.from_numpy(np.array([99999, 7], np.uint32).view(np.int32)).to(dev)
    d_tag = torch.from_numpy(np.array([4, 4], np.uint16).view(np.int16)).to(dev)
    torch.cuda.synchronize(dev)
    g.set_tags_dev(2, d_lab, d_tag)
    assert g.memory_bytes() - mem0 == 2 * 100000 + 2 * n
    assert g.tags_info() == (int(np.isin(b["ids"], [5, 7, 10, 20, 99999]).sum()), n, 100000)
    g.set_tags(np.array([99999], np.uint32), np.array([NONE], np.uint16))  # untagged, and still the table's last entry
    assert g.memory_bytes() - mem0 == 2 * 100000 + 2 * n
    g.clear_tags()
    assert g.memory_bytes() == mem0
    # no resident row: one element of row tags
    e = _upload(gpu(), b, graph=False)
    assert e.remove_ids(np.unique(b["ids"]))[0] == n
    mem0 = e.memory_bytes()
    e.set_tags(np.array([3], np.uint32), np.array([9], np.uint16))
    assert e.memory_bytes() - mem0 == 2 * 4 + 2 and e.tags_info() == (0, 0, 4) and e.tag_rows(NONE) == 0
