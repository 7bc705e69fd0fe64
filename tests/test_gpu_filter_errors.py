"""Every refusal of the label filter's entry points, with its code; after each the earlier filter is still in force, shown by
a search.  (IVFHNSW_ERR_NOMEM needs an allocation to fail, which a test cannot arrange without exhausting the device; the
path is the one every update shares: the new mask and bitmap are allocated before the installed ones are touched.)"""
import numpy as np
import pytest

from conftest import corpus
import filter_ref
from test_gpu_remove import BASE, _upload, _same_search

pytestmark = pytest.mark.gpu

NPROBE, MAX_CODES, EF = 16, 2000, 40


def test_refusals_leave_the_filter(gpu, pkg):
    b = filter_ref.clipped(corpus(**BASE))
    labels = np.random.default_rng(1).choice(b["ids"], 3000, replace=False).astype(np.uint32)
    other = np.random.default_rng(2).choice(b["ids"], 3000, replace=False).astype(np.uint32)
    g = _upload(gpu(), b)
    g.set_filter(labels)
    info = g.filter_info()
    ref = g.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF)
    assert np.isin(ref[1][ref[1] >= 0], labels).all()

    def in_force():
        assert g.filter_info() == info
        assert _same_search(g.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF), ref)
        assert g.last_scan_kernel() == "scan_k1_kernel+filter"

    L = pkg.lib()
    # null labels with n > 0, host and device form
    assert L.ivfhnsw_gpu_set_filter(g._h, 5, None, pkg.FILTER_ALLOW) == pkg.ERR_INVALID
    in_force()
    assert L.ivfhnsw_gpu_set_filter_dev(g._h, 5, None, pkg.FILTER_DENY) == pkg.ERR_INVALID
    in_force()
    # an unknown mode
    for mode in (2, -1):
        assert L.ivfhnsw_gpu_set_filter(g._h, other.size, other.ctypes.data, mode) == pkg.ERR_INVALID
        assert "mode" in L.ivfhnsw_gpu_last_error().decode()
        in_force()
    # views: neither set nor clear
    v = g.view()
    with pytest.raises(pkg.IvfHnswError) as e:
        v.set_filter(other)
    assert e.value.code == pkg.ERR_STATE
    with pytest.raises(pkg.IvfHnswError) as e:
        v.set_filter_dev(0, None)
    assert e.value.code == pkg.ERR_STATE
    with pytest.raises(pkg.IvfHnswError) as e:
        v.clear_filter()
    assert e.value.code == pkg.ERR_STATE
    assert _same_search(v.search(b["queries"], 1, NPROBE, MAX_CODES, efSearch=EF), ref)
    v.close()
    in_force()
    # null handle
    assert L.ivfhnsw_gpu_set_filter(None, 0, None, 0) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_clear_filter(None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_filter_info(None, None, None, None) == pkg.ERR_INVALID
    in_force()


def test_before_upload_and_on_a_shard(gpu, pkg):
    c = corpus(**BASE)
    labels = c["ids"][:100].copy()
    h = gpu()
    for call in (lambda: h.set_filter(labels), lambda: h.set_filter_dev(0, None)):
        with pytest.raises(pkg.IvfHnswError) as e:
            call()
        assert e.value.code == pkg.ERR_STATE and "upload_ivf" in str(e.value)
    h.clear_filter()  # nothing to clear: succeeds
    assert h.filter_info() == (-1, 0, 0)
    # a shard of three
    world = 3
    off = c["offsets"].astype(np.int64)
    sel = np.concatenate([np.arange(off[cc], off[cc + 1]) for cc in range(0, c["nc"], world)]).astype(np.int64)
    s = gpu()
    s.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"][sel], c["codes"][sel], c["norm_codes"][sel],
                 c["centroid_norms"], c["pq_centroids"], c["norm_table"], shard_rank=0, shard_world=world)
    for deny in (False, True):
        with pytest.raises(pkg.IvfHnswError) as e:
            s.set_filter(labels, deny=deny)
        assert e.value.code == pkg.ERR_STATE and "shard" in str(e.value)
    assert s.filter_info() == (-1, len(sel), len(sel))
