"""What an upsert refuses (ivfhnsw_gpu_upsert_ivf / _dev): after every failing call the handle's lists are
byte for byte what they were and a search returns the same bits -- the call is atomic, unlike remove_ids followed by
append_ivf."""
import numpy as np
import pytest

from conftest import corpus
from test_gpu_remove import BASE, GROUPING, _same_search, _upload
from test_gpu_upsert import _batch, _dev

pytestmark = pytest.mark.gpu


def _raises(pkg, code, fn, *a, **kw):
    with pytest.raises(pkg.IvfHnswError) as e:
        fn(*a, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_invalid_calls_leave_the_tables(gpu, pkg):
    import torch
    c = corpus(**BASE)
    dev = torch.device("cuda", 0)
    g = _upload(gpu(), c)
    before = g.download_ivf()
    ref = g.search(c["queries"], 1, 16, 2000, efSearch=40)
    allow = np.unique(c["ids"])[::2]
    g.set_filter(allow)
    info = g.filter_info()
    fref = g.search(c["queries"], 1, 16, 2000, efSearch=40)
    g.clear_filter()

    def unchanged():
        for x, y in zip(g.download_ivf(), before):
            assert np.array_equal(x, y)
        assert _same_search(g.search(c["queries"], 1, 16, 2000, efSearch=40), ref)

    li, lab, codes, ncodes = _batch(c, "mixed", seed=1)
    n = len(lab)
    # the same label twice: host form and _dev form, found on the device
    twice = lab.copy()
    twice[n - 1] = twice[3]
    assert "twice" in _raises(pkg, pkg.ERR_INVALID, g.upsert_ivf, li, twice, codes, ncodes)
    unchanged()
    d = [_dev(x) for x in (li, twice, codes, ncodes)]
    torch.cuda.synchronize(dev)
    assert "twice" in _raises(pkg, pkg.ERR_INVALID, g.upsert_ivf_dev, n, *d)
    unchanged()
    # ... with a filter installed: filter and filtered answers stay too
    g.set_filter(allow)
    _raises(pkg, pkg.ERR_INVALID, g.upsert_ivf, li, twice, codes, ncodes)
    assert g.filter_info() == info and _same_search(g.search(c["queries"], 1, 16, 2000, efSearch=40), fref)
    g.clear_filter()
    unchanged()
    # a list id >= nc: the host form checks on the host, the _dev form on the device
    bad = li.copy()
    bad[n // 2] = c["nc"]
    _raises(pkg, pkg.ERR_INVALID, g.upsert_ivf, bad, lab, codes, ncodes)
    unchanged()
    d = [_dev(x) for x in (bad, lab, codes, ncodes)]
    torch.cuda.synchronize(dev)
    _raises(pkg, pkg.ERR_INVALID, g.upsert_ivf_dev, n, *d)
    unchanged()
    # null buffers
    assert pkg.lib().ivfhnsw_gpu_upsert_ivf(g._h, 5, None, None, None, None, None, None) == pkg.ERR_INVALID
    d = [_dev(x) for x in (li, lab, codes, ncodes)]
    torch.cuda.synchronize(dev)
    _raises(pkg, pkg.ERR_INVALID, g.upsert_ivf_dev, n, d[0], None, d[2], d[3])
    unchanged()
    # a misaligned device pointer
    _raises(pkg, pkg.ERR_INVALID, g.upsert_ivf_dev, n - 1, d[0], d[1].data_ptr() + 1, d[2], d[3])
    _raises(pkg, pkg.ERR_INVALID, g.upsert_ivf_dev, n - 1, d[0].data_ptr() + 2, d[1], d[2], d[3])
    unchanged()
    # n = 0 succeeds and changes nothing
    nr, per = g.upsert_ivf(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, c["code_size"]), np.uint8), np.zeros(0, np.uint8))
    assert nr == 0 and not per.any()
    assert pkg.lib().ivfhnsw_gpu_upsert_ivf(g._h, 0, None, None, None, None, None, None) == pkg.OK
    unchanged()
    # and the good batch goes through afterwards
    assert g.upsert_ivf(li, lab, codes, ncodes)[0] == 1500


def test_state_errors(gpu, pkg):
    c = corpus(**BASE)
    batch = _batch(c, "mixed", seed=2)
    # before upload_ivf
    _raises(pkg, pkg.ERR_STATE, gpu().upsert_ivf, *batch)
    # a view
    g = _upload(gpu(), c)
    before = g.download_ivf()
    ref = g.search(c["queries"], 1, 16, 2000, efSearch=40)
    v = g.view()
    _raises(pkg, pkg.ERR_STATE, v.upsert_ivf, *batch)
    v.close()
    for x, y in zip(g.download_ivf(), before):
        assert np.array_equal(x, y)
    assert _same_search(g.search(c["queries"], 1, 16, 2000, efSearch=40), ref)
    # a shard of three
    world = 3
    off = c["offsets"].astype(np.int64)
    sel = np.concatenate([np.arange(off[cc], off[cc + 1]) for cc in range(0, c["nc"], world)]).astype(np.int64)
    s = gpu()
    s.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"][sel], c["codes"][sel], c["norm_codes"][sel],
                 c["centroid_norms"], c["pq_centroids"], c["norm_table"], shard_rank=0, shard_world=world)
    s_before = s.download_ivf()
    assert "shard" in _raises(pkg, pkg.ERR_STATE, s.upsert_ivf, *batch)
    for x, y in zip(s.download_ivf(), s_before):
        assert np.array_equal(x, y)
    # a Grouping handle
    gc = corpus(**GROUPING[1])
    h = _upload(gpu(), gc)
    h_before = h.download_ivf()
    href = h.search(gc["queries"], 1, 16, 600, efSearch=64)
    gb = _batch(gc, "mixed", seed=3)
    assert "grouping" in _raises(pkg, pkg.ERR_STATE, h.upsert_ivf, *gb)
    for x, y in zip(h.download_ivf(), h_before):
        assert np.array_equal(x, y)
    assert np.array_equal(h.download_grouping(), gc["subgroup_sizes"])
    assert _same_search(h.search(gc["queries"], 1, 16, 600, efSearch=64), href)


def test_resolve_keys_after_an_upsert_is_refused(gpu, pkg):
    import torch
    c = corpus(**BASE)
    dev = torch.device("cuda", 0)
    g = _upload(gpu(), c)
    q = c["queries"]
    nq = len(q)
    d_q = _dev(q)
    d = torch.empty((nq, 1), dtype=torch.float32, device=dev)
    lab = torch.empty((nq, 1), dtype=torch.int64, device=dev)
    keys = torch.empty((nq, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    g.search_dev(nq, 1, d_q, d, lab, 16, 2000, efSearch=40, d_out_keys=keys)
    g.sync()
    d2, l2 = torch.empty_like(d), torch.empty_like(lab)
    torch.cuda.synchronize(dev)
    g.resolve_keys_dev(nq, 1, keys, d2, l2)      # the plan of the search stands
    g.sync()
    assert torch.equal(l2, lab)
    g.upsert_ivf(*_batch(c, "mixed", seed=4))
    _raises(pkg, pkg.ERR_STATE, g.resolve_keys_dev, nq, 1, keys, d2, l2)   # ... and ended with the rows it described
