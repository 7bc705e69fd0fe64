"""Base values: their state on the handle and the documented errors -- the statuses of every refused call;
a refused set leaving the earlier values in force; upload_base dropping and keeping them; views; independence from the base
filter, the base filter slots, the base tags and the index's row values; query_ranges NULL taking the plain path; what
memory_bytes counts.  Exact throughout."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_filter_ref as fr
import exact_tags_ref as tr
import exact_values_ref as vr

pytestmark = pytest.mark.gpu

F = np.float32
N, D, NQ, K = 6001, 48, 40, 10


@pytest.fixture(scope="module")
def data():
    base = vr.make_base(N, D)
    q = vr.make_queries(NQ, D, base)
    import exact_ref
    dist = exact_ref.distances(base, q)
    ivs = np.array([(1, 0xfffffffd), vr.FULL, (vr.RUN0 + 1, vr.RUN0 + 3), vr.ABSENT, (vr.BAND31, vr.BAND31 + 511), vr.INVERTED], np.uint32)
    return base, q, F(np.sort(dist, axis=None)[dist.size // 4]), vr.base_values(N), ivs[np.arange(NQ) % len(ivs)]


def _same(got, want):
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def _same_range(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _status(pkg, call):
    with pytest.raises(pkg.IvfHnswError) as e:
        call()
    return e.value.code


ROWS = np.arange(N, dtype=np.uint32)
NOVALS = np.full(N, vr.NONE, np.uint32)


def _empty(qr):
    return np.array([not vr.value_mask(NOVALS, lo, hi).any() for lo, hi in qr])


def test_refused_calls_and_a_refused_set_leaves_the_values_in_force(gpu, pkg, data):
    base, q, radius, bvals, qr = data
    L = pkg.lib()
    g = gpu()
    # before upload_base
    assert _status(pkg, lambda: g.exact_search_values(q, K, qr)) == pkg.ERR_STATE
    assert _status(pkg, lambda: g.exact_range_search_values(q, radius, qr)) == pkg.ERR_STATE
    assert _status(pkg, lambda: g.set_base_values(ROWS, bvals)) == pkg.ERR_STATE
    assert _status(pkg, lambda: g.base_value_rows(0, 3)) == pkg.ERR_STATE
    g.clear_base_values()  # succeeds when there are none
    assert g.base_values_info() == (0, 0)
    g.upload_base(base)
    assert g.base_values_info() == (0, N) and g.base_value_rows(vr.NONE, vr.NONE) == N and g.base_value_rows(0, 0xfffffffe) == 0
    assert g.base_value_rows(0, vr.NONE) == N and g.base_value_rows(vr.NONE, 0) == 0
    # a _values call without a value array is legal: every row is NONE
    got = g.exact_search_values(q, K, qr)
    _same(got, vr.search_blocked(base, q, K, NOVALS, qr))
    assert (got[1][_empty(qr)] == -1).all() and _empty(qr).sum() >= NQ // 2
    _same_range(g.exact_range_search_values(q, radius, qr), vr.range_blocked(base, q, radius, NOVALS, qr))
    g.set_base_values(ROWS, bvals)
    info = g.base_values_info()
    want = vr.search_blocked(base, q, K, bvals, qr)
    want_r = vr.range_blocked(base, q, radius, bvals, qr)
    held = g.exact_range_search_values(q, radius, qr)
    _same_range(held, want_r)
    # NULL arrays with n > 0, misaligned device pointers, a row given two different values, a NULL result
    r2, v2 = np.array([5, 9, 5], np.uint32), np.array([1, 2, 3], np.uint32)
    assert L.ivfhnsw_gpu_set_base_values(g._h, 3, None, v2.ctypes.data) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_set_base_values(g._h, 3, r2.ctypes.data, None) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.set_base_values(r2, v2)) == pkg.ERR_INVALID  # row 5: values 1 and 3
    assert L.ivfhnsw_gpu_base_value_rows(g._h, 0, 1, None) == pkg.ERR_INVALID
    dev = torch.device("cuda:0")
    d_rows = torch.arange(16, dtype=torch.int32, device=dev)
    d_vals = torch.zeros(16, dtype=torch.int32, device=dev)
    assert L.ivfhnsw_gpu_set_base_values_dev(g._h, 8, d_rows.data_ptr() + 2, d_vals.data_ptr()) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_set_base_values_dev(g._h, 8, d_rows.data_ptr(), d_vals.data_ptr() + 1) == pkg.ERR_INVALID
    dq = torch.from_numpy(q).to(dev)
    od, ol = torch.empty((NQ, K), dtype=torch.float32, device=dev), torch.empty((NQ, K), dtype=torch.int64, device=dev)
    dr = torch.zeros(2 * NQ + 2, dtype=torch.int32, device=dev)
    dl = torch.zeros(NQ + 1, dtype=torch.int64, device=dev)
    tot = C.c_uint64(0)
    assert dr.data_ptr() % 8 == 0
    assert L.ivfhnsw_gpu_exact_search_values_dev(g._h, NQ, dq.data_ptr(), D, K, dr.data_ptr() + 4, od.data_ptr(),
                                                 ol.data_ptr()) == pkg.ERR_INVALID  # 4-byte aligned is not enough
    assert L.ivfhnsw_gpu_exact_range_search_values_dev(g._h, NQ, dq.data_ptr(), D, dr.data_ptr() + 4, float(radius), dl.data_ptr(),
                                                       C.byref(tot)) == pkg.ERR_INVALID
    # the plain calls' own refusals come with their status
    assert _status(pkg, lambda: g.exact_search_values(q, 101, qr)) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.exact_search_values(q, 0, qr)) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.exact_range_search_values(q, float("nan"), qr)) == pkg.ERR_INVALID
    # ... and every refusal left values and held results as they were
    assert g.base_values_info() == info and g.base_value_rows(1, 3) == 0 and g.base_value_rows(0, 0) == int((bvals == 0).sum())
    d, l = g.exact_range_results(0, int(held[0][-1]))
    assert np.array_equal(l, held[2]) and np.array_equal(d.view(np.uint32), held[1].view(np.uint32))
    _same(g.exact_search_values(q, K, qr), want)
    # a repeat with the same value counts once
    g.set_base_values(np.array([5, 5], np.uint32), np.array([3, 3], np.uint32))
    assert g.base_value_rows(3, 3) == 1
    # n == 0 changes nothing
    g.set_base_values(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert g.base_value_rows(3, 3) == 1
    g.clear_base_values()
    assert g.base_values_info() == (0, N)
    g.close()


def test_a_base_filter_is_not_combined_and_neither_reads_the_other(gpu, pkg, data):
    base, q, radius, bvals, qr = data
    g, f = gpu(), gpu()
    g.upload_base(base)
    f.upload_base(base)
    g.set_base_values(ROWS, bvals)
    # plain, _slots and _tags calls never read values
    _same(g.exact_search(q, K), f.exact_search(q, K))
    _same_range(g.exact_range_search(q, radius), f.exact_range_search(q, radius))
    lab, deny = fr.pattern("rand03", N)
    qs = np.array([1, 0xff], np.uint8)[np.arange(NQ) % 2]
    btags = tr.base_tags(N)
    qtags = np.array([tr.BIG, tr.NONE, tr.SOME], np.uint16)[np.arange(NQ) % 3]
    for h in (g, f):
        h.set_base_filter_slot(1, lab, deny=deny)
        h.set_base_tags(ROWS, btags)
    _same(g.exact_search_slots(q, K, qs), f.exact_search_slots(q, K, qs))
    _same(g.exact_search_tags(q, K, qtags), f.exact_search_tags(q, K, qtags))
    # a _values call ignores the slots and the tags
    want = vr.search_blocked(base, q, K, bvals, qr)
    _same(g.exact_search_values(q, K, qr), want)
    assert g.base_tags_info() == f.base_tags_info()
    # a base filter installed: ERR_STATE, and the plain call under it is the parent's
    lab, deny = fr.pattern("gap", N)
    for h in (g, f):
        h.set_base_filter(lab, deny=deny)
    assert _status(pkg, lambda: g.exact_search_values(q, K, qr)) == pkg.ERR_STATE
    assert _status(pkg, lambda: g.exact_range_search_values(q, radius, qr)) == pkg.ERR_STATE
    _same(g.exact_search(q, K), f.exact_search(q, K))
    _same(g.exact_search_values(q, K, None), f.exact_search(q, K))  # NULL is the plain call, base filter and all
    g.clear_base_filter()
    _same(g.exact_search_values(q, K, qr), want)
    _same_range(g.exact_range_search_values(q, radius, qr), vr.range_blocked(base, q, radius, bvals, qr))
    assert g.base_values_info()[0] == int((bvals != vr.NONE).sum())  # set / clear_base_filter did not touch the values
    g.close()
    f.close()


def test_index_values_and_base_values_never_read_each_other(gpu, data):
    from test_gpu_filter_slots import base as corpus
    from test_gpu_remove import BASE, _upload
    base, q, radius, bvals, qr = data
    c = corpus(**BASE)  # the corpus the row-value tests share
    g = _upload(gpu(), c)
    g.upload_base(base)
    ids = np.unique(c["ids"]).astype(np.uint32)
    g.set_values(ids, (ids % 7).astype(np.uint32))
    assert g.base_values_info() == (0, N)
    index_info = g.values_info()
    assert index_info[0] > 0
    three = g.value_rows(3, 3)
    g.set_base_values(ROWS, bvals)
    assert g.values_info() == index_info and g.value_rows(3, 3) == three and g.base_value_rows(3, 3) == 0 != three
    _same(g.exact_search_values(q, K, qr), vr.search_blocked(base, q, K, bvals, qr))
    g.clear_values()
    assert g.base_values_info()[0] == int((bvals != vr.NONE).sum())
    g.clear_base_values()
    g.close()


def test_upload_base_drops_the_values_and_a_later_chunk_keeps_them(gpu, data):
    base, q, _, bvals, qr = data
    g = gpu()
    g.upload_base(base[:4000], n=N)
    g.set_base_values(ROWS, bvals)
    info = g.base_values_info()
    g.upload_base(base[4000:], n=N, first=4000)  # a later chunk keeps them
    assert g.base_values_info() == info
    _same(g.exact_search_values(q, K, qr), vr.search_blocked(base, q, K, bvals, qr))
    g.upload_base(base)  # first == 0: a new store
    assert g.base_values_info() == (0, N)
    got = g.exact_search_values(q, K, qr)
    assert (got[1][_empty(qr)] == -1).all()
    _same(g.exact_search_values(q, K, np.tile(np.array(vr.FULL, np.uint32), (NQ, 1))), g.exact_search(q, K))
    g.set_base_values(ROWS, bvals)
    g.upload_base(np.zeros((0, D), np.uint8), n=0)  # n == 0: no store, no values
    assert g.base_values_info() == (0, 0)
    g.close()


def test_views(gpu, pkg, data):
    base, q, radius, bvals, qr = data
    g = gpu()
    g.upload_base(base)
    v = g.view()
    assert _status(pkg, lambda: v.set_base_values(ROWS, bvals)) == pkg.ERR_STATE
    assert _status(pkg, lambda: v.clear_base_values()) == pkg.ERR_STATE
    g.set_base_values(ROWS, bvals)  # after the view was made: a view reads its parent's values at the call
    assert v.base_values_info() == g.base_values_info() and v.base_value_rows(76, 78) == g.base_value_rows(76, 78) > 0
    _same(v.exact_search_values(q, K, qr), vr.search_blocked(base, q, K, bvals, qr))
    _same_range(v.exact_range_search_values(q, radius, qr), vr.range_blocked(base, q, radius, bvals, qr))
    g.clear_base_values()
    assert v.base_values_info() == (0, N)
    v.close()
    g.close()


def test_null_query_ranges_take_the_plain_path(gpu, data):
    base, q, radius, bvals, qr = data
    g, f = gpu(), gpu()
    g.upload_base(base)
    f.upload_base(base)
    _same(g.exact_search_values(q, K, None), f.exact_search(q, K))
    _same_range(g.exact_range_search_values(q, radius, None), f.exact_range_search(q, radius))
    assert g.memory_bytes() == f.memory_bytes()  # no plan, no plan workspace: the plain call's buffers and nothing else
    g.exact_search_values(q, K, qr)
    assert g.memory_bytes() > f.memory_bytes()
    g.close()
    f.close()


def test_memory_bytes_counts_the_values(gpu, data):
    base, q, radius, bvals, qr = data
    g = gpu()
    g.upload_base(base)
    m0 = g.memory_bytes()
    g.set_base_values(ROWS, bvals)
    assert g.memory_bytes() - m0 == 8 * N  # the values and the row order; the sort's other permutation is gone again
    g.set_base_values(np.arange(100, dtype=np.uint32), np.full(100, vr.NONE, np.uint32))
    assert g.memory_bytes() - m0 == 8 * N
    # the reorder of a range call leaves nothing behind but the results it replaced
    g.exact_range_search_values(q, radius, qr)
    m1 = g.memory_bytes()
    g.exact_range_search_values(q, radius, qr)
    assert g.memory_bytes() == m1
    g.clear_base_values()
    assert g.memory_bytes() == m1 - 8 * N
    g.close()
