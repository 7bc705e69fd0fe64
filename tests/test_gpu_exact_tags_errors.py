"""Base tags: their state on the handle and the documented errors -- the statuses of every refused call; a
refused set leaving the earlier tags in force; upload_base dropping and keeping them; views; independence from the base
filter, the base filter slots and the index's row tags; query_tags NULL taking the plain path; what memory_bytes counts.
Exact throughout."""
import numpy as np
import pytest
import torch

import exact_filter_ref as fr
import exact_tags_ref as tr

pytestmark = pytest.mark.gpu

F = np.float32
N, D, NQ, K = 6001, 48, 40, 10


@pytest.fixture(scope="module")
def data():
    base = tr.make_base(N, D)
    q = tr.make_queries(NQ, D, base)
    import exact_ref
    dist = exact_ref.distances(base, q)
    qtags = np.array([tr.BIG, tr.NONE, tr.SOME, tr.ABSENT[0], tr.MANY0 + 5], np.uint16)[np.arange(NQ) % 5]
    return base, q, F(np.sort(dist, axis=None)[dist.size // 4]), tr.base_tags(N), qtags


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


def test_refused_calls_and_a_refused_set_leaves_the_tags_in_force(gpu, pkg, data):
    base, q, radius, btags, qtags = data
    L = pkg.lib()
    g = gpu()
    # before upload_base
    assert _status(pkg, lambda: g.exact_search_tags(q, K, qtags)) == pkg.ERR_STATE
    assert _status(pkg, lambda: g.exact_range_search_tags(q, radius, qtags)) == pkg.ERR_STATE
    assert _status(pkg, lambda: g.set_base_tags(ROWS, btags)) == pkg.ERR_STATE
    assert _status(pkg, lambda: g.base_tag_rows(3)) == pkg.ERR_STATE
    g.clear_base_tags()  # succeeds when there are none
    assert g.base_tags_info() == (0, 0, 0)
    g.upload_base(base)
    assert g.base_tags_info() == (0, N, 0) and g.base_tag_rows(tr.NONE) == N and g.base_tag_rows(3) == 0
    # a _tags call without a tag array is legal: every row is NONE
    got = g.exact_search_tags(q, K, qtags)
    _same(got, tr.search_blocked(base, q, K, np.full(N, tr.NONE, np.uint16), qtags))
    assert (got[1][qtags != tr.NONE] == -1).all()
    g.set_base_tags(ROWS, btags)
    info = g.base_tags_info()
    want = tr.search_blocked(base, q, K, btags, qtags)
    want_r = tr.range_blocked(base, q, radius, btags, qtags)
    held = g.exact_range_search_tags(q, radius, qtags)
    _same_range(held, want_r)
    # NULL arrays with n > 0, misaligned device pointers, a row given two different tags, a tag beyond 16 bits
    r2, t2 = np.array([5, 9, 5], np.uint32), np.array([1, 2, 3], np.uint16)
    assert L.ivfhnsw_gpu_set_base_tags(g._h, 3, None, t2.ctypes.data) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_set_base_tags(g._h, 3, r2.ctypes.data, None) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.set_base_tags(r2, t2)) == pkg.ERR_INVALID  # row 5: tags 1 and 3
    dev = torch.device("cuda:0")
    d_rows = torch.arange(16, dtype=torch.int32, device=dev)
    d_tags = torch.zeros(16, dtype=torch.int16, device=dev)
    assert L.ivfhnsw_gpu_set_base_tags_dev(g._h, 8, d_rows.data_ptr() + 2, d_tags.data_ptr()) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_set_base_tags_dev(g._h, 8, d_rows.data_ptr(), d_tags.data_ptr() + 1) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.base_tag_rows(0x10000)) == pkg.ERR_INVALID
    dq = torch.from_numpy(q).to(dev)
    od, ol = torch.empty((NQ, K), dtype=torch.float32, device=dev), torch.empty((NQ, K), dtype=torch.int64, device=dev)
    dt = torch.zeros(NQ + 1, dtype=torch.int16, device=dev)
    assert L.ivfhnsw_gpu_exact_search_tags_dev(g._h, NQ, dq.data_ptr(), D, K, dt.data_ptr() + 1, od.data_ptr(),
                                               ol.data_ptr()) == pkg.ERR_INVALID
    # the plain calls' own refusals come with their status
    assert _status(pkg, lambda: g.exact_search_tags(q, 101, qtags)) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.exact_search_tags(q, 0, qtags)) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.exact_range_search_tags(q, float("nan"), qtags)) == pkg.ERR_INVALID
    # ... and every refusal left tags and held results as they were
    assert g.base_tags_info() == info and g.base_tag_rows(1) == 0 and g.base_tag_rows(tr.BIG) == int((btags == tr.BIG).sum())
    d, l = g.exact_range_results(0, int(held[0][-1]))
    assert np.array_equal(l, held[2]) and np.array_equal(d.view(np.uint32), held[1].view(np.uint32))
    _same(g.exact_search_tags(q, K, qtags), want)
    # a repeat with the same tag counts once
    g.set_base_tags(np.array([5, 5], np.uint32), np.array([tr.ONE, tr.ONE], np.uint16))
    assert g.base_tag_rows(tr.ONE) == 2
    # n == 0 changes nothing
    g.set_base_tags(np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    assert g.base_tag_rows(tr.ONE) == 2
    g.clear_base_tags()
    assert g.base_tags_info() == (0, N, 0)
    g.close()


def test_a_base_filter_is_not_combined_and_neither_reads_the_other(gpu, pkg, data):
    base, q, radius, btags, qtags = data
    g, f = gpu(), gpu()
    g.upload_base(base)
    f.upload_base(base)
    g.set_base_tags(ROWS, btags)
    # plain and _slots calls never read tags
    _same(g.exact_search(q, K), f.exact_search(q, K))
    _same_range(g.exact_range_search(q, radius), f.exact_range_search(q, radius))
    lab, deny = fr.pattern("rand03", N)
    qs = np.array([1, 0xff], np.uint8)[np.arange(NQ) % 2]
    for h in (g, f):
        h.set_base_filter_slot(1, lab, deny=deny)
    _same(g.exact_search_slots(q, K, qs), f.exact_search_slots(q, K, qs))
    # a _tags call ignores the slots
    want = tr.search_blocked(base, q, K, btags, qtags)
    _same(g.exact_search_tags(q, K, qtags), want)
    # a base filter installed: ERR_STATE, and the plain call under it is the parent's
    lab, deny = fr.pattern("gap", N)
    for h in (g, f):
        h.set_base_filter(lab, deny=deny)
    assert _status(pkg, lambda: g.exact_search_tags(q, K, qtags)) == pkg.ERR_STATE
    assert _status(pkg, lambda: g.exact_range_search_tags(q, radius, qtags)) == pkg.ERR_STATE
    _same(g.exact_search(q, K), f.exact_search(q, K))
    _same(g.exact_search_tags(q, K, None), f.exact_search(q, K))  # NULL is the plain call, base filter and all
    g.clear_base_filter()
    _same(g.exact_search_tags(q, K, qtags), want)
    _same_range(g.exact_range_search_tags(q, radius, qtags), tr.range_blocked(base, q, radius, btags, qtags))
    assert g.base_tags_info()[0] == int((btags != tr.NONE).sum())  # set / clear_base_filter did not touch the tags
    g.close()
    f.close()


def test_index_tags_and_base_tags_never_read_each_other(gpu, data):
    from test_gpu_filter_slots import base as corpus
    from test_gpu_remove import BASE, _upload
    base, q, radius, btags, qtags = data
    c = corpus(**BASE)  # the corpus the row-tag tests share
    g = _upload(gpu(), c)
    g.upload_base(base)
    ids = np.unique(c["ids"]).astype(np.uint32)
    g.set_tags(ids, (ids % 7).astype(np.uint16))
    assert g.base_tags_info() == (0, N, 0)
    index_info = g.tags_info()
    assert index_info[0] > 0
    three = g.tag_rows(3)
    g.set_base_tags(ROWS, btags)
    assert g.tags_info() == index_info and g.tag_rows(3) == three and g.base_tag_rows(3) == int((btags == 3).sum()) != three
    _same(g.exact_search_tags(q, K, qtags), tr.search_blocked(base, q, K, btags, qtags))
    g.clear_tags()
    assert g.base_tags_info()[0] == int((btags != tr.NONE).sum())
    g.clear_base_tags()
    g.close()


def test_upload_base_drops_the_tags_and_a_later_chunk_keeps_them(gpu, data):
    base, q, _, btags, qtags = data
    g = gpu()
    g.upload_base(base[:4000], n=N)
    g.set_base_tags(ROWS, btags)
    info = g.base_tags_info()
    g.upload_base(base[4000:], n=N, first=4000)  # a later chunk keeps them
    assert g.base_tags_info() == info
    _same(g.exact_search_tags(q, K, qtags), tr.search_blocked(base, q, K, btags, qtags))
    g.upload_base(base)  # first == 0: a new store
    assert g.base_tags_info() == (0, N, 0)
    got = g.exact_search_tags(q, K, qtags)
    assert (got[1][qtags != tr.NONE] == -1).all()
    _same(g.exact_search_tags(q, K, np.full(NQ, tr.NONE, np.uint16)), g.exact_search(q, K))
    g.set_base_tags(ROWS, btags)
    g.upload_base(np.zeros((0, D), np.uint8), n=0)  # n == 0: no store, no tags
    assert g.base_tags_info() == (0, 0, 0)
    g.close()


def test_views(gpu, pkg, data):
    base, q, radius, btags, qtags = data
    g = gpu()
    g.upload_base(base)
    v = g.view()
    assert _status(pkg, lambda: v.set_base_tags(ROWS, btags)) == pkg.ERR_STATE
    assert _status(pkg, lambda: v.clear_base_tags()) == pkg.ERR_STATE
    g.set_base_tags(ROWS, btags)  # after the view was made: a view reads its parent's tags at the call
    assert v.base_tags_info() == g.base_tags_info() and v.base_tag_rows(tr.SOME) == g.base_tag_rows(tr.SOME)
    _same(v.exact_search_tags(q, K, qtags), tr.search_blocked(base, q, K, btags, qtags))
    _same_range(v.exact_range_search_tags(q, radius, qtags), tr.range_blocked(base, q, radius, btags, qtags))
    g.clear_base_tags()
    assert v.base_tags_info() == (0, N, 0)
    v.close()
    g.close()


def test_null_query_tags_take_the_plain_path(gpu, data):
    base, q, radius, btags, qtags = data
    g, f = gpu(), gpu()
    g.upload_base(base)
    f.upload_base(base)
    _same(g.exact_search_tags(q, K, None), f.exact_search(q, K))
    _same_range(g.exact_range_search_tags(q, radius, None), f.exact_range_search(q, radius))
    assert g.memory_bytes() == f.memory_bytes()  # no plan, no plan workspace: the plain call's buffers and nothing else
    g.exact_search_tags(q, K, qtags)
    assert g.memory_bytes() > f.memory_bytes()
    g.close()
    f.close()


def test_memory_bytes_counts_the_tags(gpu, data):
    base, _, _, btags, _ = data
    g = gpu()
    g.upload_base(base)
    m0 = g.memory_bytes()
    g.set_base_tags(ROWS, btags)
    tagged = int((btags != tr.NONE).sum())
    assert g.memory_bytes() - m0 == 2 * N + 4 * tagged + 4 * 65537  # the sort's workspace is gone again
    g.set_base_tags(np.flatnonzero(btags == tr.MID).astype(np.uint32), np.full(int((btags == tr.MID).sum()), tr.NONE, np.uint16))
    assert g.memory_bytes() - m0 == 2 * N + 4 * (tagged - int((btags == tr.MID).sum())) + 4 * 65537
    g.clear_base_tags()
    assert g.memory_bytes() == m0
    g.close()
