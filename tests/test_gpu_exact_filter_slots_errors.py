"""Base filter slots: their state on the handle and the documented errors -- info after set, replace and
clear; a slot replaced between two calls; upload_base dropping and keeping them; views; the statuses of every refused call;
what memory_bytes counts; a failed call leaving results and slots as they were; plain and single-filter calls untouched by
the slots a handle holds.  Exact throughout."""
import numpy as np
import pytest
import torch

import exact_filter_ref as fr
import exact_filter_slots_ref as sr

pytestmark = pytest.mark.gpu

F = np.float32
N, D, NQ, K = 6001, 48, 40, 10


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(77)
    base = rng.integers(0, 256, size=(N, D), dtype=np.uint8)
    q = rng.integers(0, 256, size=(NQ, D), dtype=np.uint8)
    import exact_ref
    dist = exact_ref.distances(base, q)
    return base, q, F(np.sort(dist, axis=None)[dist.size // 4])


def _same(got, want):
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def _same_range(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _status(pkg, call):
    with pytest.raises(pkg.IvfHnswError) as e:
        call()
    return e.value.code


def test_info_after_set_replace_and_clear(gpu, data):
    base = data[0]
    g = gpu()
    g.upload_base(base)
    assert all(g.base_filter_slot_info(s) == (-1, 0, N) for s in range(32))
    g.set_base_filter_slot(3, np.arange(100, dtype=np.uint32))
    g.set_base_filter_slot(31, np.array([5, 5, N, N + 9], np.uint32), deny=True)
    assert g.base_filter_slot_info(3) == (0, 100, N) and g.base_filter_slot_info(31) == (1, N - 1, N)
    g.set_base_filter_slot(3, np.zeros(0, np.uint32), deny=True)  # replaced: an empty deny set passes everything
    assert g.base_filter_slot_info(3) == (1, N, N)
    g.clear_base_filter_slot(3)
    g.clear_base_filter_slot(3)  # succeeds on a slot that is not set
    assert g.base_filter_slot_info(3) == (-1, 0, N) and g.base_filter_slot_info(31) == (1, N - 1, N)
    g.set_base_filter_slot(0, np.arange(7, dtype=np.uint32))
    g.clear_base_filter_slot()  # every slot
    assert all(g.base_filter_slot_info(s) == (-1, 0, N) for s in range(32))
    assert g.base_filter_info() == (-1, N, N)  # the base filter is other state
    g.close()


def test_a_replaced_slot_changes_only_its_queries(gpu, data):
    base, q, radius = data
    g = gpu()
    g.upload_base(base)
    sets = {0: fr.pattern("rand50", N), 1: fr.pattern("rand03", N)}
    for s, (lab, deny) in sets.items():
        g.set_base_filter_slot(s, lab, deny=deny)
    qs = np.array([0, 1, sr.NONE, 5], np.uint8)[np.arange(NQ) % 4]
    before = g.exact_search_slots(q, K, qs)
    _same(before, sr.search(base, q, K, sr.slot_masks(N, sets), qs))
    sets[1] = fr.pattern("alt_first_empty", N)
    g.set_base_filter_slot(1, sets[1][0], deny=sets[1][1])
    after = g.exact_search_slots(q, K, qs)
    _same(after, sr.search(base, q, K, sr.slot_masks(N, sets), qs))
    other = qs != 1
    assert np.array_equal(before[1][other], after[1][other]) and not np.array_equal(before[1][~other], after[1][~other])
    _same_range(g.exact_range_search_slots(q, radius, qs), sr.range_search(base, q, radius, sr.slot_masks(N, sets), qs))
    g.close()


def test_upload_base_drops_the_slots_and_a_later_chunk_keeps_them(gpu, data):
    base, q, _ = data
    g = gpu()
    g.upload_base(base[:4000], n=N)
    g.set_base_filter_slot(2, np.arange(50, 5000, dtype=np.uint32))
    g.upload_base(base[4000:], n=N, first=4000)  # a later chunk keeps them
    assert g.base_filter_slot_info(2) == (0, 4950, N)
    qs = np.full(NQ, 2, np.uint8)
    masks = {2: fr.pass_mask(N, np.arange(50, 5000))}
    _same(g.exact_search_slots(q, K, qs), sr.search(base, q, K, masks, qs))
    g.upload_base(base)  # first == 0: a new store
    assert g.base_filter_slot_info(2) == (-1, 0, N)
    got = g.exact_search_slots(q, K, qs)
    assert (got[1] == -1).all()
    _same(g.exact_search_slots(q, K, np.full(NQ, sr.NONE, np.uint8)), g.exact_search(q, K))
    g.close()


def test_views(gpu, pkg, data):
    base, q, radius = data
    g = gpu()
    g.upload_base(base)
    v = g.view()
    lab, deny = fr.pattern("rand03", N)
    assert _status(pkg, lambda: v.set_base_filter_slot(0, lab)) == pkg.ERR_STATE
    assert _status(pkg, lambda: v.clear_base_filter_slot(0)) == pkg.ERR_STATE
    g.set_base_filter_slot(0, lab, deny=deny)  # after the view was made: a view reads its parent's slots at the call
    qs = np.array([0, sr.NONE], np.uint8)[np.arange(NQ) % 2]
    masks = {0: fr.pass_mask(N, lab, deny)}
    assert v.base_filter_slot_info(0) == g.base_filter_slot_info(0)
    _same(v.exact_search_slots(q, K, qs), sr.search(base, q, K, masks, qs))
    _same_range(v.exact_range_search_slots(q, radius, qs), sr.range_search(base, q, radius, masks, qs))
    v.close()
    g.close()


def test_refused_calls(gpu, pkg, data):
    base, q, radius = data
    L = pkg.lib()
    g = gpu()
    qs = np.zeros(NQ, np.uint8)
    lab = np.arange(10, dtype=np.uint32)
    # before upload_base
    assert _status(pkg, lambda: g.exact_search_slots(q, K, qs)) == pkg.ERR_STATE
    assert _status(pkg, lambda: g.exact_range_search_slots(q, radius, qs)) == pkg.ERR_STATE
    assert _status(pkg, lambda: g.set_base_filter_slot(0, lab)) == pkg.ERR_STATE
    g.upload_base(base)
    assert _status(pkg, lambda: g.set_base_filter_slot(32, lab)) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.base_filter_slot_info(32)) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.clear_base_filter_slot(32)) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_set_base_filter_slot(g._h, 0, 10, lab.ctypes.data, 7) == pkg.ERR_INVALID  # an unknown mode
    assert L.ivfhnsw_gpu_set_base_filter_slot(g._h, 0, 10, None, 0) == pkg.ERR_INVALID            # NULL labels, n > 0
    d_lab = torch.arange(12, dtype=torch.int32, device="cuda:0")
    assert L.ivfhnsw_gpu_set_base_filter_slot_dev(g._h, 0, 8, d_lab.data_ptr() + 2, 0) == pkg.ERR_INVALID  # misaligned
    assert all(g.base_filter_slot_info(s)[0] == -1 for s in range(32))
    g.set_base_filter_slot_dev(0, 10, d_lab)
    assert g.base_filter_slot_info(0) == (0, 10, N)
    # the plain calls' own refusals come with their status
    assert _status(pkg, lambda: g.exact_search_slots(q, 101, qs)) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.exact_range_search_slots(q, float("nan"), qs)) == pkg.ERR_INVALID
    # a base filter installed: not combined
    g.set_base_filter(lab)
    assert _status(pkg, lambda: g.exact_search_slots(q, K, qs)) == pkg.ERR_STATE
    assert _status(pkg, lambda: g.exact_range_search_slots(q, radius, qs)) == pkg.ERR_STATE
    g.clear_base_filter()
    g.exact_search_slots(q, K, qs)
    g.close()


def test_memory_bytes_counts_the_slots(gpu, data):
    base = data[0]
    g = gpu()
    g.upload_base(base)
    g.set_base_filter_slot(9, np.arange(3000, dtype=np.uint32))  # the first slot brings the table and the count's word
    words = 4 * ((N + 31) // 32)
    m0 = g.memory_bytes()
    g.set_base_filter_slot(0, np.arange(3000, dtype=np.uint32))  # 3000 > n / 8: pass words alone
    m1 = g.memory_bytes()
    assert m1 - m0 == words
    g.set_base_filter_slot(1, np.arange(700, dtype=np.uint32))   # 700 <= n / 8: the list as well
    m2 = g.memory_bytes()
    assert m2 - m1 == words + 4 * 700
    g.set_base_filter_slot(1, np.arange(3000, dtype=np.uint32))  # replaced by a set without a list
    assert g.memory_bytes() == m2 - 4 * 700
    g.clear_base_filter_slot(1)
    assert g.memory_bytes() == m1
    g.clear_base_filter_slot(0)
    assert g.memory_bytes() == m0
    g.close()


def test_a_failed_call_leaves_results_and_slots_as_they_were(gpu, pkg, data):
    base, q, radius = data
    g = gpu()
    g.upload_base(base)
    lab, deny = fr.pattern("rand50", N)
    g.set_base_filter_slot(4, lab, deny=deny)
    qs = np.array([4, sr.NONE], np.uint8)[np.arange(NQ) % 2]
    held = g.exact_range_search_slots(q, radius, qs)
    total = int(held[0][-1])
    info = [g.base_filter_slot_info(s) for s in range(32)]
    bad = qs.copy()
    bad[3] = 100
    assert _status(pkg, lambda: g.exact_range_search_slots(q, radius, bad)) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.exact_search_slots(q, K, bad)) == pkg.ERR_INVALID
    assert _status(pkg, lambda: g.set_base_filter_slot(40, lab)) == pkg.ERR_INVALID
    assert pkg.lib().ivfhnsw_gpu_set_base_filter_slot(g._h, 4, 10, None, 0) == pkg.ERR_INVALID
    assert [g.base_filter_slot_info(s) for s in range(32)] == info
    d, l = g.exact_range_results(0, total)
    assert np.array_equal(l, held[2]) and np.array_equal(d.view(np.uint32), held[1].view(np.uint32))
    _same_range(g.exact_range_search_slots(q, radius, qs), held)
    g.close()


def test_plain_and_single_filter_calls_do_not_read_the_slots(gpu, data):
    base, q, radius = data
    g, f = gpu(), gpu()
    g.upload_base(base)
    f.upload_base(base)
    for s, name in ((0, "none"), (1, "rand03"), (2, "rand50")):
        lab, deny = fr.pattern(name, N)
        g.set_base_filter_slot(s, lab, deny=deny)
    _same(g.exact_search(q, K), f.exact_search(q, K))
    _same_range(g.exact_range_search(q, radius), f.exact_range_search(q, radius))
    lab, deny = fr.pattern("gap", N)
    g.set_base_filter(lab, deny=deny)
    f.set_base_filter(lab, deny=deny)
    _same(g.exact_search(q, K), f.exact_search(q, K))
    _same_range(g.exact_range_search(q, radius), f.exact_range_search(q, radius))
    g.clear_base_filter()
    assert g.base_filter_slot_info(1)[0] == 0  # the base filter's calls did not touch the slots
    g.close()
    f.close()
