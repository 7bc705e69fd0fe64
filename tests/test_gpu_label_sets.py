"""The calls that take a set of uint32 labels -- the filter, the filter slots (3.19), the base filter
(3.18), removal (3.11), locate and reconstruct by label (3.16) -- share their host steps (csrc/capi_labels.cpp; DESIGN.md
1b): the largest label, the staging of host labels, the sizing and build of the label bitmap, the argument guards.  Three
parts: the same label arrays through all five subjects, host form and device form, against numpy; every argument refusal
of the ten entry points with its code and text, after which the handle answers as before; and what the calls leave
allocated.

One small IVFADC index built with numpy (nc 16, 1000 rows, d 16, M 4, no oracle, searched with host coarse results), a
Grouping twin of it for removal, and a base store of 1000 rows.  The ids are distinct, unordered and have gaps; 0, 31, 32
and 64 are among them and 63 is not, so that the first bits of the bitmap's first three words are all met.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NC, D, M, N, NSUBC = 16, 16, 4, 1000, 8
BASE_N, NQ, NPROBE, K = 1000, 8, 4, 10
TOP = 0xffffffff


def _index():
    rng = np.random.default_rng(20)
    sizes = rng.multinomial(N, np.full((NC - 1) * NSUBC, 1.0 / ((NC - 1) * NSUBC))).reshape(NC - 1, NSUBC)
    sizes = np.insert(sizes, 5, 0, axis=0).astype(np.int64)   # list 5 is empty
    off = np.concatenate([[0], np.cumsum(sizes.sum(1))]).astype(np.uint64)
    pool = np.setdiff1d(np.arange(1, 3000), [31, 32, 63, 64])
    ids = rng.permutation(np.concatenate([[0, 31, 32, 64], rng.choice(pool, N - 4, replace=False)])).astype(np.uint32)
    ix = dict(sizes=sizes, off=off, ids=ids, codes=rng.integers(0, 256, (N, M), dtype=np.uint8),
              ncodes=rng.integers(0, 256, N, dtype=np.uint8), cnorm=rng.random(NC, dtype=np.float32),
              pq=rng.standard_normal(256 * D).astype(np.float32), ntab=rng.random(256, dtype=np.float32),
              q=rng.standard_normal((NQ, D)).astype(np.float32),
              cid=np.stack([rng.permutation(NC)[:NPROBE] for _ in range(NQ)]).astype(np.uint32),
              cd=np.sort(rng.random((NQ, NPROBE), dtype=np.float32), axis=1),
              base=rng.integers(0, 256, (BASE_N, D), dtype=np.uint8), bq=rng.integers(0, 256, (NQ, D), dtype=np.uint8))
    ix["list_of_row"] = np.repeat(np.arange(NC), sizes.sum(1))
    ix["sub_of_row"] = np.concatenate([np.repeat(np.arange(NSUBC), s) for s in sizes])
    return ix


IX = _index()


def _upload(g, grouping=False, **shard):
    g.upload_ivf(D, M, IX["off"], IX["ids"], IX["codes"], IX["ncodes"], IX["cnorm"], IX["pq"], IX["ntab"], **shard)
    if grouping:
        g.upload_grouping(NSUBC, np.ones(NC, np.float32), np.zeros((NC, NSUBC), np.uint32), IX["sizes"].astype(np.uint32),
                          np.zeros((NC, NSUBC), np.float32))
    return g


def _search(g):
    return g.search(IX["q"], 1, NPROBE, 10 ** 6, coarse_ids=IX["cid"], coarse_dists=IX["cd"])


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return None
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def g(gpu):
    """The index and the base store on one handle, for the subjects that leave both as they are."""
    h = _upload(gpu())
    h.upload_base(IX["base"])
    return h


# ---- 1. the same label arrays through every subject ----------------------------------------------------------------------
def _cases():
    ids = IX["ids"]
    rng = np.random.default_rng(21)
    absent = np.setdiff1d(np.arange(3000), ids)[:40].astype(np.uint32)
    return {
        "empty": np.zeros(0, np.uint32),
        "0": np.array([0], np.uint32),
        "31": np.array([31], np.uint32),
        "32": np.array([32], np.uint32),
        "63_64": np.array([63, 64], np.uint32),
        "one": ids[500:501].copy(),
        "all": ids.copy(),
        "repeats": np.concatenate([ids[10:60], ids[10:60], ids[30:31], ids[30:31]]),
        "unsorted": rng.permutation(np.concatenate([ids[::3], np.arange(100, 200, dtype=np.uint32)])),
        "absent": absent,
        "far_above": np.concatenate([ids[::7], [1 << 20]]).astype(np.uint32),
        "top": np.concatenate([[TOP], ids[5:400:5], [TOP]]).astype(np.uint32),
    }


CASES = _cases()


@pytest.mark.parametrize("case", list(CASES))
def test_filters_and_locate_against_numpy(g, case):
    import torch
    labels = CASES[case]
    n, d_labels = len(labels), _to_dev(labels)
    hit = int(np.isin(IX["ids"], labels).sum())
    base_hit = int(np.isin(np.arange(BASE_N), labels).sum())
    assert case in ("empty", "absent") or hit > 0
    for deny in (False, True):
        want = (int(deny), N - hit if deny else hit, N)
        base_want = (int(deny), BASE_N - base_hit if deny else base_hit, BASE_N)
        for dev in (False, True):
            g.clear_filter()
            g.clear_filter_slot()
            g.clear_base_filter()
            if dev:
                g.set_filter_dev(n, d_labels, deny=deny)
                g.set_filter_slot_dev(0, n, d_labels, deny=deny)
                g.set_filter_slot_dev(31, n, d_labels, deny=deny)
                g.set_base_filter_dev(n, d_labels, deny=deny)
            else:
                g.set_filter(labels, deny=deny)
                g.set_filter_slot(0, labels, deny=deny)
                g.set_filter_slot(31, labels, deny=deny)
                g.set_base_filter(labels, deny=deny)
            assert g.filter_info() == want, (deny, dev)
            assert g.filter_slot_info(0) == want and g.filter_slot_info(31) == want, (deny, dev)
            assert g.filter_slot_info(1) == (-1, 0, N)
            assert g.base_filter_info() == base_want, (deny, dev)
    # locate: the lowest row bearing each label (the ids are distinct: at most one) and how many bear it
    order = np.argsort(IX["ids"])
    pos = np.searchsorted(IX["ids"], labels, sorter=order).clip(0, N - 1)
    found = IX["ids"][order[pos]] == labels if n else np.zeros(0, bool)
    rows_want = np.where(found, order[pos], -1).astype(np.int64) if n else np.zeros(0, np.int64)
    rows, counts = g.locate(labels)
    assert np.array_equal(rows, rows_want) and np.array_equal(counts, found.astype(np.uint32))
    dev0 = torch.device("cuda", 0)
    d_rows = torch.full((max(n, 1),), 7, dtype=torch.int64, device=dev0)
    d_counts = torch.full((max(n, 1),), 7, dtype=torch.int32, device=dev0)
    g.locate_dev(n, d_labels, d_rows, d_counts)
    if n:
        assert np.array_equal(d_rows.cpu().numpy(), rows_want)
        assert np.array_equal(d_counts.cpu().numpy().view(np.uint32), found.astype(np.uint32))
    else:
        assert int(d_rows[0]) == 7 and int(d_counts[0]) == 7


@pytest.mark.parametrize("grouping", [False, True], ids=["ivfadc", "grouping"])
@pytest.mark.parametrize("case", list(CASES))
def test_removal_against_numpy(gpu, pkg, case, grouping):
    import torch
    labels = CASES[case]
    gone = np.isin(IX["ids"], labels)
    per_list = np.bincount(IX["list_of_row"][gone], minlength=NC).astype(np.uint32)
    sizes = np.zeros((NC, NSUBC), np.uint32)
    np.add.at(sizes, (IX["list_of_row"][~gone], IX["sub_of_row"][~gone]), 1)
    for dev in (False, True):
        h = _upload(pkg.GpuIndex(0), grouping)   # a fresh upload per case and form
        if dev:
            d_per = torch.full((NC,), 7, dtype=torch.int32, device=torch.device("cuda", 0))
            n_removed = h.remove_ids_dev(len(labels), _to_dev(labels), d_per)
            per = d_per.cpu().numpy().view(np.uint32)
        else:
            n_removed, per = h.remove_ids(labels)
        assert n_removed == int(gone.sum()) and np.array_equal(per, per_list), dev
        off, ids, codes, ncodes = h.download_ivf()
        assert np.array_equal(ids, IX["ids"][~gone]) and np.array_equal(codes, IX["codes"][~gone])
        assert np.array_equal(np.diff(off.astype(np.int64)), np.bincount(IX["list_of_row"][~gone], minlength=NC))
        if grouping:
            assert np.array_equal(h.download_grouping(), sizes)
        h.close()


# ---- 2. the refusals of the ten entry points -----------------------------------------------------------------------------
NULL_TEXT = {"locate": "locate: null labels or rows", "locate_dev": "locate_dev: null labels or rows",
             "reconstruct": "reconstruct: null labels or out", "reconstruct_dev": "reconstruct_dev: null labels or out"}
ALIGN_TEXT = {"set_filter_dev": "set_filter_dev: labels must be 4-byte aligned",
              "set_filter_slot_dev": "set_filter_slot_dev: labels must be 4-byte aligned",
              "set_base_filter_dev": "set_base_filter_dev: labels must be 4-byte aligned",
              "locate_dev": "locate_dev: labels and counts must be 4-byte aligned, rows 8-byte",
              "reconstruct_dev": "reconstruct_dev: labels and out must be 4-byte aligned"}   # remove_ids_dev checks none
VIEW_TEXT = {"set_filter": "a filter goes to the handle that holds the tables, not to a view of it",
             "set_filter_slot": "a filter goes to the handle that holds the tables, not to a view of it",
             "set_base_filter": "a base filter goes to the handle that holds the store, not to a view of it",
             "remove_ids": "removals go to the handle that holds the tables, not to a view of it"}  # locate, reconstruct: a view may
SHARD_TEXT = {"set_filter": "sharded handles have no label filter", "set_filter_slot": "sharded handles have no label filter",
              "remove_ids": "so sharded handles have no removal", "locate": "a shard holds only its own lists",
              "reconstruct": "a shard holds only its own lists"}   # the base store knows no shards
ENTRIES = ["set_filter", "set_filter_slot", "set_base_filter", "remove_ids", "locate", "reconstruct"]


def test_refusals(gpu, pkg, g):
    import torch
    L = pkg.lib()
    dev0 = torch.device("cuda", 0)
    labels = IX["ids"][::4].copy()
    n = len(labels)
    d_labels = torch.from_numpy(np.concatenate([labels, labels[:1]]).view(np.int32)).to(dev0)
    d_rows = torch.zeros(n, dtype=torch.int64, device=dev0)
    d_out = torch.zeros((n, D), dtype=torch.float32, device=dev0)
    d_per = torch.zeros(NC, dtype=torch.int32, device=dev0)
    rows, out, per, miss = np.zeros(n, np.int64), np.zeros((n, D), np.float32), np.zeros(NC, np.uint32), C.c_uint64(0)
    torch.cuda.synchronize(dev0)

    def call(name, h, n_, host_ptr, dev_ptr, mode=pkg.FILTER_ALLOW):
        """rc of entry point `name` (a _dev name: its device form) on handle h with n_ labels at the pointer."""
        dev = name.endswith("_dev")
        p = dev_ptr if dev else host_ptr
        f = getattr(L, "ivfhnsw_gpu_" + name)
        stem = name[:-4] if dev else name
        if stem in ("set_filter", "set_base_filter"):
            return f(h._h, n_, p, mode)
        if stem == "set_filter_slot":
            return f(h._h, 31, n_, p, mode)
        if stem == "remove_ids":
            return f(h._h, n_, p, None, d_per.data_ptr() if dev else per.ctypes.data)
        if stem == "locate":
            return f(h._h, n_, p, d_rows.data_ptr() if dev else rows.ctypes.data, None)
        return f(h._h, n_, p, pkg.RECON_ORIGINAL, d_out.data_ptr() if dev else out.ctypes.data, C.byref(miss))

    def refused(rc, code, text):
        assert rc == code, (rc, L.ivfhnsw_gpu_last_error().decode())
        assert text in L.ivfhnsw_gpu_last_error().decode(), (text, L.ivfhnsw_gpu_last_error().decode())

    # the handle under test: a filter, slots 0 and 31, a base filter, and a quantizer so that reconstruct gets as far as
    # its arguments (sixteen nodes, every node linked to every other; no walk runs here)
    nodes = np.arange(NC, dtype=np.uint32)
    links = np.stack([np.concatenate([np.delete(nodes, i), [0]]) for i in range(NC)]).astype(np.uint32)
    g.upload_quantizer(np.full(NC, NC - 1, np.uint8), links, np.random.default_rng(22).standard_normal((NC, D)).astype(np.float32))
    g.clear_filter_slot()
    g.set_filter(IX["ids"][::2])
    g.set_filter_slot(0, IX["ids"][::3])
    g.set_filter_slot(31, IX["ids"][::5], deny=True)
    g.set_base_filter(np.arange(0, BASE_N, 3), deny=True)
    infos = lambda: (g.filter_info(), [g.filter_slot_info(s) for s in range(32)], g.base_filter_info())
    info0, search0, exact0 = infos(), _search(g), g.exact_search(IX["bq"], K)
    assert info0[0] == (0, N // 2, N) and info0[1][31] == (1, N - N // 5, N) and (search0[1] >= 0).any()

    def in_force():
        assert infos() == info0
        assert _same(_search(g), search0) and _same(g.exact_search(IX["bq"], K), exact0)

    view, empty, shard = g.view(), gpu(), gpu()
    sel = np.concatenate([np.arange(int(IX["off"][c]), int(IX["off"][c + 1])) for c in range(0, NC, 3)])
    shard.upload_ivf(D, M, IX["off"], IX["ids"][sel], IX["codes"][sel], IX["ncodes"][sel], IX["cnorm"], IX["pq"], IX["ntab"],
                     shard_rank=0, shard_world=3)
    for stem in ENTRIES:
        for name in (stem, stem + "_dev"):
            # null labels with n > 0
            refused(call(name, g, n, None, None), pkg.ERR_INVALID, NULL_TEXT.get(name, name + ": null labels"))
            in_force()
            # a mode that is neither allow nor deny
            if stem.startswith("set_"):
                for mode in (2, -1):
                    refused(call(name, g, n, labels.ctypes.data, d_labels.data_ptr(), mode), pkg.ERR_INVALID,
                            "%s: mode %d is neither IVFHNSW_FILTER_ALLOW nor IVFHNSW_FILTER_DENY" % (name, mode))
                in_force()
            # a device pointer off 4-byte alignment
            if name in ALIGN_TEXT:
                refused(call(name, g, n, None, d_labels.data_ptr() + 2), pkg.ERR_INVALID, ALIGN_TEXT[name])
                in_force()
            # on a view
            if stem in VIEW_TEXT:
                refused(call(name, view, n, labels.ctypes.data, d_labels.data_ptr()), pkg.ERR_STATE,
                        "%s: %s" % (name, VIEW_TEXT[stem]))
                in_force()
            # before the upload it needs
            refused(call(name, empty, n, labels.ctypes.data, d_labels.data_ptr()), pkg.ERR_STATE,
                    "%s before %s" % (name, "upload_base" if stem == "set_base_filter" else "upload_ivf"))
            # on a sharded handle
            if stem in SHARD_TEXT:
                refused(call(name, shard, n, labels.ctypes.data, d_labels.data_ptr()), pkg.ERR_STATE,
                        "%s: the handle is shard 0 of 3" % name)
                assert SHARD_TEXT[stem] in L.ivfhnsw_gpu_last_error().decode()
    in_force()
    assert _same(_search(view), search0)   # the view went on filtering as its parent
    assert empty.filter_info() == (-1, 0, 0) and empty.base_filter_info() == (-1, 0, 0)
    assert shard.filter_info() == (-1, len(sel), len(sel)) and shard.filter_slot_info(31) == (-1, 0, len(sel))
    view.close()
    in_force()


# ---- 3. what the calls leave allocated -----------------------------------------------------------------------------------
def test_set_and_clear_return_to_the_same_bytes(gpu):
    h = _upload(gpu())
    h.upload_base(IX["base"])
    labels, d_labels = CASES["far_above"], _to_dev(CASES["far_above"])
    n = len(labels)
    rounds = {
        "filter": (lambda: h.set_filter(labels), lambda: h.set_filter_dev(n, d_labels, deny=True), h.clear_filter),
        "one slot": (lambda: h.set_filter_slot(5, labels), lambda: h.set_filter_slot_dev(5, n, d_labels, deny=True),
                     lambda: h.clear_filter_slot(5)),
        "all slots": (lambda: [h.set_filter_slot(s, labels[s:]) for s in range(32)],
                      lambda: [h.set_filter_slot_dev(s, n, d_labels) for s in range(32)], h.clear_filter_slot),
        "base filter": (lambda: h.set_base_filter(labels), lambda: h.set_base_filter_dev(n, d_labels, deny=True),
                        h.clear_base_filter),
    }
    for what, (set_host, set_dev, clear) in rounds.items():
        set_host()
        held = h.memory_bytes()
        clear()
        first = h.memory_bytes()
        assert first < held, what
        set_dev()
        clear()
        assert h.memory_bytes() == first, what
        set_host()
        clear()
        assert h.memory_bytes() == first, what


def test_repeated_remove_and_locate_keep_their_bytes(gpu):
    h = _upload(gpu())
    absent, d_absent = CASES["absent"], _to_dev(CASES["absent"])
    assert h.remove_ids(absent)[0] == 0
    held = h.memory_bytes()
    assert h.remove_ids(absent)[0] == 0 and h.memory_bytes() == held
    assert h.remove_ids_dev(len(absent), d_absent) == 0
    held = h.memory_bytes()
    assert h.remove_ids_dev(len(absent), d_absent) == 0 and h.memory_bytes() == held
    labels = CASES["unsorted"]
    first = h.locate(labels)
    held = h.memory_bytes()
    assert _same(h.locate(labels), first) and h.memory_bytes() == held
    assert np.array_equal(h.download_ivf()[1], IX["ids"])


def test_a_view_leaves_its_parents_label_sets(gpu):
    """A view reads the filter and the slots of its parent and owns none of their buffers: destroying it frees nothing
    the parent holds."""
    h = _upload(gpu())
    h.set_filter(IX["ids"][::2])
    h.set_filter_slot(0, IX["ids"][::3])
    h.set_filter_slot(31, IX["ids"][1::3], deny=True)
    qs = np.resize(np.array([0, 31, 0xff], np.uint8), NQ)
    slots = lambda x: x.search_slots(IX["q"], 1, qs, NPROBE, 10 ** 6, coarse_ids=IX["cid"], coarse_dists=IX["cd"])
    plain = _search(h)
    held = h.memory_bytes()
    v = h.view()
    assert _same(_search(v), plain) and v.filter_info() == h.filter_info() == (0, N // 2, N)
    assert v.filter_slot_info(31) == h.filter_slot_info(31)
    v.close()
    assert h.memory_bytes() == held
    assert _same(_search(h), plain) and h.filter_info() == (0, N // 2, N)
    # the kept bitmaps are still the parent's: an update re-marks filter and slots from them
    gone = IX["ids"][:100]
    assert h.remove_ids(gone)[0] == 100
    left = IX["ids"][100:]
    assert h.filter_info() == (0, int(np.isin(left, IX["ids"][::2]).sum()), N - 100)
    assert h.filter_slot_info(0) == (0, int(np.isin(left, IX["ids"][::3]).sum()), N - 100)
    assert h.filter_slot_info(31) == (1, int((~np.isin(left, IX["ids"][1::3])).sum()), N - 100)
    h.clear_filter()
    v = h.view()
    by_slot = slots(h)
    assert _same(slots(v), by_slot) and (by_slot[1][qs == 0] >= 0).any()
    v.close()
    assert _same(slots(h), by_slot)
