"""The exact calls with a base filter slot per query (ivfhnsw_gpu_exact_search_slots / ivfhnsw_gpu_exact_range_search_slots,
DESIGN.md 3.20).  Every case is checked twice: (A) against the numpy restatement (tests/exact_filter_slots_ref.py) -- labels,
distance BITS, lims in the caller's order -- and (B) against a second handle that installs each slot's set with
set_base_filter and runs the plain call on that slot's queries.  The shapes are where the strip logic can break: groups of
31 / 32 / 33 and 129 queries, one query per slot, interleaved orders, slots that are not set, every form of the sweep, forced
column splits, with and without the tile map, more than one chunk.  Everything is exact: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import exact_filter_ref as fr
import exact_filter_slots_ref as sr
import exact_ref

pytestmark = pytest.mark.gpu

F = np.float32


def _base(rng, n, d):  # the ties of tests/test_gpu_exact_filter.py's _base
    b = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    if n > 7:
        b[1] = b[0]
        b[7] = b[0]
        b[n - 1] = b[3]
        b[4] = 0
        b[5] = 255
    return b


def _queries(rng, nq, d, base):
    q = rng.integers(0, 256, size=(nq, d), dtype=np.uint8)
    q[0] = base[0]
    if nq > 2:
        q[1] = 0
        q[2] = 255
    return q


def _same(got, want):
    (gd, gl), (wd, wl) = got, want
    assert gl.dtype == np.int64 and gd.dtype == np.float32
    assert np.array_equal(gl, wl), np.nonzero((gl != wl).any(1))[0][:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _same_range(got, want):
    (gl, gd, gb), (wl, wd, wb) = got, want
    assert gl.dtype == np.uint64 and gd.dtype == np.float32 and gb.dtype == np.int64
    assert np.array_equal(gl, wl), np.nonzero(gl != wl)[0][:5]
    assert np.array_equal(gb, wb)
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
    assert int(gl[-1]) == gb.size


_SHARED = {}


def _shared(n, d, nq):
    """(base, queries, a radius about a third of the distances lie below), computed once."""
    if (n, d, nq) not in _SHARED:
        base = _base(np.random.default_rng(1000 * d + n), n, d)
        q = _queries(np.random.default_rng(d * 7919 + n * 31 + nq * 7), nq, d, base)
        dist = exact_ref.distances(base, q[:64])
        _SHARED[n, d, nq] = (base, q, F(np.sort(dist, axis=None)[dist.size // 3]))
    return _SHARED[n, d, nq]


def _install(g, n, sets):
    masks = sr.slot_masks(n, sets)
    for s, (labels, deny) in sets.items():
        g.set_base_filter_slot(s, labels, deny=deny)
        assert g.base_filter_slot_info(s) == (1 if deny else 0, int(masks[s].sum()), n)
    return masks


def _per_slot_plain(g2, n, sets, q, qslots, k, radius):
    """(B): what the parent commit's calls answer, slot by slot, put back in the caller's order."""
    nq = q.shape[0]
    out_d = np.full((nq, k), exact_ref.FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    rng_q = [(np.zeros(0, np.float32), np.zeros(0, np.int64))] * nq
    for b in np.unique(qslots):
        idx = np.flatnonzero(qslots == b)
        if b == sr.NONE:
            g2.clear_base_filter()
        elif int(b) in sets:
            g2.set_base_filter(sets[int(b)][0], deny=sets[int(b)][1])
        else:
            continue  # a slot that is not set passes nothing
        out_d[idx], out_l[idx] = g2.exact_search(q[idx], k)
        lims, d, l = g2.exact_range_search(q[idx], radius)
        for j, qi in enumerate(idx):
            rng_q[qi] = (d[int(lims[j]):int(lims[j + 1])], l[int(lims[j]):int(lims[j + 1])])
    lims = np.zeros(nq + 1, np.uint64)
    lims[1:] = np.cumsum([p[0].size for p in rng_q], dtype=np.uint64)
    return (out_d, out_l), (lims, np.concatenate([p[0] for p in rng_q]), np.concatenate([p[1] for p in rng_q]))


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k,nq,assign,splits,use_map", sr.grid())
def test_slot_calls_equal_the_restatement_and_the_per_slot_calls(gpu, n, d, k, nq, assign, splits, use_map):
    base, q, radius = _shared(n, d, nq)
    sets = sr.slot_sets(n)
    qslots = sr.assignment(assign, nq)
    g = gpu()
    g.upload_base(base)
    g.set_option("exact_splits", splits)
    g.set_option("exact_range_map", use_map)
    want = want_r = None
    for form in (-1, 0, 1):
        g.set_option("exact_filter_form", form)  # before the slots are set: 1 keeps every slot's list
        masks = _install(g, n, sets)
        if want is None:
            want = sr.search_blocked(base, q, k, masks, qslots)
            want_r = sr.range_blocked(base, q, radius, masks, qslots)
        _same(g.exact_search_slots(q, k, qslots), want)  # (A)
        _same_range(g.exact_range_search_slots(q, radius, qslots), want_r)
    g2 = gpu()
    g2.upload_base(base)
    b_k, b_r = _per_slot_plain(g2, n, sets, q, qslots, k, radius)  # (B)
    _same(want, b_k)
    _same_range(want_r, b_r)
    # query_slots None is the plain call
    _same(g.exact_search_slots(q, k, None), g.exact_search(q, k))
    g.close()
    g2.close()


# ---- 2. more than one chunk ----------------------------------------------------------------------------------------------------
def test_k_search_over_more_than_one_chunk(gpu):
    # exact_splits = 64 and k = 100: 256 MB / (64 * 100 * 8 B) = 5242 -> chunks of 5120 queries
    n, d, k, nq = 6001, 16, 100, 5200
    base, q, _ = _shared(n, d, nq)
    sets = sr.slot_sets(n)
    qslots = np.array(sr.SET + (sr.NONE,) + sr.UNSET, np.uint8)[np.arange(nq) % 15]
    g = gpu()
    g.upload_base(base)
    masks = _install(g, n, sets)
    g.set_option("exact_splits", 64)
    _same(g.exact_search_slots(q, k, qslots), sr.search_blocked(base, q, k, masks, qslots))
    g.close()


def test_range_search_over_more_than_one_chunk(gpu):
    n, d, nq = 6001, 16, 16500  # crosses the 16384 queries of a chunk
    base, q, _ = _shared(n, d, nq)
    sets = sr.slot_sets(n)
    qslots = np.array(sr.SET + (sr.NONE,) + sr.UNSET, np.uint8)[np.arange(nq) % 15]
    dist = exact_ref.distances(base, q[:64])
    radius = F(np.sort(dist, axis=None)[dist.size // 200])
    g = gpu()
    g.upload_base(base)
    masks = _install(g, n, sets)
    want = sr.range_blocked(base, q, radius, masks, qslots)
    assert int(want[0][-1]) > nq
    for use_map in (0, 1):
        g.set_option("exact_range_map", use_map)
        _same_range(g.exact_range_search_slots(q, radius, qslots), want)
    g.close()


# ---- 3. the device forms -------------------------------------------------------------------------------------------------------
def test_dev_forms_equal_the_host_forms_and_unknown_bytes_pass_nothing(gpu, pkg):
    n, d, k, nq = 6001, 48, 10, 300
    base, q, radius = _shared(n, d, nq)
    sets = sr.slot_sets(n)
    qslots = sr.assignment("unset", nq)
    g = gpu()
    g.upload_base(base)
    masks = _install(g, n, sets)
    host_k = g.exact_search_slots(q, k, qslots)
    host_r = g.exact_range_search_slots(q, radius, qslots)
    dev = torch.device("cuda:0")
    dq, ds = torch.from_numpy(q).to(dev), torch.from_numpy(qslots).to(dev)
    od, ol = torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)
    g.exact_search_slots_dev(nq, dq, d, k, ds, od, ol)
    g.sync()
    _same((od.cpu().numpy(), ol.cpu().numpy()), host_k)
    dl = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    total = g.exact_range_search_slots_dev(nq, dq, d, ds, float(radius), dl)
    rd, rl = g.exact_range_results(0, total)
    _same_range((dl.cpu().numpy().view(np.uint64), rd, rl), host_r)

    # bytes 32..254: the device forms pass nothing for them, the host forms refuse the call and write nothing
    bad = qslots.copy()
    bad[5], bad[17] = 32, 254
    as_unset = bad.copy()
    as_unset[[5, 17]] = sr.UNSET[0]
    g.exact_search_slots_dev(nq, dq, d, k, torch.from_numpy(bad).to(dev), od, ol)
    g.sync()
    _same((od.cpu().numpy(), ol.cpu().numpy()), sr.search_blocked(base, q, k, masks, as_unset))
    assert (ol[5] == -1).all() and (ol[17] == -1).all()
    total = g.exact_range_search_slots_dev(nq, dq, d, torch.from_numpy(bad).to(dev), float(radius), dl)
    want_r = sr.range_blocked(base, q, radius, masks, as_unset)
    _same_range((dl.cpu().numpy().view(np.uint64), *g.exact_range_results(0, total)), want_r)
    for call in (lambda: g.exact_search_slots(q, k, bad), lambda: g.exact_range_search_slots(q, radius, bad)):
        with pytest.raises(pkg.IvfHnswError) as e:
            call()
        assert e.value.code == pkg.ERR_INVALID
    _same_range((dl.cpu().numpy().view(np.uint64), *g.exact_range_results(0, total)), want_r)  # the held results stand
    g.close()
