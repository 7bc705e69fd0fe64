"""The exact calls with a base tag per query (ivfhnsw_gpu_exact_search_tags / ivfhnsw_gpu_exact_range_search_tags, DESIGN.md
3.22).  Every case is checked twice: (A) against the numpy restatement (tests/exact_tags_ref.py) -- labels, distance BITS,
lims in the caller's order -- and (B) against a second handle that installs each tag's rows with set_base_filter and runs
the plain call on that tag's queries.  The shapes are where the strip logic can break: groups of 31 / 32 / 33 and 129
queries, one query per tag, interleaved orders, absent tags, 300 tags of about 4 rows, forced column splits (at 64 most
splits of a 4-row tag are empty), with and without the tile map, more than one chunk.  Everything is exact: no tolerance
anywhere."""
import numpy as np
import pytest
import torch

import exact_filter_ref as fr
import exact_ref
import exact_tags_ref as tr

pytestmark = pytest.mark.gpu

F = np.float32


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
    """(base, queries, radii: 0, the median 10th-nearest distance over the whole store, +inf), computed once."""
    if (n, d, nq) not in _SHARED:
        base = tr.make_base(n, d)
        q = tr.make_queries(nq, d, base)
        kth = fr.search(base, q[:64], 10, np.ones(n, bool))[0][:, -1]
        _SHARED[n, d, nq] = (base, q, (F(0), F(np.median(kth)), F(np.inf)))
    return _SHARED[n, d, nq]


def _check_state(g, btags):
    """base_tags_info and base_tag_rows against numpy."""
    n = btags.size
    used = tr.tags_in_use(btags)
    assert g.base_tags_info() == (int((btags != tr.NONE).sum()), n, used.size)
    probe = set(int(t) for t in used[:40]) | {tr.NONE, tr.BIG, tr.FEW, tr.SOME, tr.ONE, 0, 254, 257, 0xfffd} | set(tr.ABSENT)
    for t in sorted(probe):
        assert g.base_tag_rows(t) == int((btags == t).sum()), t


def _install(g, btags):
    g.set_base_tags(np.arange(btags.size, dtype=np.uint32), btags)
    _check_state(g, btags)


def _per_tag_plain(g2, btags, q, qtags, k, radii):
    """(B): what the parent commit's calls answer, tag by tag, put back in the caller's order."""
    nq = q.shape[0]
    out_d = np.full((nq, k), exact_ref.FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    rng_q = [[None] * nq for _ in radii]
    for t in np.unique(qtags):
        idx = np.flatnonzero(qtags == t)
        if t == tr.NONE:
            g2.clear_base_filter()
        else:
            g2.set_base_filter(np.flatnonzero(btags == t).astype(np.uint32))  # an absent tag: the empty allow set
        out_d[idx], out_l[idx] = g2.exact_search(q[idx], k)
        for r, radius in enumerate(radii):
            lims, d, l = g2.exact_range_search(q[idx], radius)
            for j, qi in enumerate(idx):
                rng_q[r][qi] = (d[int(lims[j]):int(lims[j + 1])], l[int(lims[j]):int(lims[j + 1])])
    g2.clear_base_filter()
    ranges = []
    for per_q in rng_q:
        lims = np.zeros(nq + 1, np.uint64)
        lims[1:] = np.cumsum([p[0].size for p in per_q], dtype=np.uint64)
        ranges.append((lims, np.concatenate([p[0] for p in per_q]), np.concatenate([p[1] for p in per_q])))
    return (out_d, out_l), ranges


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k,nq,assign,splits,use_map", tr.grid())
def test_tag_calls_equal_the_restatement_and_the_per_tag_calls(gpu, n, d, k, nq, assign, splits, use_map):
    base, q, radii = _shared(n, d, nq)
    btags = tr.base_tags(n)
    qtags = tr.assignment(assign, n, nq)
    g = gpu()
    g.upload_base(base)
    g.set_option("exact_splits", splits)
    g.set_option("exact_range_map", use_map)
    _install(g, btags)
    want = tr.search_blocked(base, q, k, btags, qtags)
    _same(g.exact_search_tags(q, k, qtags), want)  # (A)
    want_r = [tr.range_blocked(base, q, r, btags, qtags) for r in radii]
    for r, w in zip(radii, want_r):
        _same_range(g.exact_range_search_tags(q, r, qtags), w)
    assert int(want_r[0][0][-1]) == 0 and int(want_r[2][0][-1]) == sum(int(tr.tag_mask(btags, t).sum()) for t in qtags)
    g2 = gpu()
    g2.upload_base(base)
    g2.set_option("exact_splits", splits)
    g2.set_option("exact_range_map", use_map)
    b_k, b_r = _per_tag_plain(g2, btags, q, qtags, k, radii)  # (B)
    _same(want, b_k)
    for w, b in zip(want_r, b_r):
        _same_range(w, b)
    # query_tags None is the plain call
    _same(g.exact_search_tags(q, k, None), g.exact_search(q, k))
    _same_range(g.exact_range_search_tags(q, radii[1], None), g.exact_range_search(q, radii[1]))
    g.close()
    g2.close()


# ---- 2. more than one chunk ----------------------------------------------------------------------------------------------------
def test_k_search_over_more_than_one_chunk(gpu):
    # k = 100 under 64 splits with 305 tags in use: the chunk rule gives 128 queries (tests/cpp/exact_tags_tool.cpp), so
    # 300 queries are three chunks, the last one of 44
    n, d, k, nq = tr.MANY_N, 16, 100, 300
    base, q, _ = _shared(n, d, nq)
    btags = tr.base_tags(n)
    assert tr.tags_in_use(btags).size >= 155
    g = gpu()
    g.upload_base(base)
    _install(g, btags)
    g.set_option("exact_splits", 64)
    for assign in ("many", "interleaved", "g129"):
        qtags = tr.assignment(assign, n, nq)
        _same(g.exact_search_tags(q, k, qtags), tr.search_blocked(base, q, k, btags, qtags))
    g.close()


def test_range_search_over_more_than_one_chunk(gpu):
    n, d, nq = tr.MANY_N, 16, 16500  # crosses the 16384 queries of a chunk
    base = tr.make_base(n, d)
    q = tr.make_queries(nq, d, base)
    btags = tr.base_tags(n)
    every = np.concatenate([tr.tags_in_use(btags), np.array([tr.NONE, tr.NONE, tr.ABSENT[0]], np.uint16)])
    qtags = every[np.random.default_rng(5).integers(0, every.size, nq)]
    dist = exact_ref.distances(base, q[:64])
    radius = F(np.sort(dist, axis=None)[dist.size // 50])
    g = gpu()
    g.upload_base(base)
    _install(g, btags)
    want = tr.range_blocked(base, q, radius, btags, qtags)
    assert int(want[0][-1]) > 1000
    for use_map in (0, 1):
        g.set_option("exact_range_map", use_map)
        _same_range(g.exact_range_search_tags(q, radius, qtags), want)
    g.close()


# ---- 3. the device forms -------------------------------------------------------------------------------------------------------
def test_dev_forms_with_misaligned_queries_and_a_row_stride(gpu):
    n, d, k, nq = tr.MANY_N, 48, 10, 300
    base, q, radii = _shared(n, d, nq)
    btags = tr.base_tags(n)
    qtags = tr.assignment("absent", n, nq)
    g = gpu()
    g.upload_base(base)
    dev = torch.device("cuda:0")
    d_rows = torch.arange(n, dtype=torch.int32, device=dev)
    d_tags = torch.from_numpy(btags.view(np.int16)).to(dev)
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    g.set_base_tags_dev(n, d_rows, d_tags)
    _check_state(g, btags)
    host_k = g.exact_search_tags(q, k, qtags)
    host_r = g.exact_range_search_tags(q, radii[1], qtags)
    _same(host_k, tr.search_blocked(base, q, k, btags, qtags))
    # the queries at an odd address, d + 4 bytes apart
    stride = d + 4
    raw = torch.zeros(nq * stride + 16, dtype=torch.uint8, device=dev)
    raw[3:3 + nq * stride].view(nq, stride)[:, :d] = torch.from_numpy(q).to(dev)
    dq = raw.data_ptr() + 3
    dt = torch.from_numpy(qtags.view(np.int16)).to(dev)
    od, ol = torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # the handle's stream is not torch's
    g.exact_search_tags_dev(nq, dq, stride, k, dt, od, ol)
    g.sync()
    _same((od.cpu().numpy(), ol.cpu().numpy()), host_k)
    dl = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    total = g.exact_range_search_tags_dev(nq, dq, stride, dt, float(radii[1]), dl)
    _same_range((dl.cpu().numpy().view(np.uint64), *g.exact_range_results(0, total)), host_r)
    g.close()


# ---- 4. incremental sets -------------------------------------------------------------------------------------------------------
def test_incremental_sets_retag_and_untag(gpu):
    n, d, k, nq = tr.MANY_N, 16, 10, 129
    base, q, radii = _shared(n, d, nq)
    btags = tr.base_tags(n)
    qtags = tr.assignment("interleaved", n, nq)
    rows = np.arange(n, dtype=np.uint32)
    one, three = gpu(), gpu()
    one.upload_base(base)
    three.upload_base(base)
    one.set_base_tags(rows, btags)
    perm = np.random.default_rng(3).permutation(n)  # in three calls of scattered rows, with rows beyond the store and repeats
    state = None
    for part in np.array_split(perm, 3):
        r = np.concatenate([rows[part], rows[part][:5], np.array([n, n + 100], np.uint32)])
        t = np.concatenate([btags[part], btags[part][:5], np.array([1, 2], np.uint16)])
        three.set_base_tags(r, t)
        state = tr.apply_sets(n, [(r, t)], state)
        _check_state(three, state)
    assert np.array_equal(state, btags)
    for t in np.unique(btags):
        assert one.base_tag_rows(int(t)) == three.base_tag_rows(int(t))
    want = tr.search_blocked(base, q, k, btags, qtags)
    _same(one.exact_search_tags(q, k, qtags), want)
    _same(three.exact_search_tags(q, k, qtags), want)
    _same_range(three.exact_range_search_tags(q, radii[1], qtags), tr.range_blocked(base, q, radii[1], btags, qtags))
    # retag a row of the big tag into the one-row tag, untag a tied row, tag an untagged one
    free = int(np.flatnonzero(btags == tr.NONE)[0])
    calls = [(np.array([2, 0, free], np.uint32), np.array([tr.ONE, tr.NONE, tr.FEW], np.uint16))]
    three.set_base_tags(*calls[0])
    now = tr.apply_sets(n, calls, btags)
    _check_state(three, now)
    assert three.base_tag_rows(tr.ONE) == 2 and three.base_tag_rows(tr.BIG) == one.base_tag_rows(tr.BIG) - 2
    qt = np.array([tr.ONE, tr.BIG, tr.NONE, tr.FEW], np.uint16)[np.arange(nq) % 4]
    _same(three.exact_search_tags(q, k, qt), tr.search_blocked(base, q, k, now, qt))
    _same_range(three.exact_range_search_tags(q, radii[2], qt), tr.range_blocked(base, q, radii[2], now, qt))
    _same(one.exact_search_tags(q, k, qt), tr.search_blocked(base, q, k, btags, qt))  # the other handle's store: untouched
    # every row untagged again: the array stays, nothing is tagged
    three.set_base_tags(rows, np.full(n, tr.NONE, np.uint16))
    _check_state(three, np.full(n, tr.NONE, np.uint16))
    _same(three.exact_search_tags(q, k, qt), tr.search_blocked(base, q, k, np.full(n, tr.NONE, np.uint16), qt))
    one.close()
    three.close()
