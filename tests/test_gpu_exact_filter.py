"""The exact calls under a base filter (ivfhnsw_gpu_set_base_filter): exact_search and exact_range_search
with an allow or deny set of row numbers installed, against the numpy restatement (tests/exact_filter_ref.py, pinned to
the unfiltered restatements by tests/test_exact_filter_cpu.py) -- labels, distance BITS and lims -- in both forms of the
sweep (pass words / list of passing rows), with forced column splits and with and without the range search's tile map;
the filter's state on the handle, the documented errors, and tools/ground_truth.py --allow / --deny end to end.
Everything is exact: no tolerance anywhere."""
import itertools
import os
import sys

import numpy as np
import pytest

import exact_filter_ref as fr
import exact_range_ref
import exact_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ground_truth  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
INF = F(np.inf)


def _base(rng, n, d):
    b = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    if n > 7:
        b[1] = b[0]          # exact ties: equal rows, so equal distances, ordered by label
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
    gd, gl = got
    wd, wl = want
    assert gl.dtype == np.int64 and gd.dtype == np.float32
    assert np.array_equal(gl, wl), np.nonzero((gl != wl).any(1))[0][:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _same_range(got, want):
    (gl, gd, gb), (wl, wd, wb) = got, want
    assert gl.dtype == np.uint64 and gd.dtype == np.float32 and gb.dtype == np.int64
    assert np.array_equal(gl, wl), np.nonzero(gl != wl)[0][:5]
    assert np.array_equal(gb, wb)
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
    assert int(gl[-1]) == gb.size  # the total is lims[-1]


def _bvecs(rows):
    n, d = rows.shape
    img = np.empty((n, d + 4), np.uint8)
    img[:, :4] = np.frombuffer(np.int32(d).tobytes(), np.uint8)
    img[:, 4:] = rows
    return img


def _median_radius(dist):
    return F(np.sort(dist, axis=None)[dist.size // 2])


DS, NS, NQS, KS = (16, 48, 128, 256), (1, 31, 33, 6001), (1, 33, 129), (1, 10, 100)
NP = len(fr.PATTERNS)


def _grid():
    cases = []
    for i, (d, n) in enumerate(itertools.product(DS, NS)):  # every (d, n); nq, k and the pattern cycling
        cases.append((d, n, NQS[i % 3], KS[(i + i // 3) % 3], fr.PATTERNS[i % NP]))
    for i, name in enumerate(fr.PATTERNS):  # every pattern on the store with many words and more than one tile per wave
        cases.append((128, 6001, NQS[(i + 1) % 3], KS[i % 3], name))
        cases.append((16, 33, NQS[i % 3], KS[(i + 2) % 3], name))
    # k above the passing rows (padding), and k = 100 (the 64-row strips) with 33 <= npass <= 99
    cases += [(48, 6001, 129, 100, "rand64"), (256, 6001, 33, 100, "rand64"), (16, 33, 33, 100, "rand50"), (48, 6001, 33, 10, "only7")]
    return sorted(set(cases))


GRID = _grid()
assert all({c[i] for c in GRID} == set(ax) for i, ax in enumerate((DS, NS, NQS, KS, fr.PATTERNS)))

_BASES = {}


def _shared(d, n, nq):
    """(base, queries, their distance matrix), computed once."""
    if (d, n, nq) not in _BASES:
        base = _base(np.random.default_rng(1000 * d + n), n, d)
        q = _queries(np.random.default_rng(d * 7919 + n * 31 + nq * 7), nq, d, base)
        _BASES[d, n, nq] = (base, q, exact_ref.distances(base, q))
    return _BASES[d, n, nq]


def _install(g, n, name, seed=0):
    labels, deny = fr.pattern(name, n, seed)
    mask = fr.pass_mask(n, labels, deny)
    g.set_base_filter(labels, deny=deny)
    assert g.base_filter_info() == (1 if deny else 0, int(mask.sum()), n)
    return mask


# ---- 1. the grid: both calls, every form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,nq,k,name", GRID)
def test_filtered_calls_equal_the_restatement(gpu, d, n, nq, k, name):
    base, q, dist = _shared(d, n, nq)
    g = gpu()
    g.upload_base(base)
    mask = _install(g, n, name)
    npass = int(mask.sum())
    want = fr.search(base, q, k, mask)
    radius = _median_radius(dist)
    want_r = fr.range_search(base, q, radius, mask)
    for form in (-1, 0, 1):
        g.set_option("exact_filter_form", form)
        got = g.exact_search(q, k)
        _same(got, want)
        if k > npass:
            assert (got[1][:, npass:] == -1).all() and (got[0][:, npass:] == exact_ref.FLT_MAX).all()
        _same_range(g.exact_range_search(q, radius), want_r)
    g.close()


def test_the_grid_has_the_padded_cases():
    npass = {c: int(fr.pass_mask(c[1], *fr.pattern(c[4], c[1])).sum()) for c in GRID}
    assert any(c[3] == 100 and 33 <= m <= 99 for c, m in npass.items())
    assert any(0 < m < c[3] for c, m in npass.items()) and any(m == 0 for m in npass.values())
    # the rule itself sends the sparse pattern to the list at n = 6001, the dense ones to the pass words
    assert npass[(128, 6001, NQS[(fr.PATTERNS.index("rand03") + 1) % 3], KS[fr.PATTERNS.index("rand03") % 3], "rand03")] <= 6001 // 8


# ---- 2. forms x splits: a split with no passing row, a compact split boundary inside a word ------------------------
@pytest.mark.parametrize("name", ("rand50", "rand03", "alt_first_empty", "alt_last_empty", "gap", "last", "deny0", "only7"))
def test_k_search_every_form_and_split_count(gpu, name):
    n, d, nq = 6001, 128, 5
    base, q, _ = _shared(d, n, nq)
    g = gpu()
    g.upload_base(base)
    mask = _install(g, n, name)
    want100, want1 = fr.search(base, q, 100, mask), fr.search(base, q, 1, mask)
    if name == "deny0":
        assert want100[1][0, :2].tolist() == [1, 7]  # query 0 is row 0, which is denied: its copies, lower label first
    if name == "only7":
        assert want100[1][0].tolist() == [7] + [-1] * 99
    for form in (0, 1, -1):
        g.set_option("exact_filter_form", form)
        for s in (1, 2, 5, 64):
            g.set_option("exact_splits", s)
            _same(g.exact_search(q, 100), want100)
            _same(g.exact_search(q, 1), want1)
        g.set_option("exact_splits", -1)
        _same(g.exact_search(q, 100), want100)
    g.close()


# ---- 3. the range search: radii, map, forms, splits, read back in halves -----------------------------------------------
@pytest.mark.parametrize("name", ("rand50", "rand03", "alt_last_empty", "gap", "first"))
def test_range_search_every_form_map_and_split_count(gpu, name):
    n, d, nq = 6001, 48, 33
    base, q, dist = _shared(d, n, nq)
    g = gpu()
    g.upload_base(base)
    mask = _install(g, n, name)
    for radius in (F(0.0), _median_radius(dist), INF):
        want = fr.range_search(base, q, radius, mask)
        if radius == INF:
            assert int(want[0][-1]) == nq * int(mask.sum())
        for form, use_map, s in itertools.product((0, 1), (0, 1), (-1, 2, 5, 64)):
            g.set_option("exact_filter_form", form)
            g.set_option("exact_range_map", use_map)
            g.set_option("exact_splits", s)
            got = g.exact_range_search(q, radius)
            _same_range(got, want)
        total = int(want[0][-1])
        half = total // 2
        a, b = g.exact_range_results(0, half), g.exact_range_results(half, total - half)
        assert np.array_equal(np.concatenate([a[1], b[1]]), want[2])
        assert np.array_equal(np.concatenate([a[0], b[0]]).view(np.uint32), want[1].view(np.uint32))
    g.set_option("exact_filter_form", -1)
    g.set_option("exact_range_map", -1)
    g.set_option("exact_splits", -1)
    _same_range(g.exact_range_search(q, _median_radius(dist)), fr.range_search(base, q, _median_radius(dist), mask))
    g.close()


# ---- 4. allow S = deny of the complement; the device form ----------------------------------------------------------------
def test_allow_equals_deny_of_the_complement_and_the_dev_form(gpu):
    import torch
    n, d, nq, k = 6001, 128, 33, 10
    base, q, dist = _shared(d, n, nq)
    s = np.random.default_rng(5).random(n) < 0.3
    allow, rest = np.flatnonzero(s).astype(np.uint32), np.flatnonzero(~s).astype(np.uint32)
    want, radius = fr.search(base, q, k, s), _median_radius(dist)
    want_r = fr.range_search(base, q, radius, s)
    a, b, c = gpu(), gpu(), gpu()
    for g in (a, b, c):
        g.upload_base(base)
    a.set_base_filter(allow)
    b.set_base_filter(rest, deny=True)
    dev = torch.device("cuda", 0)
    d_lab = torch.from_numpy(np.concatenate([[0], allow]).astype(np.uint32).view(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    c.set_base_filter_dev(allow.size, d_lab[1:])  # 4 bytes past an allocation boundary: aligned to 4, not to 8
    assert a.base_filter_info() == (0, int(s.sum()), n) and b.base_filter_info() == (1, int(s.sum()), n)
    assert c.base_filter_info() == a.base_filter_info()
    for g in (a, b, c):
        _same(g.exact_search(q, k), want)
        _same_range(g.exact_range_search(q, radius), want_r)
    # the device form of the search itself, under the filter
    tq = torch.from_numpy(q).to(dev)
    od = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ol = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    c.exact_search_dev(nq, tq, d, k, od, ol)
    c.sync()
    _same((od.cpu().numpy(), ol.cpu().numpy()), want)
    # an empty device set: allow nothing, deny nothing
    c.set_base_filter_dev(0, None)
    assert c.base_filter_info() == (0, 0, n) and (c.exact_search(q, k)[1] == -1).all()
    c.set_base_filter_dev(0, None, deny=True)
    assert c.base_filter_info() == (1, n, n)
    _same(c.exact_search(q, k), exact_ref.search(base, q, k))
    for g in (a, b, c):
        g.close()


def test_any_uint32_label_is_accepted(gpu):
    n, d, nq, k = 33, 16, 33, 10
    base, q, _ = _shared(d, n, nq)
    g = gpu()
    g.upload_base(base)
    labels = np.array([3, 32, 33, 1 << 20, 0xffffffff, 3], np.uint32)  # two rows, a repeat, three labels beyond the store
    mask = fr.pass_mask(n, labels)
    assert np.flatnonzero(mask).tolist() == [3, 32]
    g.set_base_filter(labels)
    assert g.base_filter_info() == (0, 2, n)
    _same(g.exact_search(q, k), fr.search(base, q, k, mask))
    g.set_base_filter(labels, deny=True)
    assert g.base_filter_info() == (1, n - 2, n)
    _same(g.exact_search(q, k), fr.search(base, q, k, ~mask))
    g.close()


# ---- 5. state ------------------------------------------------------------------------------------------------------------
def test_clear_replace_upload_and_memory(gpu, pkg):
    n, d, nq, k = 6001, 128, 33, 10
    base, q, dist = _shared(d, n, nq)
    radius = _median_radius(dist)
    plain, plain_r = exact_ref.search(base, q, k), exact_range_ref.from_distances(dist, radius)
    g = gpu()
    g.upload_base(base)
    assert g.base_filter_info() == (-1, n, n)
    g.clear_base_filter()  # none installed: succeeds
    _same(g.exact_search(q, k), plain)
    _same_range(g.exact_range_search(q, radius), plain_r)
    before = g.memory_bytes()
    m50 = _install(g, n, "rand50")
    assert g.memory_bytes() >= before + (n + 31) // 32 * 4  # at least the pass words
    _same(g.exact_search(q, k), fr.search(base, q, k, m50))
    # replacing: the sparse filter (which also keeps the list), then back
    m03 = _install(g, n, "rand03")
    assert g.memory_bytes() >= before + (n + 31) // 32 * 4 + 4 * int(m03.sum())
    _same(g.exact_search(q, k), fr.search(base, q, k, m03))
    _same_range(g.exact_range_search(q, radius), fr.range_search(base, q, radius, m03))
    # a failed set (an unknown mode) leaves the installed filter's results
    lab = np.arange(10, dtype=np.uint32)
    assert pkg.lib().ivfhnsw_gpu_set_base_filter(g._h, lab.size, lab.ctypes.data, 2) == pkg.ERR_INVALID
    assert g.base_filter_info() == (0, int(m03.sum()), n)
    _same(g.exact_search(q, k), fr.search(base, q, k, m03))
    # a later chunk keeps the filter (and its rows change what is found), first == 0 drops it
    g.upload_base(base[1000:2000], n=n, first=1000)
    assert g.base_filter_info() == (0, int(m03.sum()), n)
    _same(g.exact_search(q, k), fr.search(base, q, k, m03))
    g.clear_base_filter()
    assert g.base_filter_info() == (-1, n, n) and g.memory_bytes() == before
    _same(g.exact_search(q, k), plain)
    _same_range(g.exact_range_search(q, radius), plain_r)
    _install(g, n, "rand50")
    g.upload_base(base)
    assert g.base_filter_info() == (-1, n, n)
    _same(g.exact_search(q, k), plain)
    _install(g, n, "rand50")
    g.upload_base(np.zeros((0, d), np.uint8), n=0)  # no store: no filter either
    assert g.base_filter_info() == (-1, 0, 0)
    g.close()


def test_a_view_reads_its_parents_filter_at_the_call(gpu, pkg):
    n, d, nq, k = 6001, 128, 33, 10
    base, q, dist = _shared(d, n, nq)
    g = gpu()
    g.upload_base(base)
    v = g.view()
    _same(v.exact_search(q, k), exact_ref.search(base, q, k))
    m = _install(g, n, "rand03")  # installed after the view was created
    assert v.base_filter_info() == g.base_filter_info()
    _same(v.exact_search(q, k), fr.search(base, q, k, m))
    _same_range(v.exact_range_search(q, INF), fr.range_search(base, q, INF, m))
    v.set_option("exact_filter_form", 0)
    _same(v.exact_search(q, k), fr.search(base, q, k, m))
    m = _install(g, n, "rand50")  # keeps no list: a view forced to the list form builds its own
    v.set_option("exact_filter_form", 1)
    _same(v.exact_search(q, k), fr.search(base, q, k, m))
    m = _install(g, n, "gap")     # ... and does not reuse it for the next filter
    _same(v.exact_search(q, k), fr.search(base, q, k, m))
    with pytest.raises(pkg.IvfHnswError) as e:
        v.set_base_filter(np.arange(3, dtype=np.uint32))
    assert e.value.code == pkg.ERR_STATE
    with pytest.raises(pkg.IvfHnswError) as e:
        v.clear_base_filter()
    assert e.value.code == pkg.ERR_STATE
    _same(v.exact_search(q, k), fr.search(base, q, k, m))
    g.clear_base_filter()
    _same(v.exact_search(q, k), exact_ref.search(base, q, k))
    v.close()
    g.close()


def test_index_filter_and_base_filter_do_not_disturb_each_other(gpu):
    from conftest import corpus
    c = corpus(seed=7, nc=128, d=128, M=16, n_base=8000, nq=32, efConstruction=100)
    nprobe, max_codes = 8, 2000

    def index(g):
        g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                     c["pq_centroids"], c["norm_table"])
        gr = c["graph"]
        g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
        return g

    n, d, nq, k = 6001, 128, 33, 10
    base, q, _ = _shared(d, n, nq)
    ids = np.asarray(c["ids"], np.uint32)
    index_allow = np.random.default_rng(1).choice(ids, len(ids) // 4, replace=False).astype(np.uint32)
    g, ref = index(gpu()), index(gpu())
    ref.set_filter(index_allow)
    want_ivf = ref.search(c["queries"], 10, nprobe, max_codes, efSearch=40)
    g.upload_base(base)
    unfiltered_ivf = g.search(c["queries"], 10, nprobe, max_codes, efSearch=40)
    # the base filter first, then the index filter with another set
    m = _install(g, n, "rand03")
    _same(g.search(c["queries"], 10, nprobe, max_codes, efSearch=40), unfiltered_ivf)
    g.set_filter(index_allow)
    assert g.filter_info()[0] == 0 and g.base_filter_info() == (0, int(m.sum()), n)
    _same(g.search(c["queries"], 10, nprobe, max_codes, efSearch=40), want_ivf)
    _same(g.exact_search(q, k), fr.search(base, q, k, m))
    # replacing or clearing one leaves the other
    m = _install(g, n, "rand50")
    _same(g.search(c["queries"], 10, nprobe, max_codes, efSearch=40), want_ivf)
    g.clear_filter()
    assert g.filter_info()[0] == -1 and g.base_filter_info() == (0, int(m.sum()), n)
    _same(g.exact_search(q, k), fr.search(base, q, k, m))
    g.set_filter(index_allow)
    g.clear_base_filter()
    _same(g.search(c["queries"], 10, nprobe, max_codes, efSearch=40), want_ivf)
    _same(g.exact_search(q, k), exact_ref.search(base, q, k))
    g.close()
    ref.close()


# ---- 6. errors -------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_earlier_state(gpu, pkg):
    import torch
    n, d, nq, k = 33, 16, 33, 10
    base, q, _ = _shared(d, n, nq)
    g = gpu()
    lab = np.array([1, 2, 3], np.uint32)
    L = pkg.lib()

    def code(f, *a, **kw):
        with pytest.raises(pkg.IvfHnswError) as e:
            f(*a, **kw)
        return e.value.code

    # before upload_base: every entry point but info and clear
    assert code(g.set_base_filter, lab) == pkg.ERR_STATE
    assert "upload_base" in L.ivfhnsw_gpu_last_error().decode()
    assert code(g.set_base_filter_dev, 0, None) == pkg.ERR_STATE
    g.clear_base_filter()
    assert g.base_filter_info() == (-1, 0, 0)
    g.upload_base(base)  # no index on this handle: none is needed
    mask = _install(g, n, "rand50")
    want = fr.search(base, q, k, mask)

    def intact():
        assert g.base_filter_info()[:2] == (0, int(mask.sum()))
        _same(g.exact_search(q, k), want)

    assert L.ivfhnsw_gpu_set_base_filter(g._h, 3, None, pkg.FILTER_ALLOW) == pkg.ERR_INVALID     # null labels, n > 0
    intact()
    assert L.ivfhnsw_gpu_set_base_filter_dev(g._h, 3, None, pkg.FILTER_DENY) == pkg.ERR_INVALID
    intact()
    for mode in (-1, 2):                                                                          # an unknown mode
        assert L.ivfhnsw_gpu_set_base_filter(g._h, 3, lab.ctypes.data, mode) == pkg.ERR_INVALID
        assert L.ivfhnsw_gpu_set_base_filter(g._h, 0, None, mode) == pkg.ERR_INVALID
        intact()
    dev = torch.device("cuda", 0)
    t = torch.zeros(16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    assert L.ivfhnsw_gpu_set_base_filter_dev(g._h, 2, t.data_ptr() + 2, pkg.FILTER_ALLOW) == pkg.ERR_INVALID  # misaligned
    assert "aligned" in L.ivfhnsw_gpu_last_error().decode()
    intact()
    for bad in (-2, 2, 7):                                                                        # the option's values
        assert code(g.set_option, "exact_filter_form", bad) == pkg.ERR_INVALID
        intact()
    assert L.ivfhnsw_gpu_abi_version() == 9
    g.close()


# ---- 7. the tool -------------------------------------------------------------------------------------------------------------
def test_ground_truth_tool_allow_and_deny_end_to_end(gpu, tmp_path):
    rng = np.random.default_rng(47)
    n, d, nq, k = 3001, 128, 25, 100
    base = _base(rng, n, d)
    q = _queries(rng, nq, d, base)
    dist = exact_ref.distances(base, q)
    s = rng.random(n) < 0.1
    labels = np.flatnonzero(s).astype(np.uint32)
    bp, qp, out, outz = (str(tmp_path / f) for f in ("base.bvecs", "query.bvecs", "gt.ivecs", "gt.npz"))
    ap, dp = str(tmp_path / "allow.ivecs"), str(tmp_path / "deny.npy")
    _bvecs(base).tofile(bp)
    _bvecs(q).tofile(qp)
    ground_truth.write_ivecs(ap, labels[None, :])
    np.save(dp, labels.astype(np.int64))
    common = ["--base", bp, "--queries", qp]
    ground_truth.main(common + ["--k", str(k), "--out", out, "--allow", ap])
    assert np.array_equal(ground_truth.read_ivecs(out), fr.search(base, q, k, s)[1])
    ground_truth.main(common + ["--k", "1", "--out", out, "--deny", dp])
    assert np.array_equal(ground_truth.read_ivecs(out), fr.search(base, q, 1, ~s)[1])
    r = _median_radius(dist)
    for flag, path, mask, mode in (("--allow", ap, s, 0), ("--deny", dp, ~s, 1)):
        ground_truth.main(common + ["--radius", repr(float(r)), "--out", outz, flag, path])
        lims, dd, lab, radius = ground_truth.read_range(outz)
        assert radius == float(r)
        _same_range((lims, dd, lab), fr.range_search(base, q, r, mask))
        assert ground_truth.read_range_filter(outz) == (mode, int(mask.sum()))
    ground_truth.main(common + ["--radius", repr(float(r)), "--out", outz])
    assert ground_truth.read_range_filter(outz) == (-1, None)
    with pytest.raises(SystemExit):  # the two flags are exclusive
        ground_truth.main(common + ["--k", "1", "--out", out, "--allow", ap, "--deny", dp])
