"""The value domain of the float16 base store, beyond integers 0..127 and standard normals.

1. The device's own bits as the reference.  exact_range_search_f16(q, +inf) gates nothing and returns every pair: the matrix
   B of the float32 values the device computes.  B is held to float64 within the documented bound, and every other call --
   the k-searches, the range searches at radii small, zero and negative, plain and tagged -- to B bit for bit: a gate that is
   a little too tight, or a selection that mishandles negative keys, loses a pair here.  Rows near a common large offset
   make distances tiny against the norms, many of them tied and some negative.
2. One power of two times an integer is exact: every value a subnormal half (2^-24), 2^-10, and 2^9 (values to 65 024).
3. The upload's rounding at float16's edges against numpy's, through the re-rank, from host and from strided device rows.
4. A query that does not round to a finite half gets padding / no results and leaves its strip's other queries alone.
5. The device-pointer entry points and a call of two query chunks."""
import itertools

import numpy as np
import pytest

import exact_f16_ref as fr
import exact_range_ref
import exact_ref
import exact_tags_ref as tr
import rerank_ref

pytestmark = pytest.mark.gpu

F = np.float32


def _same(got, want):
    assert np.array_equal(got[1], want[1]), np.nonzero((got[1] != want[1]).any(1))[0][:5]
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def _same_range(got, want):
    assert np.array_equal(got[0], want[0]), np.nonzero(got[0] != want[0])[0][:5]
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _code(pkg, f, *a, **kw):
    with pytest.raises(pkg.IvfHnswError) as e:
        f(*a, **kw)
    return e.value.code


# ---- 1. the device's own bits as the reference ------------------------------------------------------------------------------
N1, NQ1 = 1000, 70
REGIMES = {
    "near30": lambda seed, n, d: fr.offset_rows(seed, n, d, 30.0, 0.05),    # distances far below the norms, many negative bits
    "near2000": lambda seed, n, d: fr.offset_rows(seed, n, d, 2000.0, 1.0),  # the halves' spacing is 1 to 2 there: duplicates, ties
    "normal3": lambda seed, n, d: (np.random.default_rng(seed).standard_normal((n, d), dtype=F) * F(3)).astype(F),
}
R1 = [(r, d) for r in REGIMES for d in (96, 208)]  # d = 208: thirteen MFMA steps, the per-wave kernels' parts 7 and 6
_R1 = {}


@pytest.fixture(scope="module")
def regime(pkg):
    """Per (regime, d), made once: rows, queries, tags, a handle holding them, the float64 truth and the device's bit matrices
    -- B of the plain call and Bt of the tagged one, each from a range search at +inf."""
    def get(name, d):
        if (name, d) not in _R1:
            x, q = REGIMES[name](10 * d, N1, d), REGIMES[name](10 * d + 1, NQ1, d)
            q[1] = x[5]
            if name == "normal3":
                q[0] = 0  # |q|^2 = 0
            btags = (np.arange(N1) % 3).astype(np.uint16)
            qtags = np.array([0, 1, 2, tr.NONE], np.uint16)[np.arange(NQ1) % 4]
            g = pkg.GpuIndex(0)
            g.upload_base_f16(x)
            g.set_base_tags(np.arange(N1, dtype=np.uint32), btags)
            g.set_option("exact_splits", 3)
            B = fr.matrix_of(*g.exact_range_search_f16(q, np.inf), N1)
            Bt = fr.matrix_of(*g.exact_range_search_f16_tags(q, np.inf, qtags), N1)
            D, tol = fr.truth(x, q)
            mine = np.stack([tr.tag_mask(btags, t) for t in qtags])
            _R1[name, d] = dict(x=x, q=q, qtags=qtags, g=g, B=B, Bt=Bt, D=D, tol=tol, mine=mine)
        return _R1[name, d]
    yield get
    for s in _R1.values():
        s["g"].close()
    _R1.clear()


@pytest.mark.parametrize("name,d", R1)
def test_the_bits_are_within_the_bound_of_float64(regime, name, d):
    s = regime(name, d)
    B, Bt, D, tol = s["B"], s["Bt"], s["D"], s["tol"]
    assert not np.isnan(B).any()                                   # +inf returns every pair,
    assert np.array_equal(~np.isnan(Bt), s["mine"])                # ... under tags every pair of the query's tag and no other,
    assert np.array_equal(Bt[s["mine"]].view(np.uint32), B[s["mine"]].view(np.uint32))  # ... with the plain call's bits
    ratio = np.abs(B.astype(np.float64) - D) / tol
    print("%s d %d: largest |B - D| / tol = %.4f; %d of %d bits negative, %d distinct values; D in [%.4g, %.4g], |x|^2 about %.4g"
          % (name, d, ratio.max(), int((B < 0).sum()), B.size, np.unique(B).size, D.min(), D.max(), (s["x"].astype(np.float64) ** 2).sum(1).mean()))
    assert (ratio <= 1.0).all()
    if name != "normal3":
        assert np.median(D) < 2.0 ** -8 * (s["x"].astype(np.float64) ** 2).sum(1).mean()  # the regime: distances small against the norms
        assert np.unique(B).size < B.size // 4                                            # ... and many of them tied


@pytest.mark.parametrize("name,d,k,splits", [(r, d, k, sp) for r, d in R1 for k in (1, 16, 33, 100) for sp in (1, 3)])
def test_k_search_selects_from_the_bits(regime, name, d, k, splits):
    s = regime(name, d)
    s["g"].set_option("exact_splits", splits)
    _same(s["g"].exact_search_f16(s["q"], k), fr.topk_of_bits(s["B"], k))
    _same(s["g"].exact_search_f16_tags(s["q"], k, s["qtags"]), fr.topk_of_bits(s["Bt"], k, s["mine"]))


def _radius(B, which):
    """B: the entries a call may return."""
    v = np.sort(B[~np.isnan(B)])
    return {"median": float(np.median(v)),
            "entry": float(v[v.size // 10]),                        # an entry of B itself: strict <, the pairs ON it stay out
            "zero": 0.0,
            "above_min": float(np.nextafter(v[0], F(np.inf))),     # the successor of the most negative entry: the least entries alone
            "-inf": -np.inf}[which]


@pytest.mark.parametrize("name,d,which,use_map", [(r, d, w, m) for r, d in R1 for w in ("median", "entry", "zero", "above_min", "-inf")
                                                  for m in (0, 1)])
def test_range_search_cuts_the_bits(regime, name, d, which, use_map):
    s = regime(name, d)
    g = s["g"]
    g.set_option("exact_splits", 3)
    g.set_option("exact_range_map", use_map)
    r = _radius(s["B"], which)
    want = fr.range_of_bits(s["B"], r)
    _same_range(g.exact_range_search_f16(s["q"], r), want)
    rt = _radius(s["Bt"], which)
    want_t = fr.range_of_bits(s["Bt"], rt, s["mine"])
    _same_range(g.exact_range_search_f16_tags(s["q"], rt, s["qtags"]), want_t)
    if which == "-inf":
        assert want[0][-1] == 0 and want_t[0][-1] == 0
    elif which == "above_min":
        assert 1 <= want[0][-1] < s["B"].size // 2
    elif which != "zero":
        assert 0 < want[0][-1] < s["B"].size and 0 < want_t[0][-1] < s["mine"].sum()


# ---- 2. one power of two times an integer is exact --------------------------------------------------------------------------
@pytest.mark.parametrize("log2_scale,d", list(itertools.product((-24, -10, 9), (96, 256))))
def test_a_power_of_two_times_integers_is_exact(pkg, log2_scale, d):
    n, nq = 300, 33
    xi, x = fr.scaled_ints(20 * d, n, d, log2_scale)
    qi, q = fr.scaled_ints(20 * d + 1, nq, d, log2_scale)
    qi[0], q[0] = xi[7], x[7]
    if log2_scale == -24:  # every stored value is a subnormal half (or zero)
        assert ((fr.rounded(x).view(np.uint16) & 0x7c00) == 0).all() and np.array_equal(fr.rounded(x).astype(F), x)
    sq = np.float64(2.0) ** (2 * log2_scale)
    D = exact_ref.distances(xi, qi)
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x)
    want = exact_ref.search(xi, qi, 33)
    got = g.exact_search_f16(q, 33)
    print("scale 2^%d d %d: query 1's nearest: returned %r, exact %r" % (log2_scale, d, float(got[0][1, 0]), float(want[0][1, 0] * sq)))
    _same(got, ((want[0].astype(np.float64) * sq).astype(F), want[1]))
    low = float(np.sort(D, axis=None)[D.size // 20])
    for r in (low, low + 0.5, np.inf):
        lims, dist, lab = exact_range_ref.from_distances(D, r)
        _same_range(g.exact_range_search_f16(q, float(F(r * sq))), (lims, (dist.astype(np.float64) * sq).astype(F), lab))
    g.close()


# ---- 3. the upload's rounding against numpy's, through the re-rank -----------------------------------------------------------
def _edge_rows(d):
    """float32 [m, d]: edge_values() padded with ones to a length m coprime to d and laid end to end m times, so that every
    value visits every column -- every lane and slot of the store's permutation."""
    ev = fr.edge_values()
    m = ev.size
    while np.gcd(m, d) != 1:
        m += 1
    ev = np.concatenate([ev, np.ones(m - ev.size, F)])
    return np.tile(ev, d).reshape(m, d)


def _upload(g, x, how):
    """x into handle g from the host, from the host in two chunks, or from device rows a stride of d + 3 floats apart whose
    padding holds NaN (which the check must not read).  Returns what must stay alive."""
    n, d = x.shape
    if how == "host":
        g.upload_base_f16(x)
    elif how == "chunks":
        g.upload_base_f16(x[:n // 3], n=n, first=0)
        g.upload_base_f16(x[n // 3:], n=n, first=n // 3)
    else:
        import torch
        wide = np.full((n, d + 3), np.nan, F)
        wide[:, :d] = x
        t = torch.from_numpy(wide).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        g.upload_base_f16_dev(n, d, 0, n, t, row_stride=d + 3)
        return t


@pytest.mark.parametrize("d,how", list(itertools.product((16, 48), ("host", "chunks", "dev"))))
def test_upload_rounds_as_numpy_does(pkg, d, how):
    x = _edge_rows(d)
    n = len(x)
    xh = fr.rounded(x).astype(F)
    assert np.isfinite(xh).all() and (xh != x).any()
    g = pkg.GpuIndex(0)
    keep = _upload(g, x, how)
    assert g.base_kind() == pkg.BASE_F16
    cand = np.arange(n, dtype=np.int64)[:, None]
    dist, lab = g.rerank(xh, cand, 1)  # the query IS the row numpy's rounding stores: any other half in the store shows
    assert np.array_equal(lab, cand)
    assert np.array_equal(dist.view(np.uint32), np.zeros((n, 1), np.uint32)), np.nonzero(dist[:, 0])[0][:5]
    _same(g.rerank(x, cand, 1), rerank_ref.rerank(xh, x, cand, 1))  # the unrounded query against the rounded store
    del keep
    g.close()


@pytest.mark.parametrize("case", ["nan", "65520", "-65520", "misaligned"])
def test_upload_dev_refusals(pkg, case):
    import torch
    d, n = 16, 40
    rng = np.random.default_rng(11)
    x, q = rng.integers(0, 128, (n, d), dtype=np.uint8), rng.integers(0, 128, (5, d), dtype=np.uint8)
    want = exact_ref.search(x, q, 10)
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x.astype(F))
    wide = np.zeros((n, d + 3), F)
    wide[:, :d] = x[::-1]
    if case != "misaligned":
        wide[n - 1, d - 1] = {"nan": np.nan, "65520": 65520.0, "-65520": -65520.0}[case]  # the last value the check reads
    t = torch.from_numpy(wide).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    if case == "misaligned":
        assert _code(pkg, g.upload_base_f16_dev, n, d, 0, n, t.data_ptr() + 2, row_stride=d + 3) == pkg.ERR_INVALID
    else:
        assert _code(pkg, g.upload_base_f16_dev, n, d, 0, n, t, row_stride=d + 3) == pkg.ERR_INVALID  # a new store,
        assert _code(pkg, g.upload_base_f16_dev, n, d, 20, 20, t.data_ptr() + 20 * (d + 3) * 4, row_stride=d + 3) == pkg.ERR_INVALID  # a chunk
    _same(g.exact_search_f16(q.astype(F), 10), want)  # the old store still answers
    if case == "65520":  # ... and the value just below is taken
        wide[n - 1, d - 1] = np.nextafter(F(65520), F(0))
        t2 = torch.from_numpy(wide).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        g.upload_base_f16_dev(n, d, 0, n, t2, row_stride=d + 3)
        dist, _ = g.rerank(np.full((1, d), 0, F), np.array([[n - 1]], np.int64), 1)
        assert dist[0, 0] == rerank_ref.rerank(fr.rounded(wide[:, :d]).astype(F), np.zeros((1, d), F), np.array([[n - 1]]), 1)[0][0, 0]
    g.close()


# ---- 4. queries that do not round to a finite half ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [96, 208])
def test_a_query_beyond_float16_gets_nothing_and_harms_nobody(pkg, d):
    n, nq = 300, 70
    rng = np.random.default_rng(40 + d)
    x, qi = rng.integers(0, 128, (n, d), dtype=np.uint8), rng.integers(0, 128, (nq, d), dtype=np.uint8)
    btags = (np.arange(n) % 3).astype(np.uint16)
    qtags = np.array([0, 1, 2, tr.NONE], np.uint16)[np.arange(nq) % 4]
    q = qi.astype(F)
    # one bad query per tag and one untagged, each among ordinary queries of its strip; query 0 is also the row that pads
    # the strips of a tag plan
    bad = {0: np.nan, 5: np.inf, 38: 65520.0, 67: -1e6}
    for i, v in bad.items():
        q[i, (7 * i) % d] = v
    good = np.setdiff1d(np.arange(nq), list(bad))
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x.astype(F))
    g.set_base_tags(np.arange(n, dtype=np.uint32), btags)
    for splits in (1, 3):
        g.set_option("exact_splits", splits)
        for k in (16, 100):
            for got, alone, want in ((g.exact_search_f16(q, k), g.exact_search_f16(q[good], k), exact_ref.search(x, qi[good], k)),
                                     (g.exact_search_f16_tags(q, k, qtags), g.exact_search_f16_tags(q[good], k, qtags[good]),
                                      tr.search_blocked(x, qi[good], k, btags, qtags[good]))):
                assert (got[1][list(bad)] == -1).all() and (got[0][list(bad)] == exact_ref.FLT_MAX).all()
                _same((got[0][good], got[1][good]), alone)
                _same(alone, want)
    g.set_option("exact_splits", 3)
    D = exact_ref.distances(x, qi)
    for r in (float(np.median(D)), np.inf):
        for got, alone, want in ((g.exact_range_search_f16(q, r), g.exact_range_search_f16(q[good], r),
                                  exact_range_ref.from_distances(D[good], r)),
                                 (g.exact_range_search_f16_tags(q, r, qtags), g.exact_range_search_f16_tags(q[good], r, qtags[good]),
                                  tr.range_blocked(x, qi[good], r, btags, qtags[good]))):
            sizes = np.diff(got[0].astype(np.int64))
            assert (sizes[list(bad)] == 0).all()
            assert np.array_equal(sizes[good], np.diff(alone[0].astype(np.int64)))
            assert np.array_equal(got[2], alone[2]) and np.array_equal(got[1].view(np.uint32), alone[1].view(np.uint32))
            _same_range(alone, want)
    g.close()


# ---- 5. the device-pointer entry points, and a call of two chunks ------------------------------------------------------------
@pytest.mark.parametrize("d,k", [(48, 10), (208, 100)])
def test_dev_entry_points_equal_the_host_forms(pkg, d, k):
    import torch
    n, nq = 300, 70
    rng = np.random.default_rng(50 + d)
    x, q = rng.standard_normal((n, d), dtype=F), rng.standard_normal((nq, d), dtype=F)
    btags = (np.arange(n) % 3).astype(np.uint16)
    qtags = np.array([0, 1, 2, tr.NONE, 7], np.uint16)[np.arange(nq) % 5]
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x)
    g.set_base_tags(np.arange(n, dtype=np.uint32), btags)
    dev = torch.device("cuda", 0)
    wide = np.full((nq, d + 1), np.nan, F)  # an .fvecs image's stride; the header column is never read
    wide[:, 1:] = q
    tw = torch.from_numpy(wide).to(dev)
    tq, tt = torch.from_numpy(q).to(dev), torch.from_numpy(qtags.view(np.int16)).to(dev)
    od, ol = torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def out():
        g.sync()
        res = od.cpu().numpy().copy(), ol.cpu().numpy().copy()
        od.fill_(-1.0)
        ol.fill_(-7)
        torch.cuda.synchronize(dev)
        return res

    for splits in (1, 3):
        g.set_option("exact_splits", splits)
        plain, tagged = g.exact_search_f16(q, k), g.exact_search_f16_tags(q, k, qtags)
        assert (tagged[1][qtags == 7] == -1).all() and not np.array_equal(plain[1], tagged[1])
        g.exact_search_f16_dev(nq, tq, d, k, od, ol)
        _same(out(), plain)
        g.exact_search_f16_dev(nq, tw.data_ptr() + 4, d + 1, k, od, ol)
        _same(out(), plain)
        g.exact_search_f16_tags_dev(nq, tq, d, k, tt, od, ol)
        _same(out(), tagged)
        g.exact_search_f16_tags_dev(nq, tw.data_ptr() + 4, d + 1, k, tt, od, ol)
        _same(out(), tagged)
        g.exact_search_f16_tags_dev(nq, tq, d, k, None, od, ol)  # no tags: the plain call
        _same(out(), plain)
    assert _code(pkg, g.exact_search_f16_dev, nq - 1, tq.data_ptr() + 2, d, k, od, ol) == pkg.ERR_INVALID
    assert _code(pkg, g.exact_search_f16_tags_dev, nq - 1, tq.data_ptr() + 2, d, k, tt, od, ol) == pkg.ERR_INVALID
    assert _code(pkg, g.exact_search_f16_tags_dev, nq - 1, tq, d, k, tt.data_ptr() + 1, od, ol) == pkg.ERR_INVALID
    assert _code(pkg, g.exact_search_f16_dev, nq, tq, d - 1, k, od, ol) == pkg.ERR_INVALID  # row_stride < d
    g.sync()
    g.close()


def test_a_call_of_two_query_chunks(pkg):
    n, d, nq = 33, 16, 16384 + 33
    rng = np.random.default_rng(60)
    x, q = rng.integers(0, 128, (n, d), dtype=np.uint8), rng.integers(0, 128, (nq, d), dtype=np.uint8)
    q[16384 + 5] = x[20]  # a zero distance in the second chunk
    btags = (np.arange(n) % 3).astype(np.uint16)
    qtags = np.array([0, 1, 2, tr.NONE, 7], np.uint16)[np.arange(nq) % 5]
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x.astype(F))
    g.set_base_tags(np.arange(n, dtype=np.uint32), btags)
    g.set_option("exact_splits", 3)
    _same(g.exact_search_f16(q.astype(F), 1), exact_ref.search(x, q, 1))
    _same(g.exact_search_f16_tags(q.astype(F), 1, qtags), tr.search_blocked(x, q, 1, btags, qtags))
    g.close()
