"""Exact range search of the float16 store under an interval of base values per query
(ivfhnsw_gpu_exact_range_search_f16_values): integer rows bit for bit against the restatement of the uint8
_values call, the window skip and the tile map together on sparse hits, label order where rows arrive in descending label,
real rows against the device's own bits with no tolerance, the state and the refusals, and the device form over two chunks.
Stores, values and assignments are tests/exact_values_ref.py's; the bit matrix and its cut tests/exact_f16_ref.py's."""
import itertools

import numpy as np
import pytest

import exact_f16_ref as fr
import exact_ref
import exact_values_ref as vr

pytestmark = pytest.mark.gpu

F = np.float32
NQS, DS = (1, 33, 129, 300), (16, 96, 256)
# (n, d, nq, assignment, exact_splits, exact_range_map): every (n, d) once with the other axes cycling, then every assignment
# at every nq it fits on the 6001-row store
GRID = []
for i, (n, d) in enumerate(itertools.product((33, vr.BIG_N), DS)):
    a = vr.ASSIGNMENTS[(3 * i) % len(vr.ASSIGNMENTS)]
    nqs = [q for q in NQS if vr.fits(a, n, q)]
    GRID.append((n, d, nqs[i % len(nqs)], a, (1, 3)[i % 2], (1, 0)[(i // 2) % 2]))
GRID += [(vr.BIG_N, DS[i % 3], nq, a, (1, 3)[(i // 3) % 2], (1, 0)[(i // 2) % 2])
         for i, (a, nq) in enumerate((a, nq) for a in vr.ASSIGNMENTS for nq in NQS if vr.fits(a, vr.BIG_N, nq))]
GRID = sorted(set(GRID))

_STORES = {}


@pytest.fixture(scope="module")
def int_store(pkg):
    """(rows u8, values, handle with both installed) per (n, d), made once; bytes halved at d = 256, where 0..255 is not exact."""
    def get(n, d):
        if (n, d) not in _STORES:
            base = vr.make_base(n, d) >> np.uint8(d == 256)
            g = pkg.GpuIndex(0)
            g.upload_base_f16(base.astype(F))
            g.set_base_values(np.arange(n, dtype=np.uint32), vr.base_values(n))
            _STORES[n, d] = base, vr.base_values(n), g
        return _STORES[n, d]
    yield get
    for _, _, g in _STORES.values():
        g.close()
    _STORES.clear()


# ---- 1. integer rows: every operation exact, so lims, labels and distance bits are the restatement's
@pytest.mark.parametrize("n,d,nq,assign,splits,use_map", GRID)
def test_integer_rows_equal_the_restatement(int_store, n, d, nq, assign, splits, use_map):
    base, bvals, g = int_store(n, d)
    q = vr.make_queries(nq, d, vr.make_base(n, d)) >> np.uint8(d == 256)
    qr = vr.assignment(assign, n, nq)
    g.set_option("exact_splits", splits)
    g.set_option("exact_range_map", use_map)
    mask = np.stack([vr.value_mask(bvals, lo, hi) for lo, hi in qr])
    windowed = mask.any(1) & ~mask.all(1)
    # a radius ON a pair's distance: the median over the queries with a window of the 10th-smallest in-window distance
    D = exact_ref.distances(base, q)
    tenth = np.sort([np.sort(D[i][mask[i]])[:10][-1] for i in np.flatnonzero(mask.any(1))])
    on = float(tenth[tenth.size // 2]) if tenth.size else 1.0
    for radius in (0.0, on, on + 0.5) + ((np.inf,) if n == 33 else ()):
        want = vr.range_blocked(base, q, radius, bvals, qr)
        hits = np.diff(want[0].astype(np.int64))
        if radius == 0.0 or not mask.any():
            assert want[0][-1] == 0
        elif windowed.any() and radius > on:  # no case passes on empty results, and strict '<' dropped the pair ON `on`
            assert hits[windowed].any() and hits.sum() > (D[mask] < on).sum()
        got = g.exact_range_search_f16_values(q.astype(F), radius, qr)
        assert np.array_equal(got[0], want[0]), (radius, np.nonzero(got[0] != want[0])[0][:5])
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), radius


# ---- 2. the two skips compose: windows at the two ends of the value order or of one row each, hits in a few tiles only;
# under 64 splits most splits of a span are empty
@pytest.mark.parametrize("assign,splits", [("gap", 3), ("single", 3), ("gap", 64), ("single", 64)])
def test_sparse_hits_with_and_without_the_map(pkg, assign, splits):
    rng = np.random.default_rng(5)
    n, nq, d = vr.BIG_N, 129, 96
    x = rng.integers(100, 128, (n, d), dtype=np.uint8)
    q = rng.integers(0, 4, (nq, d), dtype=np.uint8)
    bvals, qr = vr.base_values(n), vr.assignment(assign, n, nq)
    mask = np.stack([vr.value_mask(bvals, lo, hi) for lo, hi in qr])
    for qi in range(0, nq, 9):  # a near row at the start, the middle and the end of the query's window, and one outside it
        rows = np.flatnonzero(mask[qi])
        for row in {rows[qi % rows.size], rows[(rows.size // 2 + qi) % rows.size], rows[-1 - qi % rows.size], np.flatnonzero(~mask[qi])[qi]}:
            x[row] = q[qi]
            x[row, 0] += 2
    want = vr.range_blocked(x, q, 50.0, bvals, qr)
    assert 0 < want[0][-1] <= 3 * nq
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x.astype(F))
    g.set_base_values(np.arange(n, dtype=np.uint32), bvals)
    g.set_option("exact_splits", splits)
    for use_map in (1, 0):  # (both equal the restatement, so each other)
        g.set_option("exact_range_map", use_map)
        got = g.exact_range_search_f16_values(q.astype(F), 50.0, qr)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    g.close()


# ---- 3. order: the tie block's values descend with the row number, so its rows reach the sweep highest label first
@pytest.mark.parametrize("splits", [1, 3])
def test_labels_ascend_where_rows_arrive_descending(int_store, splits):
    n, d, nq = vr.BIG_N, 16, 33
    base, bvals, g = int_store(n, d)
    t0, tn = vr.tie_block(n)
    q = vr.make_queries(nq, d, vr.make_base(n, d))
    qr = np.tile(np.array([(vr.TIE_TOP, vr.TIE_TOP + tn - 1)], np.uint32), (nq, 1))
    g.set_option("exact_splits", splits)
    g.set_option("exact_range_map", 1)
    lims, dist, lab = g.exact_range_search_f16_values(q.astype(F), np.inf, qr)
    assert np.array_equal(lims, np.arange(nq + 1, dtype=np.uint64) * np.uint64(tn))
    assert np.array_equal(lab.reshape(nq, tn), np.tile(np.arange(t0, t0 + tn), (nq, 1))) and (dist.reshape(nq, tn)[vr.TIE_QUERY] == 0).all()


# ---- 4. real rows: the matrix of the device's own bits (the plain range search at +inf), cut under every query's mask
@pytest.mark.parametrize("d", [96, 208])
def test_real_rows_cut_from_the_bits(pkg, d):
    n, nq = 1000, 70
    x, q = fr.offset_rows(10 * d, n, d, 30.0, 0.05), fr.offset_rows(10 * d + 1, nq, d, 30.0, 0.05)
    bvals, qr = vr.base_values(n), vr.assignment("interleaved", n, nq)
    qr[::4] = vr.FULL
    mask = np.stack([vr.value_mask(bvals, lo, hi) for lo, hi in qr])
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x)
    g.set_base_values(np.arange(n, dtype=np.uint32), bvals)
    g.set_option("exact_splits", 3)
    B = fr.matrix_of(*g.exact_range_search_f16(q, np.inf), n)
    assert not np.isnan(B).any()
    radius = float(np.median(B[mask]))
    lims, dist, lab = g.exact_range_search_f16_values(q, radius, qr)
    want = fr.range_of_bits(B, radius, mask)
    assert 0 < want[0][-1] < mask.sum() and np.array_equal(lims, want[0]) and np.array_equal(lab, want[2])
    assert np.array_equal(dist.view(np.uint32), want[1].view(np.uint32))
    plain = g.exact_range_search_f16(q[::4], radius)  # FULL queries run the staged arithmetic of the plain call
    sel = np.repeat(np.arange(nq) % 4 == 0, np.diff(lims).astype(np.int64))
    assert np.array_equal(np.diff(lims)[::4], np.diff(plain[0])) and np.array_equal(lab[sel], plain[2]) and np.array_equal(dist[sel].view(np.uint32), plain[1].view(np.uint32))
    # ... and the k-search under the same intervals, cut at the radius where it holds fewer than k hits
    k = min(n, 100)
    kd, kl = g.exact_search_f16_values(q, k, qr)
    g.close()
    for i in range(nq):
        keep = (kl[i] >= 0) & (kd[i] < F(radius))
        if keep.sum() < k:
            order = np.argsort(kl[i][keep])
            a, b = int(lims[i]), int(lims[i + 1])
            assert np.array_equal(lab[a:b], kl[i][keep][order]) and np.array_equal(dist[a:b].view(np.uint32), kd[i][keep][order].view(np.uint32))


# ---- 5. state and refusals
@pytest.mark.parametrize("case", ["none_is_plain", "view", "reupload", "on_u8", "before_upload", "nan", "u8_call", "tags_ignored"])
def test_state_and_refusals(pkg, case):
    n, d, nq, radius = 1000, 32, 40, 250000.0
    base = vr.make_base(n, d)  # (bytes are exact at d = 32)
    q = vr.make_queries(nq, d, base)
    xf, qf = base.astype(F), q.astype(F)
    bvals, qr = vr.base_values(n), vr.assignment("absent", n, nq)
    rows = np.arange(n, dtype=np.uint32)
    g = pkg.GpuIndex(0)
    if case in ("on_u8", "before_upload"):
        if case == "on_u8":
            g.upload_base(base)
            g.set_base_values(rows, bvals)
        with pytest.raises(pkg.IvfHnswError) as e:
            g.exact_range_search_f16_values(qf, radius, qr)
        assert e.value.code == pkg.ERR_STATE
        g.close()
        return
    g.upload_base_f16(xf)
    g.set_base_values(rows, bvals)
    if case == "reupload":  # first == 0 drops the values: every row is valueless
        g.upload_base_f16(xf)
        bvals = np.full(n, vr.NONE, np.uint32)
    elif case == "tags_ignored":
        g.set_base_tags(rows, (rows % 3).astype(np.uint16))
    want = vr.range_blocked(base, q, radius, bvals, qr)
    assert want[0][-1] > 0
    v = g.view() if case == "view" else g
    got = v.exact_range_search_f16_values(qf, radius, qr)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    if case == "none_is_plain":
        plain = g.exact_range_search_f16(qf, radius)
        for other in (g.exact_range_search_f16_values(qf, radius, None),
                      g.exact_range_search_f16_values(qf, radius, np.tile(np.array([vr.FULL], np.uint32), (nq, 1)))):
            assert all(np.array_equal(a, b) for a, b in zip(other, plain))
    elif case in ("nan", "u8_call"):  # a refused call leaves the earlier results readable
        with pytest.raises(pkg.IvfHnswError) as e:
            g.exact_range_search_f16_values(qf, np.nan, qr) if case == "nan" else g.exact_range_search_values(q, radius, qr)
        assert e.value.code == (pkg.ERR_INVALID if case == "nan" else pkg.ERR_STATE)
        held = g.exact_range_results(0, int(want[0][-1]))
        assert np.array_equal(held[1], want[2]) and np.array_equal(held[0].view(np.uint32), want[1].view(np.uint32))
    if v is not g:
        v.close()
    g.close()


# ---- 6. the device form: strided queries, an aligned ranges tensor; the second case is two chunks (16 384 + 33 queries),
# each with its own plan and its own strips of the tile map
@pytest.mark.parametrize("n,d,nq,splits", [(vr.BIG_N, 48, 300, 3), (33, 16, 16384 + 33, 3)])
def test_dev_form_equals_the_restatement(pkg, n, d, nq, splits):
    import torch
    base = vr.make_base(n, d)
    q = vr.make_queries(nq, d, base)
    bvals, qr = vr.base_values(n), vr.assignment("interleaved", n, nq)
    radius = float(np.median(exact_ref.distances(base, q[:64]))) + 0.5
    want = vr.range_blocked(base, q, radius, bvals, qr)
    assert want[0][-1] > 0
    g = pkg.GpuIndex(0)
    g.upload_base_f16(base.astype(F))
    g.set_base_values(np.arange(n, dtype=np.uint32), bvals)
    g.set_option("exact_splits", splits)
    dev = torch.device("cuda", 0)
    wide = np.full((nq, d + 1), np.nan, F)  # an .fvecs image's stride; the header column is never read
    wide[:, 1:] = q
    tw, tr = torch.from_numpy(wide).to(dev), torch.from_numpy(qr.view(np.int32)).to(dev)
    tl = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    assert tr.data_ptr() % 8 == 0 and g.exact_range_search_f16_values_dev(nq, tw.data_ptr() + 4, d + 1, tr, radius, tl) == want[0][-1]
    assert np.array_equal(tl.cpu().numpy().view(np.uint64), want[0])
    dist, lab = g.exact_range_results(0, int(want[0][-1]))
    assert np.array_equal(lab, want[2]) and np.array_equal(dist.view(np.uint32), want[1].view(np.uint32))
    with pytest.raises(pkg.IvfHnswError) as e:
        g.exact_range_search_f16_values_dev(nq - 1, tw.data_ptr() + 4, d + 1, tr.data_ptr() + 4, radius, tl)
    assert e.value.code == pkg.ERR_INVALID
    g.close()
