"""Base values on the float16 store (ivfhnsw_gpu_exact_search_f16_values): integer rows against the int64
numpy restatement of the uint8 _values call bit for bit, ties whose rows arrive in descending label, real rows against the
device's own bits with no tolerance, the state and the refusals around them, and the device form over two chunks.  Stores,
values and assignments are tests/exact_values_ref.py's; the bit matrix and its selection tests/exact_f16_ref.py's."""
import itertools

import numpy as np
import pytest

import exact_f16_ref as fr
import exact_values_ref as vr

pytestmark = pytest.mark.gpu

F = np.float32
NQS, DS, KS = (1, 33, 129, 300), (16, 96, 256), (1, 33, 100)


def _same(got, want):
    assert np.array_equal(got[1], want[1]), np.nonzero((got[1] != want[1]).any(1))[0][:5]
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def _code(pkg, f, *a):
    with pytest.raises(pkg.IvfHnswError) as e:
        f(*a)
    return e.value.code


def _store(pkg, rows_f32, bvals):
    g = pkg.GpuIndex(0)
    g.upload_base_f16(rows_f32)
    g.set_base_values(np.arange(len(bvals), dtype=np.uint32), bvals)
    return g


def _grid():
    """(n, d, k, nq, assignment, exact_splits): every (n, d, k) once, the other axes cycling; then every assignment at every nq it fits."""
    cases = []
    for i, (n, d, k) in enumerate(itertools.product((33, vr.BIG_N), DS, KS)):
        a = vr.ASSIGNMENTS[i % len(vr.ASSIGNMENTS)]
        nqs = [q for q in NQS if vr.fits(a, n, q)]
        cases.append((n, d, k, nqs[i % len(nqs)], a, (1, 3)[i % 2]))
    fit = [(a, nq) for a in vr.ASSIGNMENTS for nq in NQS if vr.fits(a, vr.BIG_N, nq)]
    cases += [(vr.BIG_N, DS[i % 3], KS[(i // 2) % 3], nq, a, (1, 3)[(i // 3) % 2]) for i, (a, nq) in enumerate(fit)]
    return sorted(set(cases))


_STORES = {}


@pytest.fixture(scope="module")
def int_store(pkg):
    """(rows u8, values, handle with both installed) per (n, d), made once; bytes halved at d = 256, where 0..255 is not exact."""
    def get(n, d):
        if (n, d) not in _STORES:
            base = vr.make_base(n, d) >> np.uint8(d == 256)
            _STORES[n, d] = base, vr.base_values(n), _store(pkg, base.astype(F), vr.base_values(n))
        return _STORES[n, d]
    yield get
    for _, _, g in _STORES.values():
        g.close()
    _STORES.clear()


# ---- 1. integer rows: every operation exact, so labels and distance bits are the restatement's
@pytest.mark.parametrize("n,d,k,nq,assign,splits", _grid())
def test_integer_rows_equal_the_restatement(int_store, n, d, k, nq, assign, splits):
    base, bvals, g = int_store(n, d)
    q = vr.make_queries(nq, d, vr.make_base(n, d)) >> np.uint8(d == 256)
    qr = vr.assignment(assign, n, nq)
    g.set_option("exact_splits", splits)
    _same(g.exact_search_f16_values(q.astype(F), k, qr), vr.search_blocked(base, q, k, bvals, qr))


# ---- 2. ties against arrival order: 320 identical rows whose values descend with the row number reach the sweep highest
# label first; "zeros": the block and the query are zero, so |q|^2 + |thr| = 0 and the gate has no margin
@pytest.mark.parametrize("k,splits,block", [(k, s, b) for k in KS for s, b in ((1, "helper"), (3, "helper"), (1, "zeros"))])
def test_ties_go_to_the_lower_label(pkg, k, splits, block):
    n, d, nq = vr.BIG_N, 16, 33
    t0, tn = vr.tie_block(n)
    base = vr.make_base(n, d)
    q = vr.make_queries(nq, d, base)
    if block == "zeros":
        base[t0:t0 + tn] = 0
        q[vr.TIE_QUERY] = 0
    bvals = vr.base_values(n)
    qr = np.tile(np.array([(vr.TIE_TOP, vr.TIE_TOP + tn - 1)], np.uint32), (nq, 1))
    g = _store(pkg, base.astype(F), bvals)
    g.set_option("exact_splits", splits)
    dist, lab = g.exact_search_f16_values(q.astype(F), k, qr)
    g.close()
    assert lab[vr.TIE_QUERY].tolist() == list(range(t0, t0 + k)) and (dist[vr.TIE_QUERY] == 0).all()
    _same((dist, lab), vr.search_blocked(base, q, k, bvals, qr))


# ---- 3. real rows: the matrix of the device's own bits (the range search at +inf), selected under every query's mask
@pytest.mark.parametrize("d,k", [(d, k) for d in (96, 208) for k in (1, 100)])
def test_real_rows_select_from_the_bits(pkg, d, k):
    n, nq = 1000, 70
    x, q = fr.offset_rows(10 * d, n, d, 30.0, 0.05), fr.offset_rows(10 * d + 1, nq, d, 30.0, 0.05)
    bvals, qr = vr.base_values(n), vr.assignment("interleaved", n, nq)
    qr[::4] = vr.FULL
    mask = np.stack([vr.value_mask(bvals, lo, hi) for lo, hi in qr])
    g = _store(pkg, x, bvals)
    g.set_option("exact_splits", 3)
    B = fr.matrix_of(*g.exact_range_search_f16(q, np.inf), n)
    got, plain = g.exact_search_f16_values(q, k, qr), g.exact_search_f16(q, k)
    g.close()
    assert not np.isnan(B).any() and np.unique(B).size < B.size // 4  # every pair, many of them tied
    _same(got, fr.topk_of_bits(B, k, mask))
    _same((got[0][::4], got[1][::4]), (plain[0][::4], plain[1][::4]))


# ---- 4. state and refusals
@pytest.mark.parametrize("case", ["none_is_plain", "sets", "view", "reupload", "on_u8", "before_upload", "bad_k", "u8_call", "value_rows"])
def test_state_and_refusals(pkg, case):
    n, d, k, nq = 1000, 32, 10, 40
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
        assert _code(pkg, g.exact_search_f16_values, qf, k, qr) == pkg.ERR_STATE
        g.close()
        return
    g.upload_base_f16(xf)
    before = g.exact_search_f16(qf, k)
    if case == "sets":  # three calls: set, re-value, un-value; and their outcome in one call on a second handle
        calls = [(rows[::2], bvals[::2]), (np.array([4, 6, n + 5, 999], np.uint32), np.array([7, vr.NONE, 1, 77], np.uint32)),
                 (rows[10:400:3], np.full(130, vr.NONE, np.uint32))]
        for c in calls:
            g.set_base_values(*c)
        bvals = vr.apply_sets(n, calls)
        g1 = _store(pkg, xf, bvals)
        assert g.base_values_info() == g1.base_values_info() == (int((bvals != vr.NONE).sum()), n)
        _same(g.exact_search_f16_values(qf, k, qr), g1.exact_search_f16_values(qf, k, qr))
        g1.close()
    else:
        g.set_base_values(rows, bvals)
    if case == "none_is_plain":  # ... and the plain and the tag calls ignore the values
        g.set_base_tags(rows, (rows % 3).astype(np.uint16))
        for got in (g.exact_search_f16(qf, k), g.exact_search_f16_tags(qf, k, np.full(nq, 0xffff, np.uint16)),
                    g.exact_search_f16_values(qf, k, None), g.exact_search_f16_values(qf, k, np.tile(np.array([vr.FULL], np.uint32), (nq, 1)))):
            _same(got, before)
    elif case == "view":
        v = g.view()
        assert _code(pkg, v.set_base_values, rows[:3], bvals[:3]) == pkg.ERR_STATE
        _same(v.exact_search_f16_values(qf, k, qr), vr.search_blocked(base, q, k, bvals, qr))
        v.close()
    elif case == "reupload":
        g.upload_base_f16(xf)
        assert g.base_values_info() == (0, n)
        bvals = np.full(n, vr.NONE, np.uint32)
    elif case == "bad_k":  # ... and a refused call leaves the handle's earlier results readable
        lims, dd, ll = g.exact_range_search_f16(qf, float(np.median(before[0])))
        assert len(dd) > 0
        assert _code(pkg, g.exact_search_f16_values, qf, 0, qr) == _code(pkg, g.exact_search_f16_values, qf, 101, qr) == pkg.ERR_INVALID
        d2, l2 = g.exact_range_results(0, len(dd))
        assert np.array_equal(l2, ll) and np.array_equal(d2.view(np.uint32), dd.view(np.uint32))
    elif case == "u8_call":
        assert _code(pkg, g.exact_search_values, q, k, qr) == pkg.ERR_STATE
    elif case == "value_rows":
        for lo, hi in itertools.product(vr.EDGES, vr.EDGES):
            assert g.base_value_rows(lo, hi) == int(vr.value_mask(bvals, lo, hi).sum()), (lo, hi)
    _same(g.exact_search_f16_values(qf, k, qr), vr.search_blocked(base, q, k, bvals, qr))
    g.close()


# ---- 5. the device form: strided queries, an aligned ranges tensor; the second case is cut into two chunks of 5120 queries
# (64 splits at k = 100: sweep_value_chunk)
@pytest.mark.parametrize("n,d,k,nq,splits", [(vr.BIG_N, 48, 10, 300, 3), (33, 16, 100, 5120 + 45, 64)])
def test_dev_form_equals_the_restatement(pkg, n, d, k, nq, splits):
    import torch
    base = vr.make_base(n, d)
    q = vr.make_queries(nq, d, base)
    bvals, qr = vr.base_values(n), vr.assignment("interleaved", n, nq)
    g = _store(pkg, base.astype(F), bvals)
    g.set_option("exact_splits", splits)
    dev = torch.device("cuda", 0)
    wide = np.full((nq, d + 1), np.nan, F)  # an .fvecs image's stride; the header column is never read
    wide[:, 1:] = q
    tw, tr = torch.from_numpy(wide).to(dev), torch.from_numpy(qr.view(np.int32)).to(dev)
    od, ol = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev), torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    assert tr.data_ptr() % 8 == 0
    g.exact_search_f16_values_dev(nq, tw.data_ptr() + 4, d + 1, k, tr, od, ol)
    g.sync()
    _same((od.cpu().numpy(), ol.cpu().numpy()), vr.search_blocked(base, q, k, bvals, qr))
    assert _code(pkg, g.exact_search_f16_values_dev, nq - 1, tw.data_ptr() + 4, d + 1, k, tr.data_ptr() + 4, od, ol) == pkg.ERR_INVALID
    g.close()
