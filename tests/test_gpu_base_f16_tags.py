"""Base tags on the float16 store (ivfhnsw_gpu_exact_search_f16_tags): integer rows against the int64 numpy
restatement of the uint8 _tags call bit for bit, real rows against float64 within the bound of 3.27, and the state and the
refusals around them.  Shapes, tags and assignments are tests/exact_tags_ref.py's."""
import itertools

import numpy as np
import pytest

import exact_ref
import exact_tags_ref as tr

pytestmark = pytest.mark.gpu

F = np.float32
NQS, DS, KS = (1, 33, 129, 300), (16, 96, 256), (1, 33, 100)


def _same(got, want):
    assert np.array_equal(got[1], want[1]), np.nonzero((got[1] != want[1]).any(1))[0][:5]
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def _grid():
    """(n, d, k, nq, assignment, exact_splits), the axes cycling as exact_tags_ref.grid() cycles them, plus the corners: Dense
    ranges of 5 and 2 strips under both workgroup widths, a 4-row tag under 3 splits, one query per tag on the 33-row store."""
    names = ("none", "each", "sizes", "g129", "absent")
    cases = []
    for i, (n, d, k) in enumerate(itertools.product(tr.NS, DS, KS)):
        a = names[i % len(names)]
        nqs = [q for q in NQS if tr.fits(a, n, q)]
        cases.append((n, d, k, nqs[i % len(nqs)], a, (1, 3)[i % 2]))
    i = 0
    for a in names + ("many",):
        for nq in NQS:
            if tr.fits(a, tr.MANY_N, nq):
                cases.append((tr.MANY_N, DS[i % 3], KS[(i // 2) % 3], nq, a, (1, 3)[(i // 3) % 2]))
                i += 1
    cases += [(tr.MANY_N, 96, 100, 129, "none", 3), (tr.MANY_N, 256, 1, 129, "sizes", 1), (tr.MANY_N, 16, 33, 300, "many", 3),
              (tr.MANY_N, 96, 100, 300, "many", 3), (33, 16, 1, 33, "each", 3)]
    return sorted(set(cases))


_STORES = {}


@pytest.fixture(scope="module")
def int_store(pkg):
    """(rows u8, tags, handle with both installed) per (n, d), made once; values 0..127 at d = 256, where bytes are not exact."""
    def get(n, d):
        if (n, d) not in _STORES:
            base = tr.make_base(n, d) >> np.uint8(d == 256)
            g = pkg.GpuIndex(0)
            g.upload_base_f16(base.astype(F))
            g.set_base_tags(np.arange(n, dtype=np.uint32), tr.base_tags(n))
            _STORES[n, d] = base, tr.base_tags(n), g
        return _STORES[n, d]
    yield get
    for _, _, g in _STORES.values():
        g.close()
    _STORES.clear()


# ---- 1. integer rows: every operation exact, so labels and distance bits are the restatement's
@pytest.mark.parametrize("n,d,k,nq,assign,splits", _grid())
def test_integer_rows_equal_the_restatement(int_store, n, d, k, nq, assign, splits):
    base, btags, g = int_store(n, d)
    q = tr.make_queries(nq, d, tr.make_base(n, d)) >> np.uint8(d == 256)
    qtags = tr.assignment(assign, n, nq)
    g.set_option("exact_splits", splits)
    _same(g.exact_search_f16_tags(q.astype(F), k, qtags), tr.search_blocked(base, q, k, btags, qtags))


# ---- 2. real rows against float64 on the rounded operands, each query restricted to its tag's rows
@pytest.mark.parametrize("d,k", [(96, 1), (96, 100), (256, 1), (256, 100)])
def test_real_rows_within_the_bound_of_float64(pkg, d, k):
    n, nq = 4133, 129
    rng = np.random.default_rng(d)
    x, q = rng.standard_normal((n, d), dtype=F), rng.standard_normal((nq, d), dtype=F)
    btags, qtags = tr.base_tags(n), tr.assignment("interleaved", n, nq)
    qtags[::4] = tr.NONE  # (this store has some 400 tags: the draw alone leaves no query untagged, and two Dense strips are wanted)
    xh, qh = x.astype(np.float16).astype(np.float64), q.astype(np.float16).astype(np.float64)
    xn, qn = (xh * xh).sum(1), (qh * qh).sum(1)
    D = qn[:, None] + xn[None, :] - 2.0 * (qh @ xh.T)
    tol = (d + 3) * 2.0 ** -23 * (np.sqrt(qn)[:, None] + np.sqrt(xn)[None, :]) ** 2
    mine = np.stack([tr.tag_mask(btags, t) for t in qtags])
    D = np.where(mine, D, np.inf)
    g = pkg.GpuIndex(0)
    g.upload_base_f16(x)
    g.set_base_tags(np.arange(n, dtype=np.uint32), btags)
    dist, lab = g.exact_search_f16_tags(q, k, qtags)
    plain = g.exact_search_f16(q, k)
    g.close()
    found = lab >= 0
    assert np.array_equal(found.sum(1), np.minimum(k, mine.sum(1))) and (found[:, :-1] >= found[:, 1:]).all()
    assert (np.diff(dist, axis=1) >= 0).all() and (dist[~found] == exact_ref.FLT_MAX).all()
    rows = np.broadcast_to(np.arange(nq)[:, None], lab.shape)[found]
    cols = lab[found]
    err = np.abs(dist[found].astype(np.float64) - D[rows, cols])  # (a row outside the query's tag: inf, and fails)
    print("d %d k %d: largest |returned - float64| / tol = %.4f" % (d, k, (err / tol[rows, cols]).max()))
    assert (err <= tol[rows, cols]).all()
    Dk = np.sort(D, axis=1)[:, k - 1:k]  # inf where the tag has fewer than k rows: then every row of it is returned
    assert (D[rows, cols] <= (Dk + 2 * tol)[rows, cols]).all()
    returned = np.zeros(D.shape, bool)
    returned[rows, cols] = True
    assert returned[D < Dk - 2 * tol].all()
    # the untagged queries run the staged arithmetic of the plain call
    none = qtags == tr.NONE
    assert none.sum() > 32
    _same((dist[none], lab[none]), (plain[0][none], plain[1][none]))


# ---- 3. state and refusals
@pytest.mark.parametrize("case", ["state", "none_is_plain", "on_u8", "before_upload", "view", "reupload_drops_tags", "incremental"])
def test_state_and_refusals(pkg, case):
    n, d, k, nq = 1000, 32, 10, 40
    base = tr.make_base(n, d)  # (bytes are exact at d = 32)
    q = tr.make_queries(nq, d, base)
    xf, qf = base.astype(F), q.astype(F)
    btags, qtags = tr.base_tags(n), tr.assignment("absent", n, nq)
    rows = np.arange(n, dtype=np.uint32)
    g = pkg.GpuIndex(0)
    if case in ("on_u8", "before_upload"):
        if case == "on_u8":
            g.upload_base(base)
            g.set_base_tags(rows, btags)
        with pytest.raises(pkg.IvfHnswError) as e:
            g.exact_search_f16_tags(qf, k, qtags)
        assert e.value.code == pkg.ERR_STATE
        g.close()
        return
    g.upload_base_f16(xf)
    before = g.exact_search_f16(qf, k)
    g.set_base_tags(rows, btags)
    if case == "state":
        assert g.base_tags_info() == (int((btags != tr.NONE).sum()), n, tr.tags_in_use(btags).size)
        for t in (tr.BIG, tr.FEW, tr.ONE, tr.NONE, tr.ABSENT[0]):
            assert g.base_tag_rows(t) == int((btags == t).sum())
        _same(g.exact_search_f16(qf, k), before)  # the plain call ignores the tags
        g.clear_base_tags()
        assert g.base_tags_info() == (0, n, 0)
    elif case == "none_is_plain":
        _same(g.exact_search_f16_tags(qf, k, None), before)
        _same(g.exact_search_f16_tags(qf, k, np.full(nq, tr.NONE, np.uint16)), before)
    elif case == "view":
        v = g.view()
        _same(v.exact_search_f16_tags(qf, k, qtags), tr.search_blocked(base, q, k, btags, qtags))
        v.close()
    elif case == "reupload_drops_tags":
        g.upload_base_f16(xf)
        assert g.base_tags_info() == (0, n, 0)
        qt = np.where(qtags == tr.NONE, tr.NONE, tr.BIG).astype(np.uint16)
        _same(g.exact_search_f16_tags(qf, k, qt), tr.search_blocked(base, q, k, np.full(n, tr.NONE, np.uint16), qt))
    elif case == "incremental":
        calls = [(np.array([2, 0, 999, n + 5], np.uint32), np.array([tr.ONE, tr.NONE, tr.FEW, 1], np.uint16))]
        g.set_base_tags(*calls[0])
        btags = tr.apply_sets(n, calls, btags)
        qt = np.array([tr.ONE, tr.BIG, tr.NONE, tr.FEW], np.uint16)[np.arange(nq) % 4]
        _same(g.exact_search_f16_tags(qf, k, qt), tr.search_blocked(base, q, k, btags, qt))
    if case not in ("state", "reupload_drops_tags"):
        _same(g.exact_search_f16_tags(qf, k, qtags), tr.search_blocked(base, q, k, btags, qtags))
    g.close()
