"""Reconstruction of stored vectors on the device (ivfhnsw_gpu_locate / reconstruct_rows / reconstruct /
search_reconstruct).

ROTATED-space vectors are compared bit for bit with tests/recon_ref.py (every step of the contract is one float32
operation); ORIGINAL space with numpy where the product is exact (a signed permutation) and with ivfhnsw_gpu_rotate_dev
on a handle holding the transposed matrix otherwise; locate with numpy over the uploaded ids; search_reconstruct with
search() and reconstruct_rows()."""
import numpy as np
import pytest
import torch

from conftest import corpus
import recon_ref
from recon_ref import bits
from test_gpu_remove import BASE, _upload, _same_search, _with_ids

pytestmark = pytest.mark.gpu

NPROBE, MAX_CODES, EF = 16, 2000, 40
FLT_MAX = np.finfo(np.float32).max
OPQ = dict(seed=81, nc=128, d=96, M=12, n_base=9000, nq=48, efConstruction=60, opq=True)
GROUPING = dict(seed=43, nc=256, d=96, M=16, n_base=20000, nq=64, nsubc=8)      # dsub 6: the scalar form of the kernel
GROUPING_OPQ = dict(seed=87, nc=128, d=96, M=12, n_base=9000, nq=48, efConstruction=60, nsubc=8, opq=True)
CASES = {"M8": dict(BASE, M=8), "M16": BASE, "M32": dict(BASE, M=32), "opq": OPQ, "grouping": GROUPING,
         "grouping-opq": GROUPING_OPQ}
CHUNK = 1 << 18  # rows of one internal chunk (capi_recon.cpp)

_REF = {}


def ref_rotated(name):
    """All rows of a case in ROTATED space, computed once."""
    if name not in _REF:
        _REF[name] = recon_ref.recon_rotated(corpus(**CASES[name]))
        _REF[name].setflags(write=False)
    return _REF[name]


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def is_empty(a):
    return (bits(a) == recon_ref.EMPTY_BITS).all()


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()   # a copy: cached references are read-only


# ---- 1. rows, ROTATED space ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_rows_rotated(gpu, pkg, name):
    c = corpus(**CASES[name])
    ref = ref_rotated(name)
    n = len(c["ids"])
    g = _upload(gpu(), c)
    # every row in one call
    assert same(g.reconstruct_rows(np.arange(n), pkg.RECON_ROTATED), ref)
    # a permutation with empty slots mixed in
    rng = np.random.default_rng(5)
    rows = rng.choice(n, 5000, replace=False).astype(np.int64)
    rows[rng.random(5000) < 0.1] = -1
    got = g.reconstruct_rows(rows, pkg.RECON_ROTATED)
    assert same(got, recon_ref.recon_rotated(c, rows))
    assert is_empty(got[rows < 0]) and (rows < 0).sum() > 100
    # one list: the largest and an empty one
    off = c["offsets"].astype(np.int64)
    big = int(np.argmax(np.diff(off)))
    assert same(g.reconstruct_list(big, pkg.RECON_ROTATED), ref[off[big]:off[big + 1]])
    empty = np.nonzero(np.diff(off) == 0)[0]
    assert len(empty), "the corpus has no empty list"
    assert g.reconstruct_list(int(empty[0]), pkg.RECON_ROTATED).shape == (0, c["d"])
    # the device form: the same bits, and a row outside [0, n_local) is an empty slot
    rows_d = np.concatenate([rows[:1000], [n, n + 7, -5, 1 << 40]]).astype(np.int64)
    out = torch.empty((len(rows_d), c["d"]), dtype=torch.float32, device="cuda")
    g.reconstruct_rows_dev(len(rows_d), dev(rows_d), out, pkg.RECON_ROTATED)
    g.sync()
    out = out.cpu().numpy()
    assert same(out[:1000], got[:1000]) and is_empty(out[1000:])
    if c["opq_A"] is None:
        assert same(g.reconstruct_rows(rows, pkg.RECON_ORIGINAL), got)


def test_rows_cross_the_chunk(gpu, pkg):
    """More rows than one internal chunk, host form, OPQ and ORIGINAL space (the staged path): every output row equals
    the row's vector of a call that fits one chunk."""
    c = corpus(**OPQ)
    n = len(c["ids"])
    g = _upload(gpu(), c)
    one = g.reconstruct_rows(np.arange(n), pkg.RECON_ORIGINAL)
    rng = np.random.default_rng(9)
    rows = rng.integers(0, n, CHUNK + 1000).astype(np.int64)
    rows[[0, CHUNK - 1, CHUNK, CHUNK + 999]] = -1
    rows[[1, CHUNK + 1]] = n - 1
    got = g.reconstruct_rows(rows, pkg.RECON_ORIGINAL)
    want = one[np.where(rows < 0, 0, rows)]
    want.view(np.uint32)[rows < 0] = recon_ref.EMPTY_BITS
    assert same(got, want)


# ---- 2. ORIGINAL space -----------------------------------------------------------------------------------------------
def test_original_signed_permutation(gpu, pkg):
    """x = y A with A a signed permutation: every sum has one non-zero term, so numpy's product is exact."""
    c0 = corpus(**OPQ)
    d = c0["d"]
    rng = np.random.default_rng(3)
    A = np.zeros((d, d), np.float32)
    A[np.arange(d), rng.permutation(d)] = rng.choice([-1.0, 1.0], d)
    g = _upload(gpu(), dict(c0, opq_A=A))
    y = ref_rotated("opq")
    rows = np.arange(len(y))
    assert same(g.reconstruct_rows(rows, pkg.RECON_ROTATED), y)
    got = g.reconstruct_rows(rows, pkg.RECON_ORIGINAL)
    want = (y.astype(np.float64) @ A.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got, want)   # values: -0.0 + 0.0 terms may differ in the sign of a zero only
    rows[::7] = -1
    assert is_empty(g.reconstruct_rows(rows, pkg.RECON_ORIGINAL)[::7])


@pytest.mark.parametrize("name", ["opq", "grouping-opq"])
def test_original_random_rotation(gpu, pkg, name):
    c = corpus(**CASES[name])
    A = c["opq_A"]
    y = ref_rotated(name)
    n, d = y.shape
    g = _upload(gpu(), c)
    got = g.reconstruct_rows(np.arange(n), pkg.RECON_ORIGINAL)
    # a second handle whose opq_A is the transpose: its rotation of y is x = A^T y in the pinned fmaf order
    t = _upload(gpu(), dict(c, opq_A=np.ascontiguousarray(A.T)), graph=False, grouping=False)
    out = torch.empty((n, d), dtype=torch.float32, device="cuda")
    t.rotate_dev(n, dev(y), out)
    t.sync()
    rot = out.cpu().numpy()
    assert same(got, rot)
    # against the float64 product; the bound is rotate_dev's own deviation (it predates this code and is pinned to the
    # oracle) with a factor 2 for the corpus-to-corpus spread of a d-term float32 sum
    exact = y.astype(np.float64) @ A.astype(np.float64)
    tol = 2.0 * np.abs(rot - exact).max()
    err = np.abs(got - exact).max()
    print("ORIGINAL space, %s: max |x - y A (float64)| = %.3e, bound %.3e, max |x| = %.1f" % (name, err, tol, np.abs(exact).max()))
    assert err <= tol


# ---- 3. locate -------------------------------------------------------------------------------------------------------
def first_rows(ids, labels):
    """(lowest row bearing each label or -1, rows bearing it) by numpy."""
    order = np.argsort(ids, kind="stable")
    s = ids[order]
    a = np.searchsorted(s, labels, side="left")
    b = np.searchsorted(s, labels, side="right")
    rows = np.where(b > a, order[np.minimum(a, len(ids) - 1)], -1).astype(np.int64)
    return rows, (b - a).astype(np.uint32)


def check_locate(g, ids, labels):
    labels = np.asarray(labels, np.uint32)
    rows, counts = g.locate(labels)
    want = first_rows(ids, labels)
    assert np.array_equal(rows, want[0]) and np.array_equal(counts, want[1])
    # the device form
    d_rows = torch.full((len(labels),), -7, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((len(labels),), 77, dtype=torch.int32, device="cuda")
    g.locate_dev(len(labels), dev(labels.view(np.int32)), d_rows, d_cnt)
    assert np.array_equal(d_rows.cpu().numpy(), rows)
    assert np.array_equal(d_cnt.cpu().numpy().view(np.uint32), counts)
    return rows, counts


def test_locate_unique_ids(gpu):
    c = corpus(**BASE)
    g = _upload(gpu(), c, graph=False)
    ids = c["ids"]
    rows, counts = check_locate(g, ids, np.arange(len(ids)))
    assert np.array_equal(rows, np.argsort(ids, kind="stable")) and (counts == 1).all()
    # absent labels, labels repeated in the request, a single label
    req = np.array([5, len(ids) + 3, 5, 0xfffffffe, 0, 5, 17, len(ids) + 3], np.uint32)
    rows, counts = check_locate(g, ids, req)
    assert rows[0] == rows[2] == rows[5] >= 0 and rows[1] == rows[7] == -1 and counts[1] == 0
    check_locate(g, ids, [123])
    # n = 0 does nothing
    r0, c0 = g.locate(np.zeros(0, np.uint32))
    assert r0.shape == (0,) and c0.shape == (0,)
    g.locate_dev(0, None, None, None)


def test_locate_repeated_ids_and_largest_label(gpu):
    c0 = corpus(**BASE)
    ids = (c0["ids"] % 1000).astype(np.uint32)
    ids[[3, 17000, 29999]] = 0xffffffff
    g = _upload(gpu(), _with_ids(c0, ids), graph=False)
    req = np.concatenate([np.arange(1200), [0xffffffff, 0xfffffffe, 999, 999]]).astype(np.uint32)
    rows, counts = check_locate(g, ids, req)
    assert np.array_equal(counts[:1000], np.bincount(ids[ids < 1000], minlength=1000))
    assert (rows[1000:1200] == -1).all() and (counts[1000:1200] == 0).all()
    assert rows[1200] == 3 and counts[1200] == 3 and rows[1201] == -1


def test_locate_follows_updates(gpu):
    c = corpus(**BASE)
    g = _upload(gpu(), c, graph=False)
    rng = np.random.default_rng(1)
    m = 500
    g.append_ivf(rng.integers(0, c["nc"], m).astype(np.uint32), np.arange(40000, 40000 + m, dtype=np.uint32),
                 rng.integers(0, 256, (m, c["code_size"])).astype(np.uint8), rng.integers(0, 256, m).astype(np.uint8))
    req = np.concatenate([np.arange(0, 30000, 7), np.arange(39990, 40600)]).astype(np.uint32)
    check_locate(g, g.download_ivf()[1], req)
    g.remove_ids(np.arange(0, 30000, 3).astype(np.uint32))
    off, ids, codes, ncodes = g.download_ivf()
    rows, counts = check_locate(g, ids, req)
    f = gpu()
    f.upload_ivf(c["d"], c["code_size"], off, ids, codes, ncodes, c["centroid_norms"], c["pq_centroids"], c["norm_table"])
    r2, c2 = f.locate(req)
    assert np.array_equal(rows, r2) and np.array_equal(counts, c2)


# ---- 4. by label -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["M16", "grouping-opq"])
def test_reconstruct_by_label(gpu, pkg, name):
    c0 = corpus(**CASES[name])
    ids = (c0["ids"] % 5000).astype(np.uint32)
    c = _with_ids(c0, ids)
    g = _upload(gpu(), c)
    req = np.array([0, 4999, 5000, 77, 77, 0xffffffff, 1234, 600000], np.uint32)
    for space in (pkg.RECON_ROTATED, pkg.RECON_ORIGINAL):
        got, missing = g.reconstruct(req, space)
        rows, _ = g.locate(req)
        assert same(got, g.reconstruct_rows(rows, space))
        assert missing == 3 and is_empty(got[[2, 5, 7]]) and not np.isnan(got[[0, 1, 3, 4, 6]]).any()
        out = torch.empty((len(req), c["d"]), dtype=torch.float32, device="cuda")
        assert g.reconstruct_dev(len(req), dev(req.view(np.int32)), out, space) == 3
        assert same(out.cpu().numpy(), got)
    assert same(g.reconstruct(req, pkg.RECON_ROTATED)[0][[0, 1]], ref_rotated(name)[first_rows(ids, req[:2])[0]])
    assert g.reconstruct(np.zeros(0, np.uint32))[1] == 0


# ---- 5. search and reconstruct ---------------------------------------------------------------------------------------
def tiled(q, n):
    return np.ascontiguousarray(np.tile(q, ((n + len(q) - 1) // len(q), 1))[:n])


def check_search(g, c, q, k, heap, pruning):
    kw = dict(efSearch=EF, do_pruning=pruning, heap_order=heap)
    ref = g.search(q, k, NPROBE, MAX_CODES, **kw)
    dist, lab, rows, rec = g.search_reconstruct(q, k, NPROBE, MAX_CODES, **kw)
    assert _same_search((dist, lab), ref)
    filled = lab >= 0
    assert np.array_equal(rows >= 0, filled)
    assert np.array_equal(c["ids"][rows[filled]].astype(np.int64), lab[filled])
    assert same(rec.reshape(-1, c["d"]), g.reconstruct_rows(rows.ravel()))
    assert is_empty(rec[~filled]) and (dist[~filled] == FLT_MAX).all()
    return filled


@pytest.mark.parametrize("filtered", [False, True], ids=["all", "filtered"])
@pytest.mark.parametrize("name", ["M16", "grouping"])
def test_search_reconstruct(gpu, name, filtered):
    c = corpus(**CASES[name])
    g = _upload(gpu(), c)
    if filtered:
        g.set_filter(np.random.default_rng(4).choice(c["ids"], len(c["ids"]) // 100, replace=False).astype(np.uint32))
    q64 = c["queries"][:64]
    unfilled = 0
    for k, heap in ((1, False), (10, False), (10, True)):
        for q in (q64, tiled(q64, 8192)):   # 8192: a search() of this size runs as two parts
            filled = check_search(g, c, q, k, heap, pruning=name == "grouping")
            assert filled.any()
            unfilled += (~filled).sum()
    assert (unfilled > 0) == filtered, "a 1 % filter leaves slots of k = 10 unfilled; no filter leaves none"


def test_search_reconstruct_dev_form(gpu, pkg):
    c = corpus(**BASE)
    g = _upload(gpu(), c)
    q = c["queries"][:64]
    k = 10
    dist, lab, rows, rec = g.search_reconstruct(q, k, NPROBE, MAX_CODES, efSearch=EF, space=pkg.RECON_ROTATED)
    d_dist = torch.empty((64, k), dtype=torch.float32, device="cuda")
    d_lab = torch.empty((64, k), dtype=torch.int64, device="cuda")
    d_rows = torch.empty((64, k), dtype=torch.int64, device="cuda")
    d_rec = torch.empty((64, k, c["d"]), dtype=torch.float32, device="cuda")
    for with_rows in (True, False):
        d_rec.zero_()
        g.search_reconstruct_dev(64, k, dev(q), d_dist, d_lab, d_rec, NPROBE, MAX_CODES, d_rows=d_rows if with_rows else None,
                                 efSearch=EF, space=pkg.RECON_ROTATED)
        g.sync()
        assert _same_search((d_dist.cpu().numpy(), d_lab.cpu().numpy()), (dist, lab))
        assert np.array_equal(d_rows.cpu().numpy(), rows) and same(d_rec.cpu().numpy(), rec)
    assert same(rec.reshape(-1, c["d"]), ref_rotated("M16")[rows.ravel()])


def test_search_reconstruct_returns_the_winning_row(gpu):
    """Every id 0: a lookup by label would return row 0 for every result; the rows are those of the twin with unique ids."""
    c = corpus(**BASE)
    twin = _upload(gpu(), c)
    zero = _upload(gpu(), _with_ids(c, np.zeros(len(c["ids"]), np.uint32)))
    q = c["queries"][:64]
    for k, heap in ((1, False), (10, False), (10, True)):
        a = twin.search_reconstruct(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
        b = zero.search_reconstruct(q, k, NPROBE, MAX_CODES, efSearch=EF, heap_order=heap)
        assert np.array_equal(a[2], b[2]) and same(a[3], b[3]) and np.array_equal(bits(a[0]), bits(b[0]))
        assert (b[1] == 0).all() and len(np.unique(a[2])) >= 32 and np.array_equal(c["ids"][a[2]], a[1])


# ---- 6. views --------------------------------------------------------------------------------------------------------
def test_view_reconstructs_the_parents_rows(gpu, pkg):
    c = corpus(**GROUPING_OPQ)
    g = _upload(gpu(), c)
    v = g.view()
    try:
        rows = np.arange(0, len(c["ids"]), 3)
        for space in (pkg.RECON_ROTATED, pkg.RECON_ORIGINAL):
            assert same(v.reconstruct_rows(rows, space), g.reconstruct_rows(rows, space))
        req = c["ids"][::11]
        assert np.array_equal(v.locate(req)[0], g.locate(req)[0])
        a = v.search_reconstruct(c["queries"], 10, NPROBE, MAX_CODES, efSearch=EF)
        b = g.search_reconstruct(c["queries"], 10, NPROBE, MAX_CODES, efSearch=EF)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    finally:
        v.close()


# ---- 7. errors and memory --------------------------------------------------------------------------------------------
def code_of(pkg, fn, *a, **kw):
    with pytest.raises(pkg.IvfHnswError) as e:
        fn(*a, **kw)
    return e.value.code


def test_errors(gpu, pkg):
    c = corpus(**BASE)
    rows = np.arange(4)
    lab = np.arange(4, dtype=np.uint32)
    q = c["queries"][:4]
    g = gpu()
    g.d = c["d"]
    # before upload_ivf
    for fn, a in ((g.locate, (lab,)), (g.reconstruct_rows, (rows,)), (g.reconstruct, (lab,)),
                  (g.search_reconstruct, (q, 1, NPROBE, MAX_CODES))):
        assert code_of(pkg, fn, *a) == pkg.ERR_STATE
    # lists but no quantizer: locate works, the reconstructing forms do not
    _upload(g, c, graph=False)
    assert g.locate(lab)[1].tolist() == [1, 1, 1, 1]
    for fn, a in ((g.reconstruct_rows, (rows,)), (g.reconstruct, (lab,)), (g.search_reconstruct, (q, 1, NPROBE, MAX_CODES))):
        assert code_of(pkg, fn, *a) == pkg.ERR_STATE
    # a quantizer of another shape
    small = corpus(**OPQ)["graph"]
    g.upload_quantizer(small.counts, small.links, small.vectors, small.enterpoint)
    assert code_of(pkg, g.reconstruct_rows, rows) == pkg.ERR_STATE
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    # an unknown space, rows out of range (nothing written), NULL buffers
    assert code_of(pkg, g.reconstruct_rows, rows, 2) == pkg.ERR_INVALID
    assert code_of(pkg, g.reconstruct, lab, -1) == pkg.ERR_INVALID
    assert code_of(pkg, g.search_reconstruct, q, 1, NPROBE, MAX_CODES, efSearch=EF, space=7) == pkg.ERR_INVALID
    n = len(c["ids"])
    L = pkg.lib()
    for bad in ([0, 1, n, 2], [0, -2, 1, 2]):
        r = np.array(bad, np.int64)
        out = np.full((4, c["d"]), 42.0, np.float32)
        assert L.ivfhnsw_gpu_reconstruct_rows(g._h, 4, r.ctypes.data, pkg.RECON_ROTATED, out.ctypes.data) == pkg.ERR_INVALID
        assert (out == 42.0).all()
    r = np.zeros(4, np.int64)
    assert L.ivfhnsw_gpu_reconstruct_rows(g._h, 4, r.ctypes.data, 0, None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_reconstruct_rows(g._h, 4, None, 0, r.ctypes.data) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_locate(g._h, 4, None, r.ctypes.data, None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_reconstruct(g._h, 4, None, 0, r.ctypes.data, None) == pkg.ERR_INVALID
    assert L.ivfhnsw_gpu_locate_dev(g._h, 4, 2, 8, None) == pkg.ERR_INVALID          # misaligned device pointers
    # what search_dev with out_keys refuses: heap order beyond k = 1024
    assert code_of(pkg, g.search_reconstruct, q, 1025, NPROBE, MAX_CODES, efSearch=EF, heap_order=True) == pkg.ERR_INVALID
    assert g.reconstruct_rows(rows).shape == (4, c["d"])   # the handle still works
    # a shard holds only its own lists
    s = gpu()
    own = np.arange(c["nc"]) % 2 == 0
    off = c["offsets"].astype(np.int64)
    keep = np.concatenate([np.arange(off[i], off[i + 1]) for i in np.nonzero(own)[0]])
    s.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"][keep], c["codes"][keep], c["norm_codes"][keep],
                 c["centroid_norms"], c["pq_centroids"], c["norm_table"], shard_rank=0, shard_world=2)
    s.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    for fn, a in ((s.locate, (lab,)), (s.reconstruct_rows, (rows,)), (s.reconstruct, (lab,)),
                  (s.search_reconstruct, (q, 1, NPROBE, MAX_CODES))):
        assert code_of(pkg, fn, *a) == pkg.ERR_STATE


def test_memory_stays_within_the_documented_workspace(gpu, pkg):
    c = corpus(**OPQ)
    g = _upload(gpu(), c)
    d, n = c["d"], 3000
    before = g.memory_bytes()
    g.reconstruct_rows(np.arange(n), pkg.RECON_ORIGINAL)
    rows_ws = g.memory_bytes() - before
    assert 0 < rows_ws <= n * (2 * 4 * d + 8)              # the ROTATED chunk, the staged output, the staged rows
    lab = np.arange(n, dtype=np.uint32)
    g.locate(lab)
    locate_ws = g.memory_bytes() - before - rows_ws
    bitmap = (n // 32 + 1) * 4
    assert 0 < locate_ws <= n * (20 + 16) + bitmap + 1024 * (n // 4096 + 1) + 16
    g.reconstruct_rows(np.arange(n), pkg.RECON_ORIGINAL)
    g.locate(lab)
    assert g.memory_bytes() == before + rows_ws + locate_ws    # kept, not grown again
