"""searchDisk's exact re-rank on the device (ivfhnsw_gpu_upload_base / ivfhnsw_gpu_rerank[_dev]): labels and distance BITS
against the numpy restatement of fvec_L2sqr plus a lexicographic (distance, label) top-k (tests/rerank_ref.py, pinned to
the host library's own function by tests/test_rerank_cpu.py), the upload forms, the stream ordering after search_dev,
views, the documented errors, and the recall the re-rank buys on a SIFT-like uint8 corpus."""
import numpy as np
import pytest

import rerank_ref
import synth

pytestmark = pytest.mark.gpu


def _base(rng, n, d):
    b = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    b[1] = b[0]          # exact ties: equal rows, so equal distances, ordered by label
    b[7] = b[0]
    b[n - 1] = b[3]
    return b


def _cands(rng, nq, kc, n):
    c = rng.integers(0, n, size=(nq, kc)).astype(np.int64)
    c[rng.random((nq, kc)) < 0.1] = -1                # holes
    if kc > 1:
        c[0, 1] = c[0, 0]                                # a duplicate label stays a duplicate
    if nq > 1 and kc >= 3:
        c[1, :3] = [0, 1, 7]                             # three tied rows
    if nq > 2:
        c[2] = -1                                        # an all-empty query
    if nq > 3 and kc > 2:
        c[3, kc // 2:] = -1                              # fewer valid candidates than k = kc
    return c


def _queries(rng, nq, d, kind):
    q = rng.standard_normal((nq, d)).astype(np.float32) * np.float32(70) + np.float32(120)
    return np.rint(q).astype(np.float32) if kind == "integer" else q


def _same(got, want):
    gd, gl = got
    wd, wl = want
    assert np.array_equal(gl, wl), np.nonzero((gl != wl).any(1))[0][:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


CASES = [(d, kc, k) for d in (16, 96, 128, 512) for kc in (1, 10, 100, 1000, 4096) for k in sorted({1, 10, kc}) if k <= kc]


@pytest.mark.parametrize("d,kc,k", CASES)
def test_rerank_equals_the_restatement(gpu, d, kc, k):
    rng = np.random.default_rng(d * 7919 + kc * 31 + k)
    n = 6000
    base = _base(rng, n, d)
    nq = 24 if kc <= 100 else 6
    cand = _cands(rng, nq, kc, n)
    g = gpu()
    g.upload_base(base)
    for kind in ("float", "integer"):
        q = _queries(rng, nq, d, kind)
        _same(g.rerank(q, cand, k), rerank_ref.rerank(base, q, cand, k))
    g.close()


def test_bvecs_image_in_chunks_equals_one_shot_and_dev_upload(gpu, tmp_path):
    import torch
    rng = np.random.default_rng(5)
    n, d = 3001, 128
    base = _base(rng, n, d)
    img = np.empty((n, d + 4), np.uint8)
    img[:, :4] = np.frombuffer(np.int32(d).tobytes(), np.uint8)
    img[:, 4:] = base
    path = tmp_path / "base.bvecs"
    img.tofile(path)
    q = _queries(rng, 16, d, "float")
    cand = _cands(rng, 16, 200, n)
    want = rerank_ref.rerank(base, q, cand, 10)
    g = gpu()
    g.upload_base(base)
    _same(g.rerank(q, cand, 10), want)
    # stride d + 4, straight from the file image, in uneven chunks
    for first in range(0, n, 700):
        m = min(700, n - first)
        g.upload_base(img[first:first + m, 4:], n=n, first=first, row_stride=d + 4)
    _same(g.rerank(q, cand, 10), want)
    assert g.upload_base_bvecs(str(path), chunk_rows=1000) == (n, d)
    _same(g.rerank(q, cand, 10), want)
    # the device form, from a torch tensor, again with the file's stride
    t = torch.from_numpy(img.reshape(-1)).cuda()
    torch.cuda.synchronize()
    g.upload_base_dev(n, d, 0, 1500, t[4:], row_stride=d + 4)
    g.upload_base_dev(n, d, 1500, n - 1500, t[1500 * (d + 4) + 4:], row_stride=d + 4)
    _same(g.rerank(q, cand, 10), want)
    assert g.memory_bytes() >= n * d
    g.close()


def test_rerank_dev_behind_search_dev_on_the_handles_stream(gpu):
    import torch
    c = synth.make_corpus(seed=91, nc=128, d=128, M=16, n_base=8000, nq=64, efConstruction=80)
    base = np.clip(np.rint(c["base"]), 0, 255).astype(np.uint8)
    g = gpu()
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"])
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    g.upload_base(base)
    nq, kc, k, nprobe, max_codes, ef = 64, 100, 10, 16, 4000, 64
    q = np.rint(c["queries"]).astype(np.float32)
    # host form on the labels of an ordinary search
    _, cl = g.search(q, kc, nprobe, max_codes, efSearch=ef)
    want = g.rerank(q, cl, k)
    _same(want, rerank_ref.rerank(base, q, cl, k))
    # device form queued right behind search_dev, no synchronisation in between
    tq = torch.from_numpy(q).cuda()
    cd = torch.empty((nq, kc), dtype=torch.float32, device="cuda")
    cl2 = torch.full((nq, kc), -7, dtype=torch.int64, device="cuda")
    od = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    ol = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g.search_dev(nq, kc, tq, cd, cl2, nprobe, max_codes, efSearch=ef)
    g.rerank_dev(nq, kc, tq, cl2, k, od, ol)
    g.sync()
    _same((od.cpu().numpy(), ol.cpu().numpy()), want)
    _same(g.search_rerank(q, k, kc, nprobe, max_codes, efSearch=ef), want)
    # a label >= n on the device form is an empty slot, never read
    bad = cl.copy()
    bad[:, 0] = len(base) + 5
    tb = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    g.rerank_dev(nq, kc, tq, tb, k, od, ol)
    g.sync()
    _same((od.cpu().numpy(), ol.cpu().numpy()), rerank_ref.rerank(base, q, bad, k))
    # a view sees the parent's store
    v = g.view()
    _same(v.rerank(q, cl, k), want)
    v.close()
    g.close()


def test_errors_leave_the_handle_usable(gpu, pkg):
    rng = np.random.default_rng(9)
    n, d = 500, 32
    base = _base(rng, n, d)
    q = _queries(rng, 4, d, "float")
    cand = _cands(rng, 4, 50, n)
    want = rerank_ref.rerank(base, q, cand, 5)
    g = gpu()

    def code(f, *a, **kw):
        with pytest.raises(pkg.IvfHnswError) as e:
            f(*a, **kw)
        return e.value.code

    assert code(g.rerank, q, cand, 5) == pkg.ERR_STATE                       # no store
    assert code(g.upload_base, np.zeros((4, 24), np.uint8)) == pkg.ERR_INVALID  # d % 16 != 0
    assert code(g.upload_base, np.zeros((4, 528), np.uint8)) == pkg.ERR_INVALID  # d > 512
    assert code(g.upload_base, base[:10], n=n, first=10) == pkg.ERR_STATE     # a later chunk without a store
    g.upload_base(base)
    _same(g.rerank(q, cand, 5), want)
    assert code(g.upload_base, base[:10, :16].copy(), n=n, first=10) == pkg.ERR_INVALID  # d differs from the store's
    assert code(g.upload_base, base[:10], n=n + 1, first=10) == pkg.ERR_INVALID          # n differs
    assert code(g.upload_base, base[:10], n=n, first=n - 5) == pkg.ERR_INVALID           # rows beyond n
    big = np.zeros((4, 4097), np.int64)
    assert code(g.rerank, q, big, 5) == pkg.ERR_INVALID                      # kc > 4096
    assert code(g.rerank, q, cand, 51) == pkg.ERR_INVALID                    # k > kc
    assert code(g.rerank, q, cand, 0) == pkg.ERR_INVALID                     # k = 0
    oob = cand.copy()
    oob[2, 3] = n
    assert code(g.rerank, q, oob, 5) == pkg.ERR_INVALID                      # label outside [-1, n) in the host form
    oob[2, 3] = -2
    assert code(g.rerank, q, oob, 5) == pkg.ERR_INVALID
    _same(g.rerank(q, cand, 5), want)                                        # still usable, store untouched
    g.upload_base(np.zeros((0, d), np.uint8), n=0)                           # n = 0 frees the store
    assert code(g.rerank, q, cand, 5) == pkg.ERR_STATE
    g.upload_base(base)
    _same(g.rerank(q, cand, 5), want)
    g.close()


# ---------------------------------------------------------------------------------------------- recall
def test_rerank_recall_on_a_sift_like_uint8_corpus(gpu, pkg):
    c = rerank_ref.uint8_recall_corpus(pkg, seed=77)
    g = gpu()
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"])
    g.upload_quantizer(c["counts"], c["links"], c["centroids"], 0)
    g.upload_base(c["base"])
    q, gt = c["queries"], c["gt"]
    nprobe, max_codes, ef, k, kc = 32, 20000, 80, 10, 100
    d_adc, l_adc = g.search(q, k, nprobe, max_codes, efSearch=ef)
    d_c, l_c = g.search(q, kc, nprobe, max_codes, efSearch=ef)
    dr, lr = g.search_rerank(q, k, kc, nprobe, max_codes, efSearch=ef)
    _same((dr, lr), g.rerank(q, l_c, k))
    # top-1 is the exact minimum over the query's candidates
    for i in range(len(q)):
        labs = l_c[i][l_c[i] >= 0]
        assert dr[i, 0] == rerank_ref.fvec_l2sqr(q[i], c["base"][labs].astype(np.float32)).min()
    r1_adc = float((l_adc[:, 0] == gt[:, 0]).mean())
    r1_rr = float((lr[:, 0] == gt[:, 0]).mean())
    r10_adc = float(np.mean([gt[i, 0] in l_adc[i] for i in range(len(q))]))
    r10_rr = float(np.mean([gt[i, 0] in lr[i] for i in range(len(q))]))
    print("\n[rerank recall] 200k uint8 vectors, 1024 centroids, PQ16, (%d, %d, %d), kc %d: Recall@1 %.4f -> %.4f, "
          "Recall@10 %.4f -> %.4f" % (nprobe, max_codes, ef, kc, r1_adc, r1_rr, r10_adc, r10_rr))
    assert r1_rr >= r1_adc + 0.1
    assert r10_rr >= r10_adc
    g.close()
