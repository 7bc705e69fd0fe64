"""Exact Lloyd k-means of the coarse centroids on the device (ivfhnsw_gpu_kmeans[_dev]): centroid BITS,
assignments and objectives against the numpy restatement (tests/kmeans_ref.py, whose split rule
tests/test_kmeans_ref_cpu.py pins), empty-cluster splits, a cluster far larger than any per-cluster LDS tile, the device
form, the documented errors, a 2 M x 65 536 run without the oracle, the recall learnt centroids buy over random seeds,
and tools/learn_centroids.py's .fvecs through the class surface's build_quantizer."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kmeans_ref as kr
import synth
from oracle import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "cpp", "hostlib_tool.bin")


def _mixture(rng, n, d, ncomp, spread=12.0):
    """uint8-valued float rows around ncomp SIFT-like centres, component sizes log-normal (heavy-tailed)."""
    centres = synth.sift_like(rng, ncomp, d)
    w = rng.lognormal(0.0, 1.0, ncomp)
    comp = rng.choice(ncomp, size=n, p=w / w.sum())
    x = centres[comp] + rng.normal(0.0, spread, (n, d))
    return np.clip(np.rint(x), 0, 255).astype(np.float32)


def _same(got, want):
    c, a, obj = got
    wc, wa, wobj = want
    assert np.array_equal(a, wa), np.nonzero(a != wa)[0][:8]
    bad = np.nonzero((c.view(np.uint32) != wc.view(np.uint32)).any(1))[0]
    assert bad.size == 0, ("centroid rows differ", bad[:8])
    np.testing.assert_allclose(obj, wobj, rtol=1e-9)


@pytest.mark.parametrize("d,nc,n,niter", [(128, 256, 20000, 1), (128, 1024, 30000, 3), (96, 2048, 40000, 3),
                                          (32, 4096, 50000, 1), (32, 512, 50000, 3)])
def test_iterations_equal_the_restatement(gpu, d, nc, n, niter):
    rng = np.random.default_rng(d * 7 + nc + niter)
    x = _mixture(rng, n, d, max(8, nc // 4))
    seeds = x[rng.choice(n, nc, replace=False)]
    g = gpu()
    got = g.kmeans(x, seeds, niter)
    _same(got, kr.kmeans(x, seeds, niter))


def test_empty_clusters_are_split_like_the_restatement(gpu):
    """Every seed row twice: the lower id wins each tie, the other copy is empty and takes half of the largest
    cluster -- in every iteration the restatement's splits, bit for bit."""
    rng = np.random.default_rng(21)
    n, d, half = 20000, 128, 300
    x = _mixture(rng, n, d, 64)
    base = x[rng.choice(n, half, replace=False)]
    seeds = np.concatenate([base, base[::-1], base[:12]])      # 612 rows, every one repeated
    a0, _ = kr.assign(x, seeds)
    assert np.bincount(a0, minlength=len(seeds)).tolist().count(0) >= half
    g = gpu()
    _same(g.kmeans(x, seeds, 4), kr.kmeans(x, seeds, 4))


def test_a_cluster_of_70000_points_and_its_splits(gpu):
    """70 000 of 100 000 points on ONE row (interleaved with the rest in point order), several seeds on that row: one
    cluster of 70 000 members (far beyond one LDS tile), empty twins split from it, later iterations re-divide it."""
    rng = np.random.default_rng(22)
    n, d, nc = 100000, 32, 256
    x = _mixture(rng, n, d, 40)
    spot = rng.permutation(n)[:70000]
    x[spot] = x[spot[0]]
    seeds = x[rng.choice(n, nc, replace=False)]
    seeds[:5] = x[spot[0]]
    a0, _ = kr.assign(x, seeds)
    assert np.bincount(a0, minlength=nc).max() >= 70000
    g = gpu()
    _same(g.kmeans(x, seeds, 3), kr.kmeans(x, seeds, 3))


def test_dev_form_equals_host_form_and_niter_zero_returns_the_seeds(gpu, pkg):
    import torch
    rng = np.random.default_rng(23)
    n, d, nc = 30000, 96, 1000
    x = _mixture(rng, n, d, 200)
    seeds = np.concatenate([x[rng.choice(n, nc - 10, replace=False)], x[:10]])
    g = gpu()
    c, a, obj = g.kmeans(x, seeds, 3)
    dev = torch.device("cuda", 0)
    tx = torch.from_numpy(x).to(dev)
    tc = torch.from_numpy(seeds).to(dev)
    ta = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the handle's stream does not wait for torch's
    obj_d = g.kmeans_dev(n, d, nc, tx, 3, tc, ta)
    assert np.array_equal(tc.cpu().numpy().view(np.uint32), c.view(np.uint32))
    assert np.array_equal(ta.cpu().numpy().view(np.uint32), a)
    assert np.array_equal(obj_d, obj)
    # niter = 0: the seeds come back, nothing else is written
    a0 = np.full(n, 0xdeadbeef, np.uint32)
    o0 = np.full(1, 7.5)
    c0 = seeds.copy()
    rc = pkg.lib().ivfhnsw_gpu_kmeans(g._h, n, d, nc, x.ctypes.data_as(C.c_void_p), 0, c0.ctypes.data_as(C.c_void_p),
                                      a0.ctypes.data_as(C.c_void_p), o0.ctypes.data_as(C.c_void_p))
    assert rc == pkg.OK
    assert np.array_equal(c0, seeds) and (a0 == 0xdeadbeef).all() and o0[0] == 7.5
    tc0 = torch.from_numpy(seeds).to(dev)
    ta.fill_(-1)
    torch.cuda.synchronize()
    g.kmeans_dev(n, d, nc, tx, 0, tc0, ta)
    torch.cuda.synchronize()
    assert np.array_equal(tc0.cpu().numpy(), seeds) and (ta.cpu().numpy() == -1).all()


def test_an_uploaded_index_searches_the_same_after_kmeans(gpu):
    c = synth.make_corpus(seed=7, nc=128, d=128, M=16, n_base=8000, nq=32, efConstruction=100)
    g = gpu()
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"])
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    before = [g.search(c["queries"], k, 8, 2000, efSearch=40) for k in (1, 10)]
    rng = np.random.default_rng(24)
    x = _mixture(rng, 20000, 128, 50)
    g.kmeans(x, x[:300], 2)
    after = [g.search(c["queries"], k, 8, 2000, efSearch=40) for k in (1, 10)]
    for (d0, l0), (d1, l1) in zip(before, after):
        assert np.array_equal(l0, l1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))


def test_invalid_arguments_are_refused_and_touch_nothing(gpu, pkg):
    import torch
    L = pkg.lib()
    g = gpu()
    rng = np.random.default_rng(25)
    x = _mixture(rng, 2000, 128, 10)
    c = x[:16].copy()
    a = np.full(2000, 0xabcdef01, np.uint32)
    o = np.full(2, 3.25)
    P = lambda arr: arr.ctypes.data_as(C.c_void_p)  # noqa: E731
    cases = [  # (n, d, nc, x, centroids)
        (2000, 130, 16, P(x), P(c)),   # d > 128
        (2000, 126, 16, P(x), P(c)),   # not a multiple of 4
        (2000, 0, 16, P(x), P(c)),
        (2000, 128, 0, P(x), P(c)),    # nc = 0
        (10, 128, 16, P(x), P(c)),     # nc > n
        (1 << 31, 128, 16, P(x), P(c)),  # n >= 2^31 (refused before anything is read)
        (2000, 128, 16, None, P(c)),
        (2000, 128, 16, P(x), None),
    ]
    for n, d, nc, px, pc in cases:
        for niter in (0, 2):
            rc = L.ivfhnsw_gpu_kmeans(g._h, n, d, nc, px, niter, pc, P(a), P(o))
            assert rc == pkg.ERR_INVALID, (n, d, nc, niter)
            assert np.array_equal(c, x[:16]) and (a == 0xabcdef01).all() and (o == 3.25).all()
    assert L.ivfhnsw_gpu_kmeans(None, 2000, 128, 16, P(x), 2, P(c), P(a), P(o)) == pkg.ERR_INVALID
    dev = torch.device("cuda", 0)
    tx = torch.from_numpy(x).to(dev)
    tc = torch.from_numpy(c).to(dev)
    ta = torch.full((2000,), 5, dtype=torch.int32, device=dev)
    # device form: the same limits, and a centroid pointer off 16-byte alignment
    flat = torch.zeros(16 * 128 + 1, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for args in [(2000, 100 + 30, 16, tx.data_ptr(), tc.data_ptr()), (2000, 128, 2001, tx.data_ptr(), tc.data_ptr()),
                 (2000, 128, 16, tx.data_ptr(), flat.data_ptr() + 4)]:
        n, d, nc, px, pc = args
        rc = L.ivfhnsw_gpu_kmeans_dev(g._h, n, d, nc, C.c_void_p(px), 2, C.c_void_p(pc), C.c_void_p(ta.data_ptr()), P(o))
        assert rc == pkg.ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(tc.cpu(), torch.from_numpy(x[:16])) and (ta.cpu() == 5).all() and (o == 3.25).all()
    # the handle still works
    c2, a2, o2 = g.kmeans(x, c, 1)
    assert np.isfinite(c2).all() and len(o2) == 1


def test_two_million_points_65536_clusters(gpu, pkg):
    """n = 2 M, nc = 65 536, d = 128, no oracle: finite centroids, counts summing to n, the last iteration's assignment
    = knn(k = 1) against its seeds, a falling objective."""
    import torch
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(26)
    n, d, nc = 2_000_000, 128, 65536
    centres = torch.randint(0, 200, (20000, d), generator=gen, device=dev, dtype=torch.int32).float()
    comp = torch.randint(0, 20000, (n,), generator=gen, device=dev)
    x = (centres[comp] + torch.randn((n, d), generator=gen, device=dev) * 10).round().clamp(0, 255).contiguous()
    pick = torch.randperm(n, generator=gen, device=dev)[:nc]
    seeds = x[pick].contiguous()
    g = gpu()
    c3 = seeds.clone()
    a3 = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the handle's stream does not wait for torch's
    obj3 = g.kmeans_dev(n, d, nc, x, 3, c3, a3)
    assert torch.isfinite(c3).all()
    a3h = a3.cpu().numpy().view(np.uint32)
    assert a3h.max() < nc and np.bincount(a3h, minlength=nc).sum() == n
    assert obj3[2] < obj3[0], obj3
    # out_assign of niter = 2 = knn(k = 1) of x against the centroids niter = 1 leaves
    c1 = seeds.clone()
    torch.cuda.synchronize()
    g.kmeans_dev(n, d, nc, x, 1, c1)
    c2 = seeds.clone()
    a2 = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    obj2 = g.kmeans_dev(n, d, nc, x, 2, c2, a2)
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    g.knn_dev(n, nc, d, x, c1, 1, ids)
    g.sync()
    assert torch.equal(ids, a2)
    assert obj2[0] == obj3[0] and obj2[1] == obj3[1]


def _ivf_recall(pkg, centroids, base, queries, gt, M=16, nprobe=8, max_codes=4000, ef=80):
    """The library's own build pipeline over the given centroids (as rerank_ref.uint8_recall_corpus): graph, code books
    from a sample's residuals, encode, upload, search.  Returns Recall@1."""
    rng = np.random.default_rng(5)
    nc, d = centroids.shape
    g = pkg.GpuIndex(0)
    try:
        counts, links = g.build_graph(centroids, 16, 32, 64)
        g.upload_quantizer(counts, links, centroids, 0)
        xs = base[rng.choice(len(base), 32768, replace=False)]
        idx_s, _ = g.coarse(xs, 1, 220)
        res = (xs - centroids[idx_s[:, 0]]).astype(np.float32)
        dsub = d // M
        cb0 = np.stack([res[rng.choice(len(res), 256, replace=False), m * dsub:(m + 1) * dsub] for m in range(M)])
        cb, _ = g.pq_train(res, M, cb0, niter=6)
        g.upload_codebooks(d, M, cb, np.arange(256, dtype=np.float32))
        _, codes_s, _ = g.encode(xs, precomputed_idx=idx_s[:, 0])
        recon = centroids[idx_s[:, 0]] + synth._pq_decode(codes_s, cb)
        norm_table = np.quantile((recon.astype(np.float64) ** 2).sum(1), (np.arange(256) + 0.5) / 256).astype(np.float32)
        g.upload_codebooks(d, M, cb, norm_table)
        idx, codes, ncodes = g.encode(base, efSearch=220)
        order = np.argsort(idx, kind="stable")
        offsets = np.zeros(nc + 1, np.uint64)
        offsets[1:] = np.cumsum(np.bincount(idx, minlength=nc))
        cn = (centroids.astype(np.float64) ** 2).sum(1).astype(np.float32)
        g.upload_ivf(d, M, offsets, order.astype(np.uint32), codes[order], ncodes[order], cn, cb, norm_table)
        _, lab = g.search(queries, 1, nprobe, max_codes, efSearch=ef)
    finally:
        g.close()
    return float((lab[:, 0] == gt).mean())


def test_learnt_centroids_beat_random_seeds_end_to_end(gpu, pkg):
    rng = np.random.default_rng(27)
    n, d, nc, nq = 200_000, 128, 1024, 1000
    base = _mixture(rng, n, d, 3000, spread=10.0)
    src = rng.choice(n, nq, replace=False)          # near-duplicates of base rows: recall measures the index
    queries = np.clip(np.rint(base[src] + rng.normal(0.0, 4.0, (nq, d))), 0, 255).astype(np.float32)
    gt, _ = gpu().knn(base, 1, queries)
    learnt, obj = pkg.learn_centroids(base, nc, niter=10, seed=1)
    seeds, obj0 = pkg.learn_centroids(base, nc, niter=0, seed=1)
    assert len(obj0) == 0 and obj[-1] < obj[0]
    r_learnt = _ivf_recall(pkg, learnt, base, queries, gt[:, 0])
    r_seeds = _ivf_recall(pkg, seeds, base, queries, gt[:, 0])
    print("\n[kmeans recall] 200k uint8-valued rows, heavy-tailed mixture, 1024 centroids, PQ16, (8, 4000, 80), "
          "queries = base rows + N(0, 4): "
          "Recall@1 %.4f with random seeds -> %.4f with 10 Lloyd iterations" % (r_seeds, r_learnt))
    assert r_learnt > r_seeds


def test_learn_centroids_tool_writes_what_build_quantizer_loads(gpu, pkg, tmp_path):
    rng = np.random.default_rng(28)
    n, d, nc = 6000, 128, 20                       # 6000 > 20 * 256: the tool subsamples
    x = _mixture(rng, n, d, 30).astype(np.uint8)
    learn = str(tmp_path / "learn.bvecs")
    out = str(tmp_path / "centroids.fvecs")
    rec = np.empty((n, 4 + d), np.uint8)
    rec[:, :4] = np.frombuffer(np.int32(d).tobytes(), np.uint8)
    rec[:, 4:] = x
    rec.tofile(learn)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "learn_centroids.py"), "--learn", learn, "--nc",
                        str(nc), "--niter", "5", "--seed", "9", "--out", out], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["n_used"] == nc * 256 and len(rep["obj"]) == 5
    want, obj = pkg.learn_centroids(x, nc, niter=5, seed=9)
    got = pkg.read_xvecs(out)
    assert got.shape == (nc, d) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_allclose(rep["obj"], obj, rtol=1e-12)
    info, edges = str(tmp_path / "hnsw.info"), str(tmp_path / "hnsw.edges")
    env = {k: v for k, v in os.environ.items() if k != "IVFHNSW_BUILD"}
    b = subprocess.run([TOOL, "build_quantizer", out, str(nc), str(d), "16", "100", info, edges], capture_output=True,
                       text=True, env=env, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    gph = orc.Hnsw.load(info, out, edges)
    assert gph.n == nc
    assert np.array_equal(gph.vectors, want)
