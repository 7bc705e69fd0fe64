"""numpy restatement of searchDisk's exact re-rank (IndexIVF_HNSW_Grouping.cpp:365-395), the expected values of the
re-rank tests: fvec_L2sqr's arithmetic (utils.cpp:22-52; eight float32 accumulators over blocks of 8 dims, then summed
left to right, every operation rounded to float32) and a lexicographic (distance, label) top-k."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def fvec_l2sqr(q, x):
    """q [d] float32, x [n, d] float32 -> [n] float32, bit for bit the host library's fvec_L2sqr."""
    q = np.asarray(q, np.float32)
    x = np.asarray(x, np.float32).reshape(-1, q.shape[-1])
    nb = 2 * (q.shape[-1] // 16)
    diff = q[None, :8 * nb] - x[:, :8 * nb]
    sq = (diff * diff).reshape(x.shape[0], nb, 8)
    acc = np.zeros((x.shape[0], 8), np.float32)
    for b in range(nb):
        acc = acc + sq[:, b]
    r = acc[:, 0] + acc[:, 1]
    for l in range(2, 8):
        r = r + acc[:, l]
    return r


def rerank(base_u8, queries, cand, k):
    """The k best candidates of every query by (exact distance, label); labels outside [0, n) are empty; padding
    FLT_MAX / -1.  Returns (distances [nq, k] float32, labels [nq, k] int64)."""
    n = base_u8.shape[0]
    cand = np.asarray(cand, np.int64)
    nq = cand.shape[0]
    out_d = np.full((nq, k), FLT_MAX, np.float32)
    out_l = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        c = cand[i]
        labs = c[(c >= 0) & (c < n)]
        if labs.size == 0:
            continue
        dist = fvec_l2sqr(queries[i], base_u8[labs].astype(np.float32))
        keys = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | labs.astype(np.uint64)
        keys.sort()
        m = min(k, keys.size)
        out_d[i, :m] = (keys[:m] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        out_l[i, :m] = (keys[:m] & np.uint64(0xffffffff)).astype(np.int64)
    return out_d, out_l


def uint8_recall_corpus(pkg, seed, nc=1024, n_base=200_000, d=128, M=16, nq=1000, base_noise=10.0):
    """SIFT-like uint8 data through the library's own build pipeline (as synth.make_recall_corpus, but every base row
    and query is integer-valued and clipped to 0..255, as SIFT's are); gt = the 10 exact nearest rows (ivfhnsw_gpu_knn)."""
    import synth
    rng = np.random.default_rng(seed)
    centroids = synth.clustered_centroids(rng, nc, d)
    g = pkg.GpuIndex(0)
    counts, links = g.build_graph(centroids, 16, 32, 64)
    g.upload_quantizer(counts, links, centroids, 0)
    sizes = synth.list_sizes(rng, nc, n_base).astype(np.int64)
    gen = np.repeat(np.arange(nc, dtype=np.uint32), sizes)
    rng.shuffle(gen)
    noise = rng.standard_normal((n_base, d), dtype=np.float32) * np.float32(base_noise)
    base = np.clip(np.rint(centroids[gen] + noise), 0, 255).astype(np.uint8)
    basef = base.astype(np.float32)
    pick = rng.choice(n_base, size=32768, replace=False)
    xs = basef[pick]
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
    idx, codes, ncodes = g.encode(basef, efSearch=220)
    order = np.argsort(idx, kind="stable")
    offsets = np.zeros(nc + 1, np.uint64)
    offsets[1:] = np.cumsum(np.bincount(idx, minlength=nc))
    # fresh draws from the base's own distribution (not perturbed base rows): the nearest row is then rarely far ahead of
    # the next ones, which is where PQ16's approximate distances lose the true neighbour and the exact re-rank finds it
    qgen = gen[rng.choice(n_base, size=nq, replace=False)]
    queries = np.clip(np.rint(centroids[qgen] + rng.standard_normal((nq, d), dtype=np.float32) * np.float32(base_noise)),
                      0, 255).astype(np.float32)
    gt, _ = g.knn(basef, 10, queries)
    g.close()
    return dict(d=d, nc=nc, code_size=M, centroids=centroids, counts=counts, links=links, offsets=offsets,
                ids=order.astype(np.uint32), codes=codes[order], norm_codes=ncodes[order], pq_centroids=cb,
                norm_table=norm_table, base=base, queries=queries, gt=gt.astype(np.int64),
                centroid_norms=(centroids.astype(np.float64) ** 2).sum(1).astype(np.float32))
