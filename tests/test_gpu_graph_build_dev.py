"""ivfhnsw_gpu_build_graph_dev: the whole insertion loop on device buffers -- the forward heuristic, the reverse lists and
the fold of mutuallyConnectNewElement as kernels (kernels_graph.hip) behind the neighbour-table sweep.  Checked link for
link against the oracle's SERIAL restatement of the contract (orc.Hnsw.build_exact), byte for byte against the
host-pointer form, and for what it must leave alone: its input, refused calls' outputs, and the index on the handle."""
import ctypes as C

import numpy as np
import pytest

import synth
from oracle import orc

pytestmark = pytest.mark.gpu

FILL = 0xAB  # the outputs start as this byte: what the call does not write shows


def clustered(rng, n, d, per=64, spread=18.0):
    """n rows in tight clusters of `per` around SIFT-like centres (the generator of test_gpu_graph_build.py)."""
    centres = synth.sift_like(rng, (n + per - 1) // per, d)
    x = centres[rng.integers(0, len(centres), n)] + rng.normal(0, spread, (n, d))
    return x.astype(np.float32)


def hub(n, d):
    """Unit directions scaled to norms 90..110 around a node 0 at the origin: every later node is nearer to node 0 than
    to most of its peers, so node 0's reverse list runs to a thousand entries and more."""
    rng = np.random.default_rng(5)
    u = rng.normal(0, 1, (n, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x = (u * rng.uniform(90, 110, (n, 1))).astype(np.float32)
    x[0] = 0
    return x


def vectors(kind, n, d):
    rng = np.random.default_rng(n + d)
    if kind == "clustered":
        return clustered(rng, n, d)
    if kind == "hub":
        return hub(n, d)
    if kind == "same":
        return np.tile(synth.sift_like(rng, 1, d), (n, 1))
    x = synth.sift_like(rng, n, d)
    if kind == "dups":
        x[100:180] = x[3]
    return x


_ORACLE = {}


def oracle_graph(case):
    """(x, counts, links [n, maxM]) of the oracle's serial loop, built once per case and never written to."""
    if case not in _ORACLE:
        kind, n, d, M, maxM, ncand = case
        x = vectors(kind, n, d)
        ref = orc.Hnsw.build_exact(x, M, maxM, ncand)
        counts, links = np.array(ref.counts, copy=True), np.array(ref.links, copy=True).reshape(n, maxM)
        ref.free()
        for a in (x, counts, links):
            a.setflags(write=False)
        _ORACLE[case] = (x, counts, links)
    return _ORACLE[case]


def build_dev(g, x, M, maxM, ncand):
    """build_graph_dev on fresh tensors: (counts u8 [n], links u32 [n, maxM], the vectors' tensor)."""
    import torch
    dev = torch.device("cuda", 0)
    n, d = x.shape
    tx = torch.tensor(x, device=dev)
    tc = torch.full((n,), FILL, dtype=torch.uint8, device=dev)
    tl = torch.full((n, 4 * maxM), FILL, dtype=torch.uint8, device=dev).view(torch.int32)
    torch.cuda.synchronize()  # the handle's stream does not wait for torch's
    g.build_graph_dev(n, d, tx, M, maxM, ncand, tc, tl)
    g.sync()
    return tc.cpu().numpy(), tl.cpu().numpy().view(np.uint32).reshape(n, maxM), tx


def check_against_oracle(case, counts, links):
    _, rc, rl = oracle_graph(case)
    maxM = case[4]
    assert np.array_equal(counts, rc)
    live = np.arange(maxM)[None, :] < counts[:, None]
    assert np.array_equal(np.where(live, links, 0), np.where(live, rl, 0))
    assert (links[~live] == 0).all()  # zeros from each node's count on, as the host form writes


SHAPES = [("iid", 3000, 128, 16, 32, 64), ("clustered", 20000, 32, 16, 32, 64), ("clustered", 2500, 96, 8, 16, 20),
          ("iid", 700, 16, 32, 64, 80), ("iid", 500, 64, 1, 1, 1), ("iid", 500, 64, 4, 4, 4),
          ("iid", 1, 128, 16, 32, 64), ("iid", 2, 128, 16, 32, 64), ("iid", 17, 128, 16, 32, 64),
          ("iid", 65, 128, 16, 32, 64), ("dups", 1200, 64, 16, 32, 48), ("same", 600, 64, 16, 32, 48)]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "-".join(str(v) for v in c))
def test_dev_graph_equals_the_serial_insertion_loop(gpu, case):
    kind, n, d, M, maxM, ncand = case
    x, rc, _ = oracle_graph(case)
    counts, links, _ = build_dev(gpu(), x, M, maxM, ncand)
    check_against_oracle(case, counts, links)
    if kind == "same":  # what the case is for: every distance 0, every tie rule, and shrinks that empty the lists
        assert rc.max() == 32 and abs(rc.mean() - 17.05) < 0.01


@pytest.mark.parametrize("d,hub_links", [(128, 2999), (32, 1000)])
def test_a_reverse_list_of_thousands_folds_in_order(gpu, d, hub_links):
    case = ("hub", 3000, d, 16, 32, 64)
    x, rc, rl = oracle_graph(case)
    # the hub property, on the oracle's graph: that many later nodes hold a live link to node 0, so node 0's reverse
    # list is at least that long
    live = np.arange(32)[None, :] < rc[:, None]
    assert int(((rl == 0) & live)[1:].any(axis=1).sum()) >= hub_links
    g = gpu()
    counts, links, _ = build_dev(g, x, 16, 32, 64)
    check_against_oracle(case, counts, links)
    assert g.last_graph_longest_reverse() >= hub_links


@pytest.mark.parametrize("case", [SHAPES[0], SHAPES[10]], ids=["iid-3000-128", "dups-1200-64"])
def test_host_and_device_forms_write_the_same_bytes(gpu, case):
    import torch
    kind, n, d, M, maxM, ncand = case
    x = oracle_graph(case)[0]
    g = gpu()
    hc, hl = g.build_graph(x, M, maxM, ncand)
    counts, links, tx = build_dev(g, x, M, maxM, ncand)
    assert np.array_equal(counts, hc) and np.array_equal(links, hl)
    assert torch.equal(tx.cpu(), torch.from_numpy(x))  # the vectors are only read
    counts2, links2, _ = build_dev(g, x, M, maxM, ncand)
    assert np.array_equal(counts2, counts) and np.array_equal(links2, links)


def test_invalid_arguments_are_refused_and_touch_nothing(gpu, pkg):
    import torch
    L = pkg.lib()
    g = gpu()
    dev = torch.device("cuda", 0)
    n, d = 300, 32
    flat = torch.zeros(n * d + 4, dtype=torch.float32, device=dev)
    tc = torch.full((n,), FILL, dtype=torch.uint8, device=dev)
    tl = torch.full((n * 65 * 4,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    px, pc, pl = flat.data_ptr(), tc.data_ptr(), tl.data_ptr()
    assert px % 16 == 0
    cases = [  # (d, vectors, M, maxM, ncand, counts, links)
        (d, None, 16, 32, 64, pc, pl), (d, px, 16, 32, 64, None, pl), (d, px, 16, 32, 64, pc, None),
        (d, px, 0, 32, 64, pc, pl),    # M = 0
        (d, px, 33, 32, 64, pc, pl),   # M > maxM
        (d, px, 16, 65, 80, pc, pl),   # maxM = 65
        (d, px, 16, 32, 15, pc, pl),   # ncand < M
        (d, px, 16, 32, 81, pc, pl),   # ncand = 81
        (24, px, 16, 32, 64, pc, pl),  # d no multiple of 16
        (d, px + 4, 16, 32, 64, pc, pl),  # vectors off 16-byte alignment
    ]
    for dd, v, M, maxM, ncand, c, l in cases:
        rc = L.ivfhnsw_gpu_build_graph_dev(g._h, n, dd, C.c_void_p(v), M, maxM, ncand, C.c_void_p(c), C.c_void_p(l))
        assert rc == pkg.ERR_INVALID, (dd, v, M, maxM, ncand, c, l)
    assert L.ivfhnsw_gpu_build_graph_dev(None, n, d, C.c_void_p(px), 16, 32, 64, C.c_void_p(pc), C.c_void_p(pl)) == pkg.ERR_INVALID
    g.sync()
    assert (tc.cpu() == FILL).all() and (tl.cpu() == FILL).all() and (flat.cpu() == 0).all()


def test_an_uploaded_index_searches_the_same_after_build_graph_dev(gpu):
    c = synth.make_corpus(seed=7, nc=128, d=128, M=16, n_base=8000, nq=32, efConstruction=100)
    g = gpu()
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"])
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    before = [g.search(c["queries"], k, 8, 2000, efSearch=40) for k in (1, 10)]
    m0 = g.memory_bytes()
    case = SHAPES[0]
    kind, n, d, M, maxM, ncand = case
    counts, links, _ = build_dev(g, oracle_graph(case)[0], M, maxM, ncand)
    check_against_oracle(case, counts, links)
    m1 = g.memory_bytes()
    # the workspace stays on the handle: at least the candidate table, the forward links and the sort's two arrays
    assert m1 >= m0 + n * ncand * 4 + 3 * n * M * 4
    after = [g.search(c["queries"], k, 8, 2000, efSearch=40) for k in (1, 10)]
    for (d0, l0), (d1, l1) in zip(before, after):
        assert np.array_equal(l0, l1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    m2 = g.memory_bytes()
    small = SHAPES[9]
    build_dev(g, oracle_graph(small)[0], *small[3:])
    assert g.memory_bytes() == m2 >= m1  # a smaller call frees nothing and needs nothing more
