"""The tie-overflow graph of test_gpu_walk_ties.py behind the host-pointer small-batch entry point.

After prepare_latency a host-pointer call of <= 256 queries takes the latency walk, which keeps at most 64 exact ties at
the efSearch boundary: it only flags the overflow, and the call consumes the bit and repeats itself on the throughput
walk.  test_gpu_walk_ties.py reaches that graph through coarse() (the non-deferring form) and through 9000-query searches
(no latency walk) only."""
import numpy as np
import pytest

from oracle import orc
from test_gpu_walk_ties import D, EF, build, queries

pytestmark = pytest.mark.gpu


def index_over_graph(gpu, M):
    """build(70) as the coarse quantizer of a tiny index with code size M, as
    test_tail_spill_inside_a_full_search_and_a_split_batch has it: (handle, oracle graph, oracle index)."""
    counts, links, vec, ep = build(70)
    n = len(counts)
    rng = np.random.default_rng(3)
    sizes = rng.integers(1, 6, n)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(sizes)
    tot = int(offsets[-1])
    codes = rng.integers(0, 256, (tot, M)).astype(np.uint8)
    ncodes = rng.integers(0, 256, tot).astype(np.uint8)
    ids = np.arange(tot, dtype=np.uint32)
    pq = rng.normal(0, 0.2, (M, 256, D // M)).astype(np.float32)
    ntab = np.sort(rng.normal(9, 1, 256)).astype(np.float32)
    cn = (vec.astype(np.float64) ** 2).sum(1).astype(np.float32)
    g = gpu()
    g.upload_ivf(D, M, offsets, ids, codes, ncodes, cn, pq, ntab)
    g.upload_quantizer(counts, links, vec, ep)
    og = orc.Hnsw.from_arrays(counts, links, vec, 16, ep)
    ox = orc.Index(D, M, og, pq, ntab, offsets, ids, codes, ncodes, cn)
    ox.set_params(16, 10 ** 9, EF)
    return g, og, ox


@pytest.mark.parametrize("M", [16, 4])
def test_host_pointer_small_batch_repeats_itself_on_the_throughput_walk(gpu, M):
    """M = 16 (dsub 6): calls of <= 8 queries end in the one-launch tail kernel, which copies the status itself and whose
    meeting words the latency walk clears; M = 4: no tail kernel, the status comes back by copy.  Nothing of one call may
    stay behind for the next."""
    g, og, ox = index_over_graph(gpu, M)
    g.prepare_latency()
    q = queries(200, 11)
    rd, rl, _, _, _ = ox.search_batch(q, 1, 8)

    def check(lo, hi):
        dist, lab = g.search(q[lo:hi], 1, 16, 10 ** 9, efSearch=EF)
        assert np.array_equal(lab, rl[lo:hi]), (lo, hi)
        assert np.array_equal(dist.view(np.uint32), rd[lo:hi].view(np.uint32)), (lo, hi)

    for i in range(6):
        check(i, i + 1)
    g.sync()          # the overflow bit was consumed, not left behind
    check(0, 3)
    g.sync()
    check(0, 200)
    g.sync()
    # "no latency walk" did not stick: coarse() takes the latency walk with its own redo launch
    ids, dist = g.coarse(q[:3], 16, EF)
    for i in range(3):
        rid, rdist = og.search_knn(q[i], EF, 16)
        assert np.array_equal(ids[i, :len(rid)], rid), i
        assert np.array_equal(dist[i, :len(rid)].view(np.uint32), np.asarray(rdist, np.float32).view(np.uint32))
    check(7, 8)
    if M == 16:
        assert g.last_scan_kernel() == "ivf_tail_kernel"
    g.sync()
    og.free()
