"""A split call (two uneven parts on two streams, capi_search.cpp search_dev_split) builds both parts' ADC tables on a
third stream beside the walks, and each part then runs plan and scan behind its walk and meets its tables in front of
the scan.  Nothing about the results may move: every comparison here is torch.equal on labels and on distance BITS,
against the same call in one part (set_batch_split(0)) and against the oracle on the first 512 queries.

nq = 8195: the first part gets 6147 queries, which is no multiple of the table kernel's four queries per workgroup, and
the second part's tables start at query 6147 of the batch.  (The second part itself is whole rounds of the scan's
resident workgroups by construction -- 2048 here -- so it cannot be given an odd count.)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import corpus
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NQ = 8195
_EARLY_ON = os.environ.get("IVFHNSW_EARLY_LUT", "1") != "0" and os.environ.get("IVFHNSW_PLAN_LUT", "1") != "0"
PARAMS = (16, 2500, 40)  # nprobe, max_codes, efSearch


def _corpus(M=16, opq=False):
    return corpus(seed=81, nc=256, d=128, M=M, n_base=20000, nq=NQ, efConstruction=60, opq=opq)


def _upload(g, c):
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"], opq_A=c["opq_A"])
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)


def _search_dev(g, d_q, k):
    """One search_dev call on the handle's stream: (distances, labels) as device tensors, no synchronisation."""
    import torch
    nq = d_q.shape[0]
    dd = torch.full((nq, k), -1.0, dtype=torch.float32, device=d_q.device)
    ll = torch.full((nq, k), -7, dtype=torch.int64, device=d_q.device)
    nprobe, max_codes, ef = PARAMS
    g.search_dev(nq, k, d_q, dd, ll, nprobe, max_codes, efSearch=ef)
    return dd, ll


def _same(a, b):
    import torch
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def _both_forms(gpu, c, k):
    """The default split call and the same call in one part, on one handle bound to torch's current stream."""
    import torch
    g = gpu()
    _upload(g, c)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    d_q = torch.from_numpy(c["queries"]).to(torch.device("cuda", 0))
    two = _search_dev(g, d_q, k)
    parts = g.last_batch_parts()
    g.set_batch_split(0)
    one = _search_dev(g, d_q, k)
    assert g.last_batch_parts() == (NQ, 0)
    torch.cuda.current_stream().synchronize()
    return two, one, parts


@pytest.mark.parametrize("M,opq", [(16, False), (16, True), (8, False)], ids=["pq16", "pq16-opq", "pq8-dsub16"])
def test_split_call_with_early_tables_equals_one_part_and_oracle(gpu, M, opq):
    """IVFADC, k = 1.  The OPQ case fails if the tables are built from unrotated queries; PQ8 gives dsub 16."""
    import torch
    c = _corpus(M=M, opq=opq)
    two, one, parts = _both_forms(gpu, c, 1)
    assert parts[1] > 0 and parts[0] + parts[1] == NQ and parts[0] % 4 != 0
    assert _same(two, one)
    ox = synth.oracle_index(c)
    ox.set_params(*PARAMS, do_pruning=False)
    ref_d, ref_l, _, _, _ = ox.search_batch(c["queries"][:512], k=1)
    assert torch.equal(two[1][:512].cpu(), torch.from_numpy(ref_l.reshape(512, 1).astype(np.int64)))
    assert torch.equal(two[0][:512].cpu().view(torch.int32),
                       torch.from_numpy(np.ascontiguousarray(ref_d.reshape(512, 1)).view(np.int32)))


def test_split_call_k10_ascending(gpu):
    """k = 10, not heap order: this call takes the split as well."""
    c = _corpus()
    two, one, parts = _both_forms(gpu, c, 10)
    assert parts[1] > 0
    assert _same(two, one)
    ox = synth.oracle_index(c)
    ox.set_params(*PARAMS, do_pruning=False)
    ref_d, ref_l, _, _, _ = ox.search_batch(c["queries"][:512], k=10)
    o = np.argsort(ref_d, axis=1, kind="stable")
    ref_ds = np.take_along_axis(ref_d, o, 1)
    ref_ls = np.take_along_axis(ref_l, o, 1)
    dev_d = two[0][:512].cpu().numpy()
    dev_l = two[1][:512].cpu().numpy()
    assert np.array_equal(dev_d.view(np.uint32), ref_ds.view(np.uint32))
    untied = np.all(np.diff(ref_ds, axis=1) > 0, axis=1)  # equal distances may stand in either order
    assert untied.sum() > 256 and np.array_equal(dev_l[untied], ref_ls[untied])


def test_calls_back_to_back_and_on_another_stream(gpu):
    """Two calls with different queries and nothing between them, then one on another torch stream: a table buffer
    rewritten while a scan still reads it, or a join that misses the helper stream, shows as a wrong result."""
    import torch
    c = _corpus()
    dev = torch.device("cuda", 0)
    g = gpu()
    _upload(g, c)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    q = torch.from_numpy(c["queries"]).to(dev)
    qs = [q, q.flip(0).contiguous(), q.roll(1234, 0).contiguous()]
    g.set_batch_split(0)
    ones = [_search_dev(g, x, 1) for x in qs]
    torch.cuda.current_stream().synchronize()
    g.set_batch_split(1000)
    a = _search_dev(g, qs[0], 1)
    b = _search_dev(g, qs[1], 1)
    assert g.last_batch_parts()[1] > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g.set_stream(side.cuda_stream)
    with torch.cuda.stream(side):
        cc = _search_dev(g, qs[2], 1)
        # read through the side stream only: the whole call, helper stream included, must be behind it
        cc_host = (cc[0].cpu(), cc[1].cpu())
    assert _same(a, ones[0]) and _same(b, ones[1])
    assert _same(cc_host, (ones[2][0].cpu(), ones[2][1].cpu()))
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    assert not _same(a, b)  # the three batches really differ


@pytest.mark.parametrize("level", [1, 2])
def test_stage_accounting_of_a_split_call(gpu, level):
    """The scan is bracketed twice per call (one launch per part) at both levels; the walk as today: once per part at
    level 1, not at all at level 2.  At level 1 the table launches (helper stream) and the plan launches are bracketed too."""
    import torch
    c = _corpus()
    g = gpu()
    _upload(g, c)
    d_q = torch.from_numpy(c["queries"]).to(torch.device("cuda", 0))
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    plain = _search_dev(g, d_q, 1)
    g.set_profiling(level)
    g.reset_stage_ms()
    calls = 3
    outs = [_search_dev(g, d_q, 1) for _ in range(calls)]
    assert g.last_batch_parts()[1] > 0
    torch.cuda.current_stream().synchronize()
    st = g.stage_ms()
    g.set_profiling(0)
    assert st["scan"][1] == 2 * calls and st["scan"][0] > 0.0
    if level == 1:
        assert st["coarse"][1] == 2 * calls and st["coarse"][0] > 0.0
        assert st["lut"][1] == 2 * calls and st["lut"][0] > 0.0
        # (with a knob set to 0, plan and tables go in one launch behind each walk, accounted as the table stage)
        assert st["plan"][1] == (2 * calls if _EARLY_ON else 0)
    else:
        assert st["coarse"][1] == 0 and st["lut"][1] == 0 and st["plan"][1] == 0
    assert all(_same(o, plain) for o in outs)


def test_early_tables_only_where_the_second_walk_leaves_slots(gpu):
    """A second part of 2048 queries leaves half of the walk's 4096 resident wavefront slots to the table workgroups: the
    tables are early and each part launches its plan alone.  A scan-heavy call whose second part is 4096 queries fills every
    slot: it keeps plan and tables in one launch behind each walk (accounted as the table stage), as before."""
    if os.environ.get("IVFHNSW_SPLIT"):
        pytest.skip("IVFHNSW_SPLIT fixes the share")
    c = corpus(seed=73, nc=256, d=128, M=16, n_base=100000, nq=9000, efConstruction=60)
    g = gpu()
    _upload(g, c)
    g.set_profiling(1)
    for (nprobe, max_codes, ef), second, early in (((8, 200, 120), 2048, _EARLY_ON), ((64, 60000, 64), 4096, False)):
        g.reset_stage_ms()
        g.search(c["queries"], 1, nprobe, max_codes, efSearch=ef)
        assert g.last_batch_parts() == (9000 - second, second)
        st = g.stage_ms()
        assert st["lut"][1] == 2 and st["scan"][1] == 2
        assert st["plan"][1] == (2 if early else 0)
    g.set_profiling(0)


CHILD = r'''
import hashlib, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import __graft_entry__ as ge
import synth
pkg = ge.load_pkg()
h = hashlib.sha256()
for opq in (False, True):
    c = synth.make_corpus(seed=83, nc=256, d=128, M=16, n_base=20000, nq=8195, efConstruction=60, opq=opq)
    g = pkg.GpuIndex(0)
    g.upload_ivf(c["d"], c["code_size"], c["offsets"], c["ids"], c["codes"], c["norm_codes"], c["centroid_norms"],
                 c["pq_centroids"], c["norm_table"], opq_A=c["opq_A"])
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    for k in (1, 10):
        dist, lab = g.search(c["queries"], k, 16, 2500, efSearch=40)
        assert g.last_batch_parts()[1] > 0
        h.update(dist.tobytes()); h.update(lab.tobytes())
print("DIGEST", h.hexdigest())
'''


def _run(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT)], capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("DIGEST")]
    assert line, r.stdout[-500:]
    return line[0]


def test_knob_restores_the_launches_behind_the_walk():
    """IVFHNSW_EARLY_LUT is read once per process: 0 (plan and tables in one launch behind each walk) and 1 (tables
    beside the walks) in a child process each, one digest."""
    assert _run({"IVFHNSW_EARLY_LUT": "0"}) == _run({"IVFHNSW_EARLY_LUT": "1"})
