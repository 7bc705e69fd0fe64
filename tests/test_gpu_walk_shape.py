"""The walk's shaped instantiations (kernels_hnsw.hip: D / MAXM / MERGE as template constants, the loop over a query's
expansions peeled into a fill and a steady phase; the rule that picks them is csrc/walk_form.h) against the oracle's walk.

Every case is 512 queries at nprobe 32 and is walked twice on the device, once with the shaped form and once with
IVFHNSW_WALK_SHAPE=0 (the generic instantiation).  Both must equal the oracle -- ids, their order and the distance bits of
every query, no tolerance -- and therefore each other, which is asserted too.  The knobs are read once per process, so each
environment setting is one child process that walks all the cases; IVFHNSW_WALK_TAGW=10 with IVFHNSW_WALK_LATE_VISIT=1 makes
these small graphs take the form a million-node graph takes (10-bit tags, survivors entered late).  The graphs, the queries
and the oracle's answers are made once, here, and handed to the children in a file.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import synth
from oracle import orc
import test_gpu_walk_ties as ties

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, K = 512, 32
BIG = {"IVFHNSW_WALK_TAGW": "10", "IVFHNSW_WALK_LATE_VISIT": "1"}
SETTINGS = {"shaped": BIG, "generic": dict(BIG, IVFHNSW_WALK_SHAPE="0"),
            "shaped-nomerge": dict(BIG, IVFHNSW_WALK_MERGE="0"),
            "generic-nomerge": dict(BIG, IVFHNSW_WALK_MERGE="0", IVFHNSW_WALK_SHAPE="0")}

CHILD = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_pkg()
z = np.load(%(cases)r)
out = {}
for name in str(z["names"]).split(","):
    g = pkg.GpuIndex(0)
    g.upload_quantizer(z[name + ".counts"], z[name + ".links"], z[name + ".vectors"], int(z[name + ".ep"]))
    for ef in z[name + ".efs"]:
        ids, dist = g.coarse(z[name + ".q"], %(k)d, int(ef))
        out["%%s.%%d.ids" %% (name, ef)] = ids
        out["%%s.%%d.dist" %% (name, ef)] = dist
    g.close()
np.savez(%(out)r, **out)
print("WALKED", len(out))
'''


def _queries(rng, cents, spread):
    return (cents[rng.choice(len(cents), NQ)] + rng.normal(0, spread, size=(NQ, cents.shape[1]))).astype(np.float32)


def _with_degrees(graph, degrees, rng):
    """The graph with every third node's link list cut, or filled with further distinct ids, to one of `degrees`."""
    counts = graph.counts.copy()
    links = graph.links.copy().reshape(len(counts), -1)
    n, maxM = links.shape
    for i in range(0, n, 3):
        want = degrees[(i // 3) % len(degrees)]
        have = list(links[i, :counts[i]])
        while len(have) < want:
            c = int(rng.integers(0, n))
            if c != i and c not in have:
                have.append(c)
        links[i] = 0
        links[i, :want] = have[:want]
        counts[i] = want
    return orc.Hnsw.from_arrays(counts, links, graph.vectors, 16, graph.enterpoint)


def _make_cases():
    """name -> (graph, queries, efs)"""
    rng = np.random.default_rng(1201)
    cases = {}
    cents = synth.sift_like(rng, 2048, 128)
    graph = orc.Hnsw.build(cents, M=16, efConstruction=60)          # the insertion loop; maxM 32
    assert graph.maxM == 32
    q = _queries(rng, cents, 10.0)
    cases["base"] = (graph, q, (40, 80, 33))                         # NCH 1 and 2; ef 33: one expansion fills the set
    deg = _with_degrees(graph, (0, 1, 7, 8, 9, 32), rng)            # the count-in-key fetch boundaries
    assert set((0, 1, 7, 8, 9, 32)) <= set(int(c) for c in deg.counts)
    cases["degrees"] = (deg, q, (80,))
    far = q.copy()                                                   # a quarter outside the byte range, on both sides
    far[0:NQ:8] = q[0:NQ:8] * 3.0                                    # above it (x_hi)
    far[1:NQ:8] = q[1:NQ:8] - 4.0 * np.abs(q).mean()                 # below it (x_any alone)
    far[2:NQ:32] = 1.0e4
    far[3:NQ:32] = -1.0e4
    cases["far"] = (graph, far, (80,))
    deep = rng.normal(0, 1.0, size=(2048, 96))
    deep = (deep / np.linalg.norm(deep, axis=1, keepdims=True)).astype(np.float32)
    cases["d96"] = (orc.Hnsw.build(deep, M=16, efConstruction=60), _queries(rng, deep, 0.05), (80,))
    base = synth.sift_like(rng, 341, 128)                            # every centroid six times: ties at the ef boundary
    dup = np.concatenate([base] * 6)[rng.permutation(2046)]
    qd = _queries(rng, base, 5.0)
    qd[:64] = base[:64]
    cases["ties"] = (orc.Hnsw.build(dup, M=16, efConstruction=60), qd, (40, 80))
    counts, links, vec, ep = ties.build(70)                          # 72 tail entries: past the LDS tail, the redo form
    assert vec.shape[1] == 96 and links.shape[1] == 32
    cases["redo"] = (orc.Hnsw.from_arrays(counts, links, vec, 16, ep), ties.queries(NQ, 7), (80,))
    few = synth.sift_like(rng, 60, 128)                              # fewer than ef nodes: the steady loop is never entered
    cases["few"] = (orc.Hnsw.build(few, M=16, efConstruction=60), _queries(rng, few, 10.0), (80,))
    # shapes that must take the generic form (tests/test_walk_form_cpu.py has the rule) and stay equal
    m16 = orc.Hnsw.build(cents, M=8, efConstruction=60)
    assert m16.maxM == 16
    cases["maxm16"] = (m16, q, (80,))
    c64 = synth.sift_like(rng, 2048, 64)
    cases["d64"] = (orc.Hnsw.build(c64, M=16, efConstruction=60), _queries(rng, c64, 10.0), (80,))
    return cases


CASES = [("base", 40), ("base", 80), ("base", 33), ("degrees", 80), ("far", 80), ("d96", 80), ("ties", 40), ("ties", 80),
         ("redo", 80), ("few", 80), ("maxm16", 80), ("d64", 80)]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("walk_shape")
    cases = _make_cases()
    blob = {"names": ",".join(cases)}
    for name, (graph, q, efs) in cases.items():
        blob.update({name + ".counts": graph.counts, name + ".links": graph.links, name + ".vectors": graph.vectors,
                     name + ".ep": graph.enterpoint, name + ".q": q, name + ".efs": np.asarray(efs)})
    path = str(tmp / "cases.npz")
    np.savez(path, **blob)
    return {"cases": cases, "path": path, "tmp": tmp, "runs": {}, "refs": {}}


def _device(world, setting):
    """The results of all cases under one environment setting: one child process, started once."""
    if setting not in world["runs"]:
        out = str(world["tmp"] / (setting + ".npz"))
        r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, cases=world["path"], out=out, k=K)],
                           capture_output=True, text=True, env=dict(os.environ, **SETTINGS[setting]), timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        assert "WALKED" in r.stdout
        world["runs"][setting] = np.load(out)
    return world["runs"][setting]


def _oracle(world, name, ef):
    if (name, ef) not in world["refs"]:
        graph, q, _ = world["cases"][name]
        world["refs"][name, ef] = [graph.search_knn(x, ef, K) for x in q]
    return world["refs"][name, ef]


def _check(world, name, ef, settings):
    ref = _oracle(world, name, ef)
    got = [(_device(world, s)["%s.%d.ids" % (name, ef)], _device(world, s)["%s.%d.dist" % (name, ef)]) for s in settings]
    for s, (ids, dist) in zip(settings, got):
        assert ids.shape == (NQ, K)
        for i, (rid, rd) in enumerate(ref):
            n = len(rid)
            assert np.array_equal(ids[i, :n], rid), "%s, %s ef %d, query %d: ids differ" % (s, name, ef, i)
            assert np.array_equal(dist[i, :n].view(np.uint32), np.asarray(rd, np.float32).view(np.uint32)), \
                "%s, %s ef %d, query %d: distance bits differ" % (s, name, ef, i)
            assert (ids[i, n:] == 0xffffffff).all()
    for ids, dist in got[1:]:
        assert np.array_equal(ids, got[0][0]) and np.array_equal(dist.view(np.uint32), got[0][1].view(np.uint32))


@pytest.mark.parametrize("name,ef", CASES)
def test_shaped_and_generic_walks_equal_the_oracle(world, name, ef):
    _check(world, name, ef, ("shaped", "generic"))


@pytest.mark.parametrize("name,ef", [("base", 40), ("base", 80), ("ties", 80)])
def test_admissions_one_by_one(world, name, ef):
    """IVFHNSW_WALK_MERGE=0 picks the MERGE = false instantiation of the shaped form and stays exact."""
    _check(world, name, ef, ("shaped-nomerge", "generic-nomerge"))


def test_the_fixtures_reach_what_they_are_for(world):
    """The tie graphs do put ties at the ef boundary, the small graph has fewer than ef nodes, and the redo graph's answers
    contain the node that only a walk with the whole tail finds (tests/test_gpu_walk_ties.py)."""
    assert any(len(rid) == K and rd[-1] == rd[-2] for rid, rd in _oracle(world, "ties", 40))
    assert world["cases"]["few"][0].n < 80
    assert all(len(rid) == K for rid, _ in _oracle(world, "few", 80))
    assert all(6 in rid for rid, _ in _oracle(world, "redo", 80))
