"""The walk's rejection bound (csrc/walk_bound.h: every row's own quantisation error, carried in the top nine bits of its
norm-table entry, and margins sized to the integer form at d <= 128) against the oracle's walk: ids, their order and the
distance bits of every query, no tolerance.  The filter only decides which float rows are READ, so any row it wrongly drops
shows as a differing answer.

Graphs of 4096 nodes, maxM 32, ef 80, 32 results, 256 queries a case.  Tables: byte-exact (integers 0..255, so every error
code is zero or covers a few ulps) with duplicate rows and rows one ulp off a duplicate in one component; exact rows with
1 % outliers half a step off in every component (the table-wide error is theirs, the other rows' codes are the smallest);
and the iid sift_like table.  d 128 and 96 take the shaped forms; d 32 (the generic instantiation, margins as they were) and
d 144 (the gather form: no norm table at all) must stay equal too.  Every case is walked in two child processes (the knobs
are read once per process): "big", IVFHNSW_WALK_TAGW=10 with IVFHNSW_WALK_LATE_VISIT=1, the form a million-node graph takes
(per-row errors), and "small", no knobs, the form without a norm table (the table-wide error, the sized margins alone).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import synth
from oracle import orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NQ, K, EF = 4096, 256, 32, 80
SETTINGS = {"big": {"IVFHNSW_WALK_TAGW": "10", "IVFHNSW_WALK_LATE_VISIT": "1"}, "small": {}}

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
    ids, dist = g.coarse(z[name + ".q"], %(k)d, %(ef)d)
    out[name + ".ids"] = ids
    out[name + ".dist"] = dist
    g.close()
np.savez(%(out)r, **out)
print("WALKED", len(out))
'''


def _exact(rng, n, d):
    """Integers 0..255 with both ends present: lo 0, step 1, every row its own byte row."""
    x = np.clip(np.rint(np.abs(rng.normal(0.0, 45.0, size=(n, d)))), 0, 255).astype(np.float32)
    x[0, 0], x[0, 1] = 0.0, 255.0
    return x


def _exact_with_duplicates(rng, d):
    """A quarter of N distinct rows; every row twice more as itself, once one ulp up and once one ulp down in one component."""
    base = _exact(rng, N // 4, d)
    x = np.concatenate([base, base, base, base])
    j = rng.integers(0, d, N // 4)
    r = np.arange(N // 4)
    x[2 * (N // 4) + r, j] = np.nextafter(np.maximum(base[r, j], 1.0), np.float32(np.inf))
    x[3 * (N // 4) + r, j] = np.nextafter(np.maximum(base[r, j], 1.0), np.float32(0.0))
    x = x[rng.permutation(N)]
    assert x.min() == 0.0 and x.max() == 255.0
    return x


def _outliers(rng, d):
    x = np.minimum(_exact(rng, N, d), 254.0)
    x[0, 1] = 255.0
    x[7::100] += 0.5
    x[7::100] = np.minimum(x[7::100], 255.0)
    return x.astype(np.float32)


def _queries(rng, rows, spread):
    q = (rows[rng.choice(len(rows), NQ)] + rng.normal(0, spread, size=(NQ, rows.shape[1]))).astype(np.float32)
    q[:32] = rows[rng.choice(len(rows), 32)]        # rows themselves: distance zero, ties among duplicates
    q[32:48] = q[32:48] * 3.0                       # above the byte range
    q[48:64] = q[48:64] - 4.0 * np.abs(q).mean()    # below it
    return q


def _make_cases():
    rng = np.random.default_rng(1401)
    cases = {}
    for d in (128, 96):
        for kind, rows in (("dups", _exact_with_duplicates(rng, d)), ("outliers", _outliers(rng, d)),
                           ("sift", synth.sift_like(rng, N, d))):
            cases["%s%d" % (kind, d)] = rows
    cases["sift32"] = synth.sift_like(rng, N, 32)    # generic instantiation
    cases["sift144"] = synth.sift_like(rng, N, 144)  # gather form
    out = {}
    for name, rows in cases.items():
        graph = orc.Hnsw.build(rows, M=16, efConstruction=60)
        assert graph.maxM == 32 and graph.n == N
        out[name] = (graph, _queries(rng, rows, 10.0))
    return out


CASES = ["dups128", "outliers128", "sift128", "dups96", "outliers96", "sift96", "sift32", "sift144"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("walk_bound")
    cases = _make_cases()
    assert list(cases) == CASES
    blob = {"names": ",".join(cases)}
    for name, (graph, q) in cases.items():
        blob.update({name + ".counts": graph.counts, name + ".links": graph.links, name + ".vectors": graph.vectors,
                     name + ".ep": graph.enterpoint, name + ".q": q})
    path = str(tmp / "cases.npz")
    np.savez(path, **blob)
    return {"cases": cases, "path": path, "tmp": tmp, "runs": {}, "refs": {}}


def _device(world, setting):
    """The results of all cases under one environment setting: one child process, started once."""
    if setting not in world["runs"]:
        out = str(world["tmp"] / (setting + ".npz"))
        r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, cases=world["path"], out=out, k=K, ef=EF)],
                           capture_output=True, text=True, env=dict(os.environ, **SETTINGS[setting]), timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        assert "WALKED" in r.stdout
        world["runs"][setting] = np.load(out)
    return world["runs"][setting]


def _oracle(world, name):
    if name not in world["refs"]:
        graph, q = world["cases"][name]
        world["refs"][name] = [graph.search_knn(x, EF, K) for x in q]
    return world["refs"][name]


@pytest.mark.parametrize("setting", ["big", "small"])
@pytest.mark.parametrize("name", CASES)
def test_walk_equals_the_oracle(world, name, setting):
    ref = _oracle(world, name)
    run = _device(world, setting)
    ids, dist = run[name + ".ids"], run[name + ".dist"]
    assert ids.shape == (NQ, K)
    for i, (rid, rd) in enumerate(ref):
        n = len(rid)
        assert n == K
        assert np.array_equal(ids[i, :n], rid), "%s, %s, query %d: ids differ" % (setting, name, i)
        assert np.array_equal(dist[i, :n].view(np.uint32), np.asarray(rd, np.float32).view(np.uint32)), \
            "%s, %s, query %d: distance bits differ" % (setting, name, i)


def test_the_tables_are_what_they_are_for(world):
    """The duplicate tables do put equal distances into the answers, and the outlier rows are 1 % of their table."""
    assert any(rd[j] == rd[j + 1] for _, rd in _oracle(world, "dups128") for j in range(K - 1))
    rows = world["cases"]["outliers128"][0].vectors.reshape(N, -1)
    off = (rows != np.rint(rows)).any(axis=1)
    assert 30 <= off.sum() <= 50 and off[7]
