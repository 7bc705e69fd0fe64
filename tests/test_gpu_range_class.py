"""Range search through the class surface (IndexIVF_HNSW::range_search) on IndexIVF_HNSW and
IndexIVF_HNSW_Grouping, without and with set_id_filter: the three arrays the method returns are compared exactly with
range_ref (the oracle's scored set; IVFADC also in scan order)."""
import os
import subprocess

import numpy as np
import pytest

import hostio
import range_ref
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("range_tool") / "range_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "range_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
                    "-livfhnsw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


CASES = {"ivf": (dict(seed=71, nc=128, d=128, M=16, n_base=8000, nq=32, efConstruction=80), 8, 1500, 32, False),
         "grouping": (dict(seed=73, nc=128, d=128, M=16, n_base=8000, nq=32, efConstruction=80, nsubc=8), 8, 700, 40, True)}


def _rounds(path, nq, n):
    raw = np.fromfile(path, np.uint8)
    out, at = [], 0
    for _ in range(n):
        lims = raw[at:at + 8 * (nq + 1)].view(np.uint64)
        at += 8 * (nq + 1)
        total = int(lims[-1])
        dist = raw[at:at + 4 * total].view(np.float32)
        at += 4 * total
        lab = raw[at:at + 8 * total].view(np.int64)
        at += 8 * total
        out.append((lims, dist, lab))
    assert at == len(raw)
    return out


@pytest.mark.parametrize("kind", ["ivf", "grouping"])
@pytest.mark.parametrize("quantile", [0.05, None], ids=["q05", "inf"])
def test_class_range_search(tool, tmp_path, kind, quantile):
    kw, nprobe, max_codes, ef, pruning = CASES[kind]
    c = synth.make_corpus(**kw)
    nq = len(c["queries"])
    sc = range_ref.scored_batch(c, c["queries"], nprobe, max_codes, ef, pruning, key=("class", kind))
    radius = np.float32(np.inf) if quantile is None else range_ref.pooled_quantile(sc, quantile)
    p = hostio.dump_corpus(c, str(tmp_path))
    allow = np.random.default_rng(3).choice(c["ids"], len(c["ids"]) // 3, replace=False).astype(np.uint32)
    lp = str(tmp_path / "labels.u32")
    allow.tofile(lp)
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    env.pop("IVFHNSW_SHARDS", None)
    out = str(tmp_path / "out.bin")
    args = [kind, c["d"], c["nc"], c["code_size"], c["nsubc"], p["centroids"], p["info"], p["edges"], p["pq"], p["norm_pq"],
            p["opq"], p["index"], p["queries"], nq, nprobe, max_codes, ef, int(pruning), int(radius.view(np.uint32)), lp, 0, out]
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    plain, filt, cleared = _rounds(out, nq, 3)
    assert plain[0][-1] > 0
    for i in range(nq):
        assert np.array_equal(range_ref.result_set(*plain, i), range_ref.expected_set(sc, i, radius)), i
    if kind == "ivf":
        assert range_ref.same_range(plain, range_ref.expected_ivf(c, sc, max_codes, radius))
    assert range_ref.same_range(filt, range_ref.filtered(plain, allow))
    assert 0 < filt[0][-1] < plain[0][-1] and np.isin(filt[2], allow).all()
    assert range_ref.same_range(cleared, plain)
