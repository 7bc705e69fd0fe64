"""add_batch on a searched index through the class surface (IndexIVF_HNSW::add_batch, IndexIVF_HNSW.cpp:75-131): with
the device copy current the class appends the batch in HBM (ivfhnsw_gpu_add) instead of uploading the whole index at
the next search.  add, search, add more, search, as the reference's vector-add driver does: both ways give the same
labels and distance bits in every round and write the same .index file, and the last round finds the oracle's labels
on the lists add_batch builds."""
import os
import subprocess

import numpy as np
import pytest

import hostio
import synth
from test_gpu_append import _csr_append

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("append_tool") / "append_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "append_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
                    "-livfhnsw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_add_search_rounds_in_place_equal_reupload(tool, tmp_path):
    c = synth.make_corpus(seed=91, nc=128, d=128, M=16, n_base=9000, nq=48, efConstruction=80)
    p = hostio.dump_corpus(c, str(tmp_path))
    base = c["base"]
    bpath = str(tmp_path / "base.fvecs")
    hostio.write_xvecs(bpath, base)
    nq, k, nrounds, nprobe, max_codes, ef = len(c["queries"]), 10, 4, 16, 2000, 40
    res = {}
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    env.pop("IVFHNSW_SHARDS", None)
    for mode in ("inplace", "reupload"):
        out, idx = str(tmp_path / (mode + ".bin")), str(tmp_path / (mode + ".index"))
        args = [c["d"], c["nc"], c["code_size"], p["centroids"], p["info"], p["edges"], p["pq"], p["norm_pq"], bpath,
                nrounds, p["queries"], nq, k, nprobe, max_codes, ef, mode, out, idx]
        r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        raw = np.fromfile(out, np.uint8)
        lab = raw[:nrounds * nq * k * 8].view(np.int64).reshape(nrounds, nq, k)
        dist = raw[nrounds * nq * k * 8:].view(np.float32).reshape(nrounds, nq, k)
        res[mode] = (lab, dist, open(idx, "rb").read())
    (la, da, ia), (lb, db, ib) = res["inplace"], res["reupload"]
    assert np.array_equal(la, lb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert ia == ib, "the written indexes differ"
    nb = len(base)
    assert (la >= 0).all()
    assert (la[0] < nb // nrounds).all(), "round 0 can only find the first segment"
    assert (la[-1] >= nb // nrounds).any(), "the last round finds rows added later"
    # the oracle on the lists add_batch builds: its encode of every row, appended round by round
    nc = c["nc"]
    empty = dict(c, offsets=np.zeros(nc + 1, np.uint64), ids=np.zeros(0, np.uint32),
                 codes=np.zeros((0, c["code_size"]), np.uint8), norm_codes=np.zeros(0, np.uint8))
    ox = synth.oracle_index(empty)
    ox.set_params(nprobe, max_codes, ef)
    lists = (empty["offsets"], empty["ids"], empty["codes"], empty["norm_codes"])
    for r in range(nrounds):
        a, b = nb * r // nrounds, nb * (r + 1) // nrounds
        idx_, codes, ncodes, _ = ox.add_batch_encode(base[a:b])
        lists = _csr_append(lists, nc, idx_, np.arange(a, b, dtype=np.uint32), codes, ncodes)
    full = dict(c, offsets=lists[0], ids=lists[1], codes=lists[2], norm_codes=lists[3])
    of = synth.oracle_index(full)
    of.set_params(nprobe, max_codes, ef)
    ref_d, ref_l = of.search_batch(c["queries"], k=k)[:2]
    # the same k labels per query (the class reports distances on its own scale: one constant per query apart)
    assert np.array_equal(np.sort(la[-1], axis=1), np.sort(ref_l, axis=1))
