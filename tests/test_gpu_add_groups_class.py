"""add_group on a searched Grouping index through the class surface (IndexIVF_HNSW_Grouping::add_group,
IndexIVF_HNSW_Grouping.cpp:43-157): with the device copy current the class installs a new group in HBM
(ivfhnsw_gpu_add_groups) instead of uploading the whole index at the next search, and the table passes
the vector-add driver runs after its adds (compute_centroid_norms, compute_inter_centroid_dists) re-send at most their
own table.  Add a quarter of the groups, run the passes, search, and again: both ways give the same labels and distance
bits in every round -- also in a search BETWEEN add_group and the passes -- and write the same .index file; the last
round finds the oracle's labels on the index add_group builds; and the class counts one full upload against one per
search."""
import os
import subprocess

import numpy as np
import pytest

import hostio
import synth
from test_gpu_add_groups import _assemble, _assign

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("add_groups_tool") / "add_groups_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "add_groups_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
                    "-livfhnsw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("pruning", [0, 1], ids=["plain", "pruning"])
def test_add_group_rounds_in_place_equal_reupload(tool, tmp_path, pruning):
    c = synth.make_corpus(seed=97, nc=128, d=128, M=16, n_base=9000, nq=48, efConstruction=80, nsubc=8)
    p = hostio.dump_corpus(c, str(tmp_path))
    base = c["base"]
    bpath, apath = str(tmp_path / "base.fvecs"), str(tmp_path / "assign.u32")
    hostio.write_xvecs(bpath, base)
    assign = _assign(c).astype(np.uint32)
    assign.tofile(apath)
    nq, k, nrounds, nprobe, max_codes, ef = len(c["queries"]), 10, 4, 16, 2000, 80
    res = {}
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    env.pop("IVFHNSW_SHARDS", None)
    for mode in ("inplace", "reupload"):
        out, idx = str(tmp_path / (mode + ".bin")), str(tmp_path / (mode + ".index"))
        args = [c["d"], c["nc"], c["code_size"], c["nsubc"], p["centroids"], p["info"], p["edges"], p["pq"], p["norm_pq"],
                bpath, apath, nrounds, p["queries"], nq, k, nprobe, max_codes, ef, pruning, mode, out, idx]
        r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        raw = np.fromfile(out, np.uint8)
        nblk = nrounds + 1
        lab = raw[:nblk * nq * k * 8].view(np.int64).reshape(nblk, nq, k)
        dist = raw[nblk * nq * k * 8:].view(np.float32).reshape(nblk, nq, k)
        uploads = int(r.stdout.split("full_uploads")[1].split()[0])
        res[mode] = (lab, dist, open(idx, "rb").read(), uploads)
    (la, da, ia, ua), (lb, db, ib, ub) = res["inplace"], res["reupload"]
    assert np.array_equal(la, lb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert ia == ib, "the written indexes differ"
    # the in-place path was taken: everything went up once (the first search), against once per search
    assert ua == 1 and ub == nrounds + 1
    nc = c["nc"]
    first = set(np.nonzero(assign < nc // nrounds)[0].tolist())
    assert (la[-2] >= 0).all()
    assert all(int(x) in first for x in la[0][la[0] >= 0]), "round 0 can only find the first quarter of the groups"
    assert any(int(x) not in first for x in la[-2].ravel()), "the last round finds rows added later"
    assert not np.array_equal(la[nrounds], la[0])      # the search in between already sees round 1's groups
    # the oracle on the index add_group builds (its add_group_encode per group, the tool's efSearch)
    groups = {cc: (np.ascontiguousarray(base[assign == cc]), np.nonzero(assign == cc)[0].astype(np.uint32))
              for cc in range(nc)}
    full = _assemble(c, c["graph"], groups)
    of = synth.oracle_index(full)
    of.set_params(nprobe, max_codes, ef, do_pruning=bool(pruning))
    ref_l = of.search_batch(c["queries"], k=k)[1].reshape(nq, k)
    # the same k labels per query (the class reports distances on its own scale: one constant per query apart)
    assert np.array_equal(np.sort(la[nrounds - 1], axis=1), np.sort(ref_l, axis=1))
