"""searchDisk through the class surface (IndexIVF_HNSW_Grouping::searchDisk, IndexIVF_HNSW_Grouping.cpp:365-395): the
host loop over the base file and the device re-rank -- loaded by upload_base(), or by IVFHNSW_RERANK=device at the first
call -- give the same labels and distance bits, with and without OPQ, and searchDisk_batch(kc = 0) equals nq searchDisk
calls.  Queries are integer-valued, as SIFT's are: every distance is then an exact integer, so the reference's cmp order
(distances within 0.001 are equal, utils.cpp:193-201) and the device's (distance, label) order coincide."""
import os
import subprocess

import numpy as np
import pytest

import hostio
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rerank_tool") / "rerank_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "rerank_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
                    "-livfhnsw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _run(tool, p, c, nq, k, base_path, mode, out, nprobe=8, max_codes=1500, ef=40, pruning=True):
    env = dict(os.environ)
    env.pop("IVFHNSW_RERANK", None)
    if mode == "env":
        env["IVFHNSW_RERANK"] = "device"
    env.setdefault("OMP_NUM_THREADS", "8")
    args = [c["d"], c["nc"], c["code_size"], c["nsubc"], p["centroids"], p["info"], p["edges"], p["pq"], p["norm_pq"],
            p["opq"], p["index"], p["queries"], nq, k, nprobe, max_codes, ef, int(pruning), base_path, mode, out]
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = np.fromfile(out, np.uint8)
    lab = raw[:2 * nq * k * 8].view(np.int64).reshape(2, nq, k)
    dist = raw[2 * nq * k * 8:].view(np.float32).reshape(2, nq, k)
    return lab, dist


@pytest.mark.parametrize("opq", [False, True])
def test_searchDisk_on_the_device_equals_the_host_loop(tool, tmp_path, opq):
    c = synth.make_corpus(seed=83 + opq, nc=128, d=128, M=16, n_base=8000, nq=24, efConstruction=80, nsubc=8, opq=opq)
    q = np.clip(np.rint(c["queries"]), 0, 255).astype(np.float32)
    p = hostio.dump_corpus(c, str(tmp_path), queries=q)
    base = np.clip(np.rint(c["base"]), 0, 255).astype(np.uint8)
    img = np.empty((len(base), c["d"] + 4), np.uint8)
    img[:, :4] = np.frombuffer(np.int32(c["d"]).tobytes(), np.uint8)
    img[:, 4:] = base
    bpath = str(tmp_path / "base.bvecs")
    img.tofile(bpath)
    nq = len(q)
    for k in (1, 10, 100):
        res = {m: _run(tool, p, c, nq, k, bpath, m, str(tmp_path / ("%s_%d.bin" % (m, k)))) for m in ("host", "device", "env")}
        hl, hd = res["host"]
        assert (hl[0] >= 0).any()
        for m in ("device", "env"):
            ml, md = res[m]
            assert np.array_equal(ml, hl), (m, k)
            assert np.array_equal(md.view(np.uint32), hd.view(np.uint32)), (m, k)
        for m in ("host", "device", "env"):  # searchDisk_batch(kc = 0) == nq searchDisk calls
            ml, md = res[m]
            assert np.array_equal(ml[0], ml[1]) and np.array_equal(md[0].view(np.uint32), md[1].view(np.uint32)), (m, k)
        # ascending by exact distance, padded at the end
        d0 = hd[0]
        assert (np.diff(d0, axis=1) >= 0).all()
