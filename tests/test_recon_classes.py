"""Reconstruction through the class surface (IndexIVF_HNSW::reconstruct_labels / search_and_reconstruct)
on IndexIVF_HNSW (with OPQ) and IndexIVF_HNSW_Grouping: a driver compiled against the installed headers and libraries
must return what the C ABI returns on an upload of the same index, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import corpus
import hostio
from test_gpu_remove import _upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("recon_tool") / "recon_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "recon_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
                    "-livfhnsw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


CASES = {"ivf": (dict(seed=81, nc=128, d=96, M=12, n_base=9000, nq=48, efConstruction=60, opq=True), 8, 1500, 32, False),
         "grouping": (dict(seed=73, nc=128, d=128, M=16, n_base=8000, nq=32, efConstruction=80, nsubc=8), 8, 700, 40, True)}
K = 10


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("kind", ["ivf", "grouping"])
def test_class_reconstruction_equals_the_c_abi(gpu, pkg, tool, tmp_path, kind):
    kw, nprobe, max_codes, ef, pruning = CASES[kind]
    c = corpus(**kw)
    d, nq = c["d"], len(c["queries"])
    labels = np.concatenate([c["ids"][::97], [len(c["ids"]) + 5, 0xffffffff]]).astype(np.uint32)
    p = hostio.dump_corpus(c, str(tmp_path))
    lp = str(tmp_path / "labels.u32")
    labels.tofile(lp)
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    env.pop("IVFHNSW_SHARDS", None)
    out = str(tmp_path / "out.bin")
    args = [kind, d, c["nc"], c["code_size"], c["nsubc"], p["centroids"], p["info"], p["edges"], p["pq"], p["norm_pq"],
            p["opq"], p["index"], p["queries"], nq, K, nprobe, max_codes, ef, int(pruning), lp, out]
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = np.fromfile(out, np.uint8)
    at = 0

    def take(dtype, *shape):
        nonlocal at
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = raw[at:at + n].view(dtype).reshape(shape)
        at += n
        return a

    by_label = take(np.float32, len(labels), d)
    dist, lab, rec = take(np.float32, nq, K), take(np.int64, nq, K), take(np.float32, nq, K, d)
    dist1, lab1, rec1 = take(np.float32, K), take(np.int64, K), take(np.float32, K, d)
    assert at == len(raw)

    g = _upload(gpu(), c)
    want, missing = g.reconstruct(labels, pkg.RECON_ORIGINAL)
    assert missing == 2 and same(by_label, want)
    assert np.isnan(by_label[-2:]).all() and not np.isnan(by_label[:-2]).any()
    ref = g.search_reconstruct(c["queries"], K, nprobe, max_codes, efSearch=ef, do_pruning=pruning, heap_order=True)
    assert same(dist, ref[0]) and same(lab, ref[1]) and same(rec, ref[3])
    assert same(dist1, ref[0][0]) and same(lab1, ref[1][0]) and same(rec1, ref[3][0])
    assert (lab >= 0).any()
