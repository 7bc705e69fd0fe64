"""update_batch on a searched index through the class surface (IndexIVF_HNSW::update_batch): with the device
copy current the class changes the host lists as remove_ids + add_batch would and the device lists by one
ivfhnsw_gpu_upsert_ivf.  A twin that runs remove_ids followed by add_batch gives the same labels and distance bits in every
round and writes the same .index file, which holds upsert_ref's lists; the search after invalidate_device() (the host lists
uploaded again) equals the one on the device copy changed in place; a repeated label throws and changes nothing; a
Grouping index refuses."""
import os
import subprocess

import numpy as np
import pytest

import hostio
import synth
import upsert_ref
from oracle import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = dict(seed=91, nc=128, d=128, M=16, n_base=9000, nq=48, efConstruction=80)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("upsert_tool") / "upsert_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "upsert_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
                    "-livfhnsw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_update_batch_equals_remove_then_add(tool, tmp_path):
    c = synth.make_corpus(**CASE)
    p = hostio.dump_corpus(c, str(tmp_path))
    rng = np.random.default_rng(6)
    nq, k, nprobe, max_codes, ef = len(c["queries"]), 10, 16, 2000, 40
    n = 1500
    off = c["offsets"].astype(np.int64)
    big = int(np.argmax(np.diff(off)))
    resident = np.union1d(rng.choice(c["ids"], n // 2, replace=False), c["ids"][off[big]:off[big + 1]])   # one list replaced whole
    labels = rng.permutation(np.concatenate([resident, np.arange(10 ** 6, 10 ** 6 + n // 2)]).astype(np.uint32))
    x = (c["base"][rng.integers(0, len(c["base"]), len(labels))] + rng.normal(0, 3.0, (len(labels), c["d"]))).astype(np.float32)
    xpath, lpath = str(tmp_path / "new.fvecs"), str(tmp_path / "labels.u32")
    hostio.write_xvecs(xpath, x)
    labels.tofile(lpath)
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    env.pop("IVFHNSW_SHARDS", None)
    res = {}
    for mode in ("update", "pair"):
        out, idx = str(tmp_path / (mode + ".bin")), str(tmp_path / (mode + ".index"))
        args = ["search", c["d"], c["nc"], c["code_size"], p["centroids"], p["info"], p["edges"], p["pq"], p["norm_pq"], p["opq"],
                p["index"], p["queries"], nq, k, nprobe, max_codes, ef, xpath, lpath, mode, out, idx]
        r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        raw = np.fromfile(out, np.uint8)
        nb = 4 * nq * k
        lab = raw[:nb * 8].view(np.int64).reshape(4, nq, k)
        dist = raw[nb * 8:nb * 12].view(np.float32).reshape(4, nq, k)
        res[mode] = (lab, dist, raw[nb * 12:].view(np.uint64), open(idx, "rb").read())
    (la, da, ta, ia), (lb, db, tb, ib) = res["update"], res["pair"]
    assert np.array_equal(la, lb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert ta[0] == tb[0] == len(resident)
    assert ta[1] == 1, "a repeated label did not throw std::invalid_argument"
    assert ia == ib, "the written indexes differ"
    # the update changed the answers; the refused call changed nothing; the device copy changed in place answers as the
    # host lists uploaded again
    assert not np.array_equal(la[0], la[1])
    for r in (2, 3):
        assert np.array_equal(la[1], la[r]) and np.array_equal(da[1].view(np.uint32), da[r].view(np.uint32)), r
    # the lists the class should hold
    ox = synth.oracle_index(c)
    ox.set_params(nprobe, max_codes, ef)
    idx_, codes, ncodes, _ = ox.add_batch_encode(x)
    fc, _ = upsert_ref.upserted_corpus(c, idx_, labels, codes, ncodes)
    written = orc.read_index(str(tmp_path / "update.index"), False)
    for key in ("offsets", "ids", "codes", "norm_codes"):
        assert np.array_equal(written[key], np.asarray(fc[key]).reshape(written[key].shape)), key
    ref_l = synth.oracle_index(fc)
    ref_l.set_params(nprobe, max_codes, ef)
    assert np.array_equal(np.sort(la[1], axis=1), np.sort(ref_l.search_batch(c["queries"], k=k)[1], axis=1))


def test_grouping_refuses(tool):
    r = subprocess.run([tool, "refused", "128", "64", "16", "8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "IndexIVF_HNSW_Grouping::update_batch" in r.stdout
