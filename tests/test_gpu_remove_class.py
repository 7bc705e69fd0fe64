"""remove_ids on a searched index through the class surface (IndexIVF_HNSW::remove_ids): with the device
copy current the class removes the codes in HBM (ivfhnsw_gpu_remove_ids) and filters only the host lists that changed;
after invalidate_device() it filters every list on the host and uploads the index again at the next search.  search,
remove, search, add (IVFADC), remove, search, write: both ways give the same labels and distance bits in every round and
write the same .index file, which holds the filtered lists, and the last round finds the oracle's labels on them."""
import os
import subprocess

import numpy as np
import pytest

import hostio
import remove_ref
import synth
from oracle import orc
from test_gpu_append import _csr_append

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("remove_tool") / "remove_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "remove_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
                    "-livfhnsw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


CASES = {"ivf": dict(seed=91, nc=128, d=128, M=16, n_base=9000, nq=48, efConstruction=80),
         "grouping": dict(seed=92, nc=128, d=128, M=16, n_base=9000, nq=48, efConstruction=80, nsubc=16)}


@pytest.mark.parametrize("kind", ["ivf", "grouping"])
def test_remove_search_rounds_in_place_equal_reupload(tool, tmp_path, kind):
    c = synth.make_corpus(**CASES[kind])
    p = hostio.dump_corpus(c, str(tmp_path))
    rng = np.random.default_rng(5)
    nq, k, nprobe, max_codes, ef, pruning = len(c["queries"]), 10, 16, 2000, 40, kind == "grouping"
    lab1 = rng.choice(c["ids"], 2000, replace=False).astype(np.uint32)
    off = c["offsets"].astype(np.int64)
    big = int(np.argmax(np.diff(off)))
    lab1 = np.concatenate([lab1, c["ids"][off[big]:off[big + 1]]])     # one list emptied
    add_first = 10 ** 6
    if kind == "ivf":
        xadd = c["base"][:1500] + np.float32(0.5)
        apath = str(tmp_path / "add.fvecs")
        hostio.write_xvecs(apath, xadd)
    else:
        xadd, apath = None, "-"
    left = np.setdiff1d(c["ids"], lab1)
    lab2 = rng.choice(left, 1000, replace=False).astype(np.uint32)
    if xadd is not None:
        lab2 = np.concatenate([lab2, np.arange(add_first, add_first + 200, dtype=np.uint32)])
    l1p, l2p = str(tmp_path / "l1.u32"), str(tmp_path / "l2.u32")
    lab1.astype(np.uint32).tofile(l1p)
    lab2.astype(np.uint32).tofile(l2p)
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    env.pop("IVFHNSW_SHARDS", None)
    res = {}
    for mode in ("inplace", "reupload"):
        out, idx = str(tmp_path / (mode + ".bin")), str(tmp_path / (mode + ".index"))
        args = ["search", kind, c["d"], c["nc"], c["code_size"], c["nsubc"], p["centroids"], p["info"], p["edges"],
                p["pq"], p["norm_pq"], p["opq"], p["index"], p["queries"], nq, k, nprobe, max_codes, ef, int(pruning),
                l1p, l2p, apath, add_first, mode, out, idx]
        r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        raw = np.fromfile(out, np.uint8)
        nb = 3 * nq * k
        lab = raw[:nb * 8].view(np.int64).reshape(3, nq, k)
        dist = raw[nb * 8:nb * 12].view(np.float32).reshape(3, nq, k)
        removed = raw[nb * 12:].view(np.uint64)
        res[mode] = (lab, dist, removed, open(idx, "rb").read())
    (la, da, ra, ia), (lb, db, rb, ib) = res["inplace"], res["reupload"]
    assert np.array_equal(la, lb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert np.array_equal(ra, rb)
    assert ia == ib, "the written indexes differ"
    # the lists the class should hold: filter, append add_batch's encode of the new rows, filter again
    fc, f1 = remove_ref.filtered_corpus(c, lab1)
    assert ra[0] == f1["removed"].sum()
    assert not np.isin(la[1], lab1).any() and not np.isin(la[2], lab1).any()
    if xadd is not None:
        ox = synth.oracle_index(fc)
        ox.set_params(nprobe, max_codes, ef)
        idx_, codes, ncodes, _ = ox.add_batch_encode(xadd)
        ids = np.arange(add_first, add_first + len(xadd), dtype=np.uint32)
        cur = _csr_append((fc["offsets"], fc["ids"], fc["codes"], fc["norm_codes"]), c["nc"], idx_, ids, codes, ncodes)
        fc = dict(fc, offsets=cur[0], ids=cur[1], codes=cur[2], norm_codes=cur[3])
    final, f2 = remove_ref.filtered_corpus(fc, lab2)
    assert ra[1] == f2["removed"].sum()
    written = orc.read_index(str(tmp_path / "inplace.index"), kind == "grouping")
    for key in ("offsets", "ids", "codes", "norm_codes"):
        assert np.array_equal(written[key], final[key]), key
    if kind == "grouping":
        assert np.array_equal(written["subgroup_sizes"], final["subgroup_sizes"])
    of = synth.oracle_index(final)
    of.set_params(nprobe, max_codes, ef, do_pruning=pruning)
    ref_l = of.search_batch(c["queries"], k=k)[1]
    # the same k labels per query (the class reports distances on its own scale: one constant per query apart)
    assert np.array_equal(np.sort(la[2], axis=1), np.sort(ref_l, axis=1))
