"""The label filter through the class surface (IndexIVF_HNSW::set_id_filter / clear_id_filter): search,
set_id_filter, search, add_batch (IVFADC), search, invalidate_device(), search, clear_id_filter, search, write.  Every round
finds the oracle's labels on the matching poisoned corpus (filter_ref), and the written .index file holds the lists as
they are, whatever the filter."""
import os
import subprocess

import numpy as np
import pytest

import filter_ref
import hostio
import synth
from oracle import orc
from test_gpu_append import _csr_append

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_tool") / "filter_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filter_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
                    "-livfhnsw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


CASES = {"ivf": dict(seed=91, nc=128, d=128, M=16, n_base=9000, nq=48, efConstruction=80),
         "grouping": dict(seed=92, nc=128, d=128, M=16, n_base=9000, nq=48, efConstruction=80, nsubc=16)}


@pytest.mark.parametrize("kind,deny", [("ivf", False), ("ivf", True), ("grouping", False)])
def test_filter_rounds_equal_the_oracle(tool, tmp_path, kind, deny):
    b = filter_ref.clipped(synth.make_corpus(**CASES[kind]))
    p = hostio.dump_corpus(b, str(tmp_path))
    rng = np.random.default_rng(7)
    nq, k, nprobe, max_codes, ef, pruning = len(b["queries"]), 10, 16, 2000, 40, kind == "grouping"
    add_first = 10 ** 6
    cur = b
    new_ids = np.zeros(0, np.uint32)
    new_pass = np.zeros(0, bool)
    if kind == "ivf":
        xadd = b["base"][:1500] + np.float32(0.5)
        apath = str(tmp_path / "add.fvecs")
        hostio.write_xvecs(apath, xadd)
        ox = synth.oracle_index(b)
        ox.set_params(nprobe, max_codes, ef)
        idx_, codes, ncodes, _ = ox.add_batch_encode(xadd)
        new_ids = np.arange(add_first, add_first + len(xadd), dtype=np.uint32)
        lists = _csr_append((b["offsets"], b["ids"], b["codes"], b["norm_codes"]), b["nc"], idx_, new_ids, codes, ncodes)
        cur = dict(b, offsets=lists[0], ids=lists[1], codes=lists[2], norm_codes=lists[3])
        # half of the new rows pass; one whose norm code is 255 cannot be told from a poisoned row, so it does not pass
        new_pass = (np.arange(len(xadd)) % 2 == 0) & (ncodes != 255)
    old_pass = rng.random(len(b["ids"])) < 0.3
    passing_ids = np.concatenate([b["ids"][old_pass], new_ids[new_pass]]).astype(np.uint32)
    denied_ids = np.concatenate([b["ids"][~old_pass], new_ids[~new_pass]]).astype(np.uint32)
    labels = denied_ids if deny else passing_ids
    lp = str(tmp_path / "labels.u32")
    labels.tofile(lp)
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    env.pop("IVFHNSW_SHARDS", None)
    out, idx = str(tmp_path / "out.bin"), str(tmp_path / "out.index")
    args = [kind, b["d"], b["nc"], b["code_size"], b["nsubc"], p["centroids"], p["info"], p["edges"], p["pq"], p["norm_pq"],
            p["opq"], p["index"], p["queries"], nq, k, nprobe, max_codes, ef, int(pruning), lp, int(deny), apath if kind == "ivf"
            else "-", add_first, out, idx]
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = np.fromfile(out, np.uint8)
    nb = 5 * nq * k
    lab = raw[:nb * 8].view(np.int64).reshape(5, nq, k)
    dist = raw[nb * 8:nb * 12].view(np.float32).reshape(5, nq, k)
    want = [b, filter_ref.poisoned(b, filter_ref.passing(b["ids"], passing_ids)),
            filter_ref.poisoned(cur, filter_ref.passing(cur["ids"], passing_ids)), None, cur]
    want[3] = want[2]
    for rnd, corpus_ in enumerate(want):
        ox = synth.oracle_index(corpus_)
        ox.set_params(nprobe, max_codes, ef, do_pruning=pruning)
        ref_l = ox.search_batch(b["queries"], k=k)[1]
        # the same k labels per query (the class reports distances on its own scale: one constant per query apart)
        assert np.array_equal(np.sort(lab[rnd], axis=1), np.sort(ref_l, axis=1)), rnd
        assert (dist[rnd][lab[rnd] < 0] == FLT_MAX).all(), rnd
        if rnd in (1, 2, 3):
            got = lab[rnd][lab[rnd] >= 0]
            assert np.isin(got, passing_ids).all() and len(got) > 0, rnd
    assert not np.array_equal(lab[0], lab[1]) and np.array_equal(lab[2], lab[3])
    written = orc.read_index(idx, kind == "grouping")
    for key in ("offsets", "ids", "codes", "norm_codes"):
        assert np.array_equal(written[key], np.asarray(cur[key]).reshape(written[key].shape)), key
