"""IndexIVF_HNSW::remove_ids on the host lists: an index read from a .index file, with no device handle
ever made, loses the codes of the labels from its lists -- and, for Grouping, from its sub-groups -- and write() writes
the remaining index.  The written file equals the lists and sub-group sizes numpy filters (tests/remove_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import remove_ref
import synth
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("remove_tool") / "remove_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "remove_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
                    "-livfhnsw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


CASES = {"ivf": dict(seed=31, nc=64, d=64, M=8, n_base=4000, nq=8, efConstruction=40),
         "grouping": dict(seed=32, nc=64, d=64, M=8, n_base=4000, nq=8, efConstruction=40, nsubc=8)}


@pytest.mark.parametrize("kind", ["ivf", "grouping"])
@pytest.mark.parametrize("labels", ["random", "whole_list", "none", "repeated_and_absent"])
def test_remove_ids_writes_the_filtered_index(tool, tmp_path, kind, labels):
    c = synth.make_corpus(**CASES[kind])
    rng = np.random.default_rng(len(labels))
    off = c["offsets"].astype(np.int64)
    big = int(np.argmax(np.diff(off)))
    lab = {"random": rng.choice(c["ids"], 900, replace=False),
           "whole_list": c["ids"][off[big]:off[big + 1]],
           "none": np.zeros(0, np.uint32),
           "repeated_and_absent": np.concatenate([c["ids"][:50], c["ids"][:50], [4000, 77777, 0xffffffff]])}[labels]
    lab = np.ascontiguousarray(lab, np.uint32)
    src, dst, lpath = (str(tmp_path / n) for n in ("in.index", "out.index", "labels.u32"))
    synth.oracle_index(c).write(src)
    lab.tofile(lpath)
    r = subprocess.run([tool, "host", kind, str(c["d"]), str(c["nc"]), str(c["code_size"]), str(c["nsubc"]), src, lpath,
                        dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    want = remove_ref.filter_lists(c["offsets"], c["ids"], c["codes"], c["norm_codes"], lab,
                                   c["subgroup_sizes"] if kind == "grouping" else None)
    assert int(r.stdout.split()[-1]) == int(want["removed"].sum())
    got = orc.read_index(dst, kind == "grouping")
    for key in ("offsets", "ids", "codes", "norm_codes"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["centroid_norms"], c["centroid_norms"])
    if kind == "grouping":
        assert np.array_equal(got["subgroup_sizes"], want["subgroup_sizes"])
        for key in ("alphas", "nn_centroid_idxs", "inter_centroid_dists"):
            assert np.array_equal(got[key], np.asarray(c[key]).reshape(got[key].shape)), key
    if labels == "whole_list":
        assert got["offsets"][big + 1] == got["offsets"][big]
