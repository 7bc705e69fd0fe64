"""Row tags through the class surface (IndexIVF_HNSW::set_id_tags, clear_id_tags, search_batch_tags, range_search_tags;
DESIGN.md 3.21), of both classes: the tags are set before the device copy exists, then search and range search run, again
after add_batch (IVFADC: appended to the device copy in place), after invalidate_device() (the copy is remade) and after
some ids are re-tagged on the current copy.  Every round equals the C ABI on an upload of the same index with the same
tags: the k labels of every query, and the range search's lims and labels in scan order (radius +inf: every scored code
that passes).  As in test_gpu_filter_slots_class, distances are not compared: the class reports them on its own scale.
The driver itself checks what must throw (where the _slots calls throw, and a label given two tags) and clear_id_tags."""
import os
import subprocess

import numpy as np
import pytest

import filter_ref
import hostio
import synth
import tags_ref as tr
from oracle import orc
from test_gpu_append import _csr_append
from test_gpu_filter_slots_class import CASES, _rounds
from test_gpu_remove import _upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tags_tool") / "tags_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "tags_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
                    "-livfhnsw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("kind", ["ivf", "grouping"])
def test_class_rounds_equal_the_c_abi(gpu, tool, tmp_path, kind):
    b = filter_ref.clipped(synth.make_corpus(**CASES[kind]))
    p = hostio.dump_corpus(b, str(tmp_path))
    nq, k, nprobe, max_codes, ef, pruning = len(b["queries"]), 10, 16, 2000, 40, kind == "grouping"
    add_first = 10 ** 6
    cur, apath = b, "-"
    new_ids = np.zeros(0, np.uint32)
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
    labels, tags = tr.tagged(tr.assignment(b))
    # rows to come: every other one tagged 0, every third of the rest 0xfffe
    labels = np.concatenate([labels, new_ids[::2], new_ids[1::6]]).astype(np.uint32)
    tags = np.concatenate([tags, np.zeros(len(new_ids[::2]), np.uint16), np.full(len(new_ids[1::6]), 0xfffe, np.uint16)])
    order = np.random.default_rng(5).permutation(len(labels))  # the two incremental calls each take a mixture
    labels, tags = labels[order], tags[order]
    # re-tagging: 300 ids of tag 0 move to 255, 300 more are untagged
    zero = labels[tags == 0][:600]
    relabels, retags = zero, np.concatenate([np.full(300, 255, np.uint16), np.full(300, tr.NONE, np.uint16)])
    after = dict(zip(labels.tolist(), tags.tolist()))
    after.update(zip(relabels.tolist(), retags.tolist()))
    labels2 = np.array(sorted(after), np.uint32)
    tags2 = np.array([after[int(l)] for l in labels2], np.uint16)
    qt = tr.query_tags(nq)
    files = {}
    for name, arr in (("query_tags.u16", qt), ("labels.u32", labels), ("tags.u16", tags), ("relabels.u32", relabels),
                      ("retags.u16", retags)):
        files[name] = str(tmp_path / name)
        arr.tofile(files[name])
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    env.pop("IVFHNSW_SHARDS", None)
    out, idx = str(tmp_path / "out.bin"), str(tmp_path / "out.index")
    args = [kind, b["d"], b["nc"], b["code_size"], b["nsubc"], p["centroids"], p["info"], p["edges"], p["pq"], p["norm_pq"],
            p["opq"], p["index"], p["queries"], nq, k, nprobe, max_codes, ef, int(pruning), files["query_tags.u16"],
            files["labels.u32"], files["tags.u16"], apath, add_first, files["relabels.u32"], files["retags.u16"], out, idx, "end"]
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = _rounds(out, nq, k)
    want = [(b, labels, tags), (cur, labels, tags), (cur, labels, tags), (cur, labels2, tags2)]
    q = b["queries"]
    for rnd, (corpus_, lab_, tag_) in enumerate(want):
        h = _upload(gpu(), corpus_)
        h.set_tags(lab_[tag_ != tr.NONE], tag_[tag_ != tr.NONE])
        d, l = h.search_tags(q, k, qt, nprobe, max_codes, efSearch=ef, do_pruning=pruning, heap_order=True)
        assert h.last_scan_kernel().endswith("+tags")
        assert np.array_equal(np.sort(got[rnd]["labels"], axis=1), np.sort(l, axis=1)), rnd
        assert (got[rnd]["dist"][got[rnd]["labels"] < 0] == tr.FLT_MAX).all(), rnd
        lims, _, rl = h.range_search_tags(q, np.inf, qt, nprobe, max_codes, efSearch=ef, do_pruning=pruning)
        assert np.array_equal(got[rnd]["lims"], lims), rnd
        assert np.array_equal(got[rnd]["range_labels"], rl), rnd
        for t in (0, 255, 256, 0xfffe):
            lab = got[rnd]["labels"][qt == t]
            assert np.isin(lab[lab >= 0], lab_[tag_ == t]).all() and (lab >= 0).any(), (rnd, t)
        assert (got[rnd]["labels"][qt == tr.ABSENT] == -1).all()
        assert (got[rnd]["labels"][qt == tr.NONE] >= 0).all()
        h.close()
    assert np.array_equal(got[1]["labels"], got[2]["labels"])  # the remade copy answers as the appended one
    assert not np.array_equal(got[2]["labels"], got[3]["labels"])  # the re-tagged ids left tag 0
    assert not np.isin(got[3]["labels"][qt == 0], relabels).any()
    if kind == "ivf":
        assert not np.array_equal(got[0]["lims"], got[1]["lims"])  # the added rows are scanned
        new = got[1]["labels"][got[1]["labels"] >= add_first]
        assert len(new) > 0
    written = orc.read_index(idx, kind == "grouping")
    for key in ("offsets", "ids", "codes", "norm_codes"):
        assert np.array_equal(written[key], np.asarray(cur[key]).reshape(written[key].shape)), key
