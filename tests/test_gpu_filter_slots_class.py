"""Filter slots through the class surface (IndexIVF_HNSW::set_id_filter_slot, clear_id_filter_slot, search_batch_slots,
range_search_slots): the slots are set before the device copy exists, then search and range search run,
again after add_batch (IVFADC: appended to the device copy in place), after invalidate_device() (the copy is remade) and
after one slot is cleared.  Every round equals the C ABI on an upload of the same index with the same slots: the k labels
of every query, and the range search's lims and labels in scan order (radius +inf: every scored code that passes).  As in
test_gpu_filter_class, distances are not compared: the class reports them on its own scale."""
import os
import subprocess

import numpy as np
import pytest

import filter_ref
import filter_slots_ref as fs
import hostio
import synth
from oracle import orc
from test_gpu_append import _csr_append
from test_gpu_remove import _upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"ivf": dict(seed=91, nc=128, d=128, M=16, n_base=9000, nq=48, efConstruction=80),
         "grouping": dict(seed=92, nc=128, d=128, M=16, n_base=9000, nq=48, efConstruction=80, nsubc=16)}
ROUNDS = 4


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_slots_tool") / "filter_slots_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filter_slots_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
                    "-livfhnsw_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _rounds(path, nq, k):
    raw = np.fromfile(path, np.uint8)
    out, at = [], 0
    for _ in range(ROUNDS):
        r = {}
        r["labels"] = raw[at:at + 8 * nq * k].view(np.int64).reshape(nq, k)
        at += 8 * nq * k
        r["dist"] = raw[at:at + 4 * nq * k].view(np.float32).reshape(nq, k)
        at += 4 * nq * k
        r["lims"] = raw[at:at + 8 * (nq + 1)].view(np.uint64)
        at += 8 * (nq + 1)
        total = int(r["lims"][-1])
        r["range_labels"] = raw[at:at + 8 * total].view(np.int64)
        at += 8 * total + 4 * total
        out.append(r)
    assert at == len(raw)
    return out


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
    sets = fs.slot_sets(b)
    # rows to come: every other one allowed by slot 0 and by slot 31, every third denied by slot 7
    sets[0] = (np.concatenate([sets[0][0], new_ids[::2]]).astype(np.uint32), False)
    sets[31] = (np.concatenate([sets[31][0], new_ids[::2]]).astype(np.uint32), False)
    sets[7] = (np.concatenate([sets[7][0], new_ids[::3]]).astype(np.uint32), True)
    qs = fs.query_slots(nq)
    qp = str(tmp_path / "query_slots.u8")
    qs.tofile(qp)
    set_args = []
    for s, (labels, deny) in sets.items():
        lp = str(tmp_path / ("labels%d.u32" % s))
        labels.tofile(lp)
        set_args += [s, int(deny), lp]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    env.pop("IVFHNSW_SHARDS", None)
    out, idx = str(tmp_path / "out.bin"), str(tmp_path / "out.index")
    clear_slot = 31
    args = [kind, b["d"], b["nc"], b["code_size"], b["nsubc"], p["centroids"], p["info"], p["edges"], p["pq"], p["norm_pq"],
            p["opq"], p["index"], p["queries"], nq, k, nprobe, max_codes, ef, int(pruning), qp, len(sets)] + set_args + \
           [apath, add_first, clear_slot, out, idx]
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = _rounds(out, nq, k)
    less = {s: v for s, v in sets.items() if s != clear_slot}
    want = [(b, sets), (cur, sets), (cur, sets), (cur, less)]
    q = b["queries"]
    for rnd, (corpus_, sets_) in enumerate(want):
        h = fs.install(_upload(gpu(), corpus_), sets_)
        d, l = h.search_slots(q, k, qs, nprobe, max_codes, efSearch=ef, do_pruning=pruning, heap_order=True)
        assert h.last_scan_kernel().endswith("+slots")
        assert np.array_equal(np.sort(got[rnd]["labels"], axis=1), np.sort(l, axis=1)), rnd
        assert (got[rnd]["dist"][got[rnd]["labels"] < 0] == fs.FLT_MAX).all(), rnd
        lims, _, rl = h.range_search_slots(q, np.inf, qs, nprobe, max_codes, efSearch=ef, do_pruning=pruning)
        assert np.array_equal(got[rnd]["lims"], lims), rnd
        assert np.array_equal(got[rnd]["range_labels"], rl), rnd
        for s, (labels, deny) in sets_.items():
            lab = got[rnd]["labels"][qs == s]
            assert (np.isin(lab[lab >= 0], labels) != deny).all() and (lab >= 0).any(), (rnd, s)
        assert (got[rnd]["labels"][qs == fs.UNSET] == -1).all()
    assert (got[3]["labels"][qs == clear_slot] == -1).all() and (got[2]["labels"][qs == clear_slot] >= 0).any()
    assert np.array_equal(got[1]["labels"], got[2]["labels"])  # the remade copy answers as the appended one
    if kind == "ivf":
        assert not np.array_equal(got[0]["lims"], got[1]["lims"])  # the added rows are scanned
        new = got[1]["labels"][got[1]["labels"] >= add_first]
        assert len(new) > 0 and np.isin(new, np.concatenate([sets[0][0], sets[31][0], new_ids])).all()
    written = orc.read_index(idx, kind == "grouping")
    for key in ("offsets", "ids", "codes", "norm_codes"):
        assert np.array_equal(written[key], np.asarray(cur[key]).reshape(written[key].shape)), key
