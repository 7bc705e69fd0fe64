"""Row values through the class surface (IndexIVF_HNSW::set_id_values, clear_id_values, search_batch_values,
range_search_values), of both classes: the values are set before the device copy exists, then search and
range search run, again after add_batch (IVFADC: appended to the device copy in place), after invalidate_device() (the copy
is remade), after update_batch (IVFADC: one upsert on the device copy), after remove_ids and after some ids are re-valued
on the current copy.  Every round equals the C ABI on a handle taken through the same steps with the same values: the k
labels of every query, and the range search's lims and labels in scan order (radius +inf: every scored code that passes).
As in test_gpu_tags_class, distances are not compared: the class reports them on its own scale.  The driver itself checks
what must throw (a label given two values, a _values call while set_id_filter is installed) and clear_id_values."""
import os
import subprocess

import numpy as np
import pytest

import filter_ref
import hostio
import synth
import values_ref as vr
from oracle import orc
from test_gpu_filter_slots_class import CASES
from test_gpu_remove import _upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 6


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("values_tool") / "values_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "values_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
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
    rng = np.random.default_rng(12)
    nq, k, nprobe, max_codes, ef, pruning = len(b["queries"]), 10, 16, 2000, 40, kind == "grouping"
    add_first = 10 ** 6
    apath = upath = "-"
    new_ids = np.zeros(0, np.uint32)
    upd_labels = np.zeros(0, np.uint32)
    ox = synth.oracle_index(b)
    ox.set_params(nprobe, max_codes, ef)
    if kind == "ivf":
        xadd = b["base"][:1500] + np.float32(0.5)
        apath = str(tmp_path / "add.fvecs")
        hostio.write_xvecs(apath, xadd)
        add = ox.add_batch_encode(xadd)[:3]
        new_ids = np.arange(add_first, add_first + len(xadd), dtype=np.uint32)
        # update_batch: 400 resident labels (values kept by label) and 400 new ones (beyond the table: none)
        upd_labels = rng.permutation(np.concatenate([rng.choice(np.unique(b["ids"]), 400, replace=False),
                                                     np.arange(2 * 10 ** 6, 2 * 10 ** 6 + 400)]).astype(np.uint32))
        xupd = (b["base"][rng.integers(0, len(b["base"]), len(upd_labels))] +
                rng.normal(0, 3.0, (len(upd_labels), b["d"]))).astype(np.float32)
        upath = str(tmp_path / "upd.fvecs")
        hostio.write_xvecs(upath, xupd)
        upd = ox.add_batch_encode(xupd)[:3]
    gone = rng.choice(np.unique(b["ids"]), 2000, replace=False).astype(np.uint32)
    gone = gone[~np.isin(gone, upd_labels)]
    labels, values = vr.valued(vr.assignment(b))
    # rows to come: every other one inside the band across the sign bit, every third of the rest at 0xfffffffe
    labels = np.concatenate([labels, new_ids[::2], new_ids[1::6]]).astype(np.uint32)
    values = np.concatenate([values, np.full(len(new_ids[::2]), 0x80000001, np.uint32),
                             np.full(len(new_ids[1::6]), 0xfffffffe, np.uint32)])
    order = np.random.default_rng(5).permutation(len(labels))  # the two incremental calls each take a mixture
    labels, values = labels[order], values[order]
    # re-valuing: 300 ids of the band move to the 2^16 band, 300 more lose their value
    band, band16 = vr.PATTERN[3], vr.PATTERN[6]
    inband = labels[(values >= band[0]) & (values <= band[1]) & ~np.isin(labels, gone)][:600]
    relabels, revalues = inband, np.concatenate([np.full(300, 0x10000, np.uint32), np.full(300, vr.NONE, np.uint32)])
    qr = vr.query_ranges(nq)
    files = {}
    for name, arr in (("query_ranges.u32", qr), ("labels.u32", labels), ("values.u32", values), ("upd_labels.u32", upd_labels),
                      ("gone.u32", gone), ("relabels.u32", relabels), ("revalues.u32", revalues)):
        files[name] = str(tmp_path / name)
        np.ascontiguousarray(arr).tofile(files[name])
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    env.pop("IVFHNSW_SHARDS", None)
    out, idx = str(tmp_path / "out.bin"), str(tmp_path / "out.index")
    args = [kind, b["d"], b["nc"], b["code_size"], b["nsubc"], p["centroids"], p["info"], p["edges"], p["pq"], p["norm_pq"],
            p["opq"], p["index"], p["queries"], nq, k, nprobe, max_codes, ef, int(pruning), files["query_ranges.u32"],
            files["labels.u32"], files["values.u32"], apath, add_first, upath, files["upd_labels.u32"], files["gone.u32"],
            files["relabels.u32"], files["revalues.u32"], out, idx, "end"]
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = _rounds(out, nq, k)
    # the C ABI through the same steps
    q = b["queries"]
    h = _upload(gpu(), b)
    h.set_values(labels, values)
    asg = dict(zip(labels.tolist(), values.tolist()))

    def step(rnd):
        if rnd == 1 and kind == "ivf":
            h.append_ivf(add[0], new_ids, add[1], add[2])
        if rnd == 3 and kind == "ivf":
            assert h.upsert_ivf(upd[0], upd_labels, upd[1], upd[2])[0] == 400
        if rnd == 4:
            assert h.remove_ids(gone)[0] == len(gone)
        if rnd == 5:
            h.set_values(relabels, revalues)
            asg.update(zip(relabels.tolist(), revalues.tolist()))

    for rnd in range(ROUNDS):
        step(rnd)
        d, l = h.search_values(q, k, qr, nprobe, max_codes, efSearch=ef, do_pruning=pruning, heap_order=True)
        assert h.last_scan_kernel().endswith("+values")
        assert np.array_equal(np.sort(got[rnd]["labels"], axis=1), np.sort(l, axis=1)), rnd
        assert (got[rnd]["dist"][got[rnd]["labels"] < 0] == vr.FLT_MAX).all(), rnd
        lims, _, rl = h.range_search_values(q, np.inf, qr, nprobe, max_codes, efSearch=ef, do_pruning=pruning)
        assert np.array_equal(got[rnd]["lims"], lims), rnd
        assert np.array_equal(got[rnd]["range_labels"], rl), rnd
        lab_ = np.array(sorted(asg), np.uint32)
        val_ = np.array([asg[int(x)] for x in lab_], np.uint32)
        for rg in (band, band16, (0, 0), vr.VALUED):
            lab = got[rnd]["labels"][vr.mine(qr, rg)]
            assert np.isin(lab[lab >= 0], vr.labels_in((lab_, val_), rg)).all() and (lab >= 0).any(), (rnd, rg)
        assert (got[rnd]["labels"][vr.mine(qr, vr.INVERTED)] == -1).all()
        assert (got[rnd]["labels"][vr.mine(qr, vr.FULL)] >= 0).all()
    assert np.array_equal(got[1]["labels"], got[2]["labels"])  # the remade copy answers as the appended one
    assert not np.array_equal(got[4]["labels"], got[5]["labels"])  # the re-valued ids left the band
    assert not np.isin(got[5]["labels"][vr.mine(qr, band)], relabels).any()
    assert not np.isin(got[4]["range_labels"], gone).any() and np.isin(got[3]["range_labels"], gone).any()
    if kind == "ivf":
        assert not np.array_equal(got[0]["lims"], got[1]["lims"])  # the added rows are scanned
        assert (got[1]["labels"] >= add_first).any()
        assert not np.array_equal(got[2]["lims"], got[3]["lims"])  # the update moved rows
    off, ids, codes, ncodes = h.download_ivf()
    h.close()
    written = orc.read_index(idx, kind == "grouping")
    for key, arr in (("offsets", off), ("ids", ids), ("codes", codes), ("norm_codes", ncodes)):
        assert np.array_equal(written[key], np.asarray(arr).reshape(written[key].shape)), key
