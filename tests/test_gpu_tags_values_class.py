"""Tag AND value through the class surface (IndexIVF_HNSW::search_batch_tags_values, range_search_tags_values; DESIGN.md
3.26), of both classes, on the tags and values the object keeps beside itself: both are set before the device copy exists,
then search and range search run, again after add_batch (IVFADC: appended to the device copy in place), after
invalidate_device() (the copy is remade), after update_batch (IVFADC: one upsert on the device copy), after remove_ids and
after some ids are re-tagged and re-valued on the current copy.  Every round equals the C ABI on a handle taken through the
same steps with the same tags and values: the k labels of every query, and the range search's lims and labels in scan order
(radius +inf: every scored code that passes).  As in test_gpu_values_class, distances are not compared: the class reports
them on its own scale.  The driver itself checks the two delegations (a null array), what must throw (a call while
set_id_filter is installed) and the calls after clear_id_tags + clear_id_values."""
import os
import subprocess

import numpy as np
import pytest

import filter_ref
import hostio
import synth
import tags_values_ref as tv
from oracle import orc
from test_gpu_filter_slots_class import CASES
from test_gpu_remove import _upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 6


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tags_values_tool") / "tags_values_tool")
    lib = os.path.join(ROOT, "ivf-hnsw_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "tags_values_tool.cpp"), "-o", exe, "-L" + lib, "-livfhnsw",
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
    asg0 = tv.assignment(b)
    m = asg0[1] != tv.TAG_NONE
    tlabels, tags = asg0[0][m], asg0[1][m]
    m = asg0[2] != tv.VALUE_NONE
    vlabels, values = asg0[0][m], asg0[2][m]
    # rows to come: every other one tagged 0 and inside the band across the sign bit, every third of the rest tagged 0xfffe
    # with the value 0x80000001 too; the others carry neither
    tlabels = np.concatenate([tlabels, new_ids[::2], new_ids[1::6]]).astype(np.uint32)
    tags = np.concatenate([tags, np.zeros(len(new_ids[::2]), np.uint16), np.full(len(new_ids[1::6]), 0xfffe, np.uint16)])
    vlabels = np.concatenate([vlabels, new_ids[::2], new_ids[1::6]]).astype(np.uint32)
    values = np.concatenate([values, np.full(len(new_ids[::2]) + len(new_ids[1::6]), 0x80000001, np.uint32)])
    order = np.random.default_rng(5).permutation(len(tlabels))  # the two incremental calls each take a mixture
    tlabels, tags = tlabels[order], tags[order]
    order = np.random.default_rng(6).permutation(len(vlabels))
    vlabels, values = vlabels[order], values[order]
    # re-tagging and re-valuing: of the ids that pass (0, band), 300 move to tag 255 with the value 0 and 300 lose both
    band = (0, tv.BAND31)
    inband = tv.labels_in(asg0, band)
    inband = inband[~np.isin(inband, gone) & ~np.isin(inband, upd_labels)][:600]
    assert len(inband) == 600
    relabels = inband
    retags = np.concatenate([np.full(300, 255, np.uint16), np.full(300, tv.TAG_NONE, np.uint16)])
    revalues = np.concatenate([np.zeros(300, np.uint32), np.full(300, tv.VALUE_NONE, np.uint32)])
    qt, qr = tv.query_tags(nq), tv.query_ranges(nq)
    files = {}
    for name, arr in (("query_tags.u16", qt), ("query_ranges.u32", qr), ("tlabels.u32", tlabels), ("tags.u16", tags),
                      ("vlabels.u32", vlabels), ("values.u32", values), ("upd_labels.u32", upd_labels), ("gone.u32", gone),
                      ("relabels.u32", relabels), ("retags.u16", retags), ("revalues.u32", revalues)):
        files[name] = str(tmp_path / name)
        np.ascontiguousarray(arr).tofile(files[name])
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    env.pop("IVFHNSW_SHARDS", None)
    out, idx = str(tmp_path / "out.bin"), str(tmp_path / "out.index")
    args = [kind, b["d"], b["nc"], b["code_size"], b["nsubc"], p["centroids"], p["info"], p["edges"], p["pq"], p["norm_pq"],
            p["opq"], p["index"], p["queries"], nq, k, nprobe, max_codes, ef, int(pruning), files["query_tags.u16"],
            files["query_ranges.u32"], files["tlabels.u32"], files["tags.u16"], files["vlabels.u32"], files["values.u32"], apath,
            add_first, upath, files["upd_labels.u32"], files["gone.u32"], files["relabels.u32"], files["retags.u16"],
            files["revalues.u32"], out, idx, "end"]
    r = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = _rounds(out, nq, k)
    # the C ABI through the same steps
    q = b["queries"]
    h = _upload(gpu(), b)
    h.set_tags(tlabels, tags)
    h.set_values(vlabels, values)
    tag_of = dict(zip(tlabels.tolist(), tags.tolist()))
    val_of = dict(zip(vlabels.tolist(), values.tolist()))

    def step(rnd):
        if rnd == 1 and kind == "ivf":
            h.append_ivf(add[0], new_ids, add[1], add[2])
        if rnd == 3 and kind == "ivf":
            assert h.upsert_ivf(upd[0], upd_labels, upd[1], upd[2])[0] == 400
        if rnd == 4:
            assert h.remove_ids(gone)[0] == len(gone)
        if rnd == 5:
            h.set_tags(relabels, retags)
            h.set_values(relabels, revalues)
            tag_of.update(zip(relabels.tolist(), retags.tolist()))
            val_of.update(zip(relabels.tolist(), revalues.tolist()))

    for rnd in range(ROUNDS):
        step(rnd)
        d, l = h.search_tags_values(q, k, qt, qr, nprobe, max_codes, efSearch=ef, do_pruning=pruning, heap_order=True)
        assert h.last_scan_kernel().endswith("+tags+values")
        assert np.array_equal(np.sort(got[rnd]["labels"], axis=1), np.sort(l, axis=1)), rnd
        assert (got[rnd]["dist"][got[rnd]["labels"] < 0] == tv.FLT_MAX).all(), rnd
        lims, _, rl = h.range_search_tags_values(q, np.inf, qt, qr, nprobe, max_codes, efSearch=ef, do_pruning=pruning)
        assert np.array_equal(got[rnd]["lims"], lims), rnd
        assert np.array_equal(got[rnd]["range_labels"], rl), rnd
        lab_ = np.array(sorted(set(tag_of) | set(val_of)), np.uint32)
        now = (lab_, np.array([tag_of.get(int(x), tv.TAG_NONE) for x in lab_], np.uint16),
               np.array([val_of.get(int(x), tv.VALUE_NONE) for x in lab_], np.uint32))
        for p in (band, (tv.TAG_NONE, tv.UPPER31), (255, (0, 0)), (256, tv.VALUED)):
            lab = got[rnd]["labels"][tv.mine(qt, qr, p)]
            assert np.isin(lab[lab >= 0], tv.labels_in(now, p)).all() and (lab >= 0).any(), (rnd, p)
        for p in tv.PADDING:
            assert (got[rnd]["labels"][tv.mine(qt, qr, p)] == -1).all(), (rnd, p)
        assert (got[rnd]["labels"][tv.mine(qt, qr, tv.UNFILTERED)] >= 0).all()
    assert np.array_equal(got[1]["labels"], got[2]["labels"])  # the remade copy answers as the appended one
    assert not np.array_equal(got[4]["labels"], got[5]["labels"])  # the re-tagged, re-valued ids left their pair
    assert not np.isin(got[5]["labels"][tv.mine(qt, qr, band)], relabels).any()
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
