"""CPU side of the reconstruction feature: the interface exists at every layer below the device, and
tests/recon_ref.py -- the expectation of tests/test_gpu_recon.py -- restates the corpus generator's own arithmetic."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import corpus
import recon_ref
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ivfhnsw_gpu_locate", "ivfhnsw_gpu_locate_dev", "ivfhnsw_gpu_reconstruct_rows",
               "ivfhnsw_gpu_reconstruct_rows_dev", "ivfhnsw_gpu_reconstruct", "ivfhnsw_gpu_reconstruct_dev",
               "ivfhnsw_gpu_search_reconstruct", "ivfhnsw_gpu_search_reconstruct_dev")
GROUPING = dict(seed=43, nc=256, d=96, M=16, n_base=20000, nq=64, nsubc=8)


def test_surface(pkg):
    hdr = open(os.path.join(ROOT, "include", "ivfhnsw_hip.h")).read()
    declared = set(re.findall(r"\bint (ivfhnsw_gpu_[a-z_0-9]+)\s*\(", hdr))
    lib = pkg.lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared, sym
        assert sym in pkg.ABI_SYMBOLS, sym
        assert hasattr(lib, sym), sym
    assert re.search(r"#define IVFHNSW_RECON_ORIGINAL 0\b", hdr) and re.search(r"#define IVFHNSW_RECON_ROTATED 1\b", hdr)
    assert (pkg.RECON_ORIGINAL, pkg.RECON_ROTATED) == (0, 1)
    assert lib.ivfhnsw_gpu_abi_version() == 9
    for name in ("locate", "locate_dev", "reconstruct_rows", "reconstruct_rows_dev", "reconstruct", "reconstruct_dev",
                 "search_reconstruct", "search_reconstruct_dev", "reconstruct_list"):
        fn = getattr(pkg.GpuIndex, name)
        assert callable(fn) and "self" in inspect.signature(fn).parameters, name
    # the header says what ORIGINAL space is under OPQ, and that it is not the reference's arithmetic
    assert "IndexIVF_HNSW.cpp:106-113" in hdr and "0x7fc00000" in hdr


def _synth_anchor(c):
    """The anchors as synth.make_corpus computes them (its own expressions), in resident-row order."""
    cents = c["centroids"]
    off = c["offsets"].astype(np.int64)
    lst = np.repeat(np.arange(c["nc"]), np.diff(off))
    if not c["nsubc"]:
        return cents[lst]
    out = np.empty((len(lst), c["d"]), np.float32)
    for i in range(c["nc"]):
        sc = cents[i][None, :] + c["alphas"][i] * (cents[c["nn_centroid_idxs"][i]] - cents[i][None, :])
        sub = np.repeat(np.arange(c["nsubc"]), c["subgroup_sizes"][i])
        out[off[i]:off[i + 1]] = sc[sub]
    return out


@pytest.mark.parametrize("kw", [dict(nc=256, d=128, M=16, n_base=20000), GROUPING], ids=["ivfadc", "grouping"])
def test_helper_restates_the_generator(kw):
    c = corpus(**kw)
    n = len(c["ids"])
    rows = np.arange(n)
    # rows -> lists -> sub-groups
    off = c["offsets"].astype(np.int64)
    lst = recon_ref.row_lists(c["offsets"], rows)
    assert (off[lst] <= rows).all() and (rows < off[lst + 1]).all()
    if c["nsubc"]:
        l2, sub = recon_ref.row_subgroups(c["offsets"], c["subgroup_sizes"], rows)
        assert np.array_equal(l2, lst)
        got = np.zeros_like(c["subgroup_sizes"])
        np.add.at(got, (l2, sub), 1)
        assert np.array_equal(got, c["subgroup_sizes"]) and (np.diff(sub)[np.diff(lst) == 0] >= 0).all()
    # without OPQ the helper is the generator's anchor + decode, bit for bit
    anchor = _synth_anchor(c)
    want = (anchor + synth._pq_decode(c["codes"], c["pq_centroids"])).astype(np.float32)
    got = recon_ref.recon_rotated(c)
    assert np.array_equal(recon_ref.bits(got), recon_ref.bits(want))
    # and it is a reconstruction: closer to the base vectors than the anchors alone
    base = c["base"][c["ids"]]
    err = ((got.astype(np.float64) - base) ** 2).sum(1).mean()
    err0 = ((anchor.astype(np.float64) - base) ** 2).sum(1).mean()
    assert err < err0, (err, err0)
    # empty slots
    some = recon_ref.recon_rotated(c, [3, -1, 0])
    assert (recon_ref.bits(some[1]) == 0x7FC00000).all() and np.array_equal(some[[0, 2]], got[[3, 0]])
