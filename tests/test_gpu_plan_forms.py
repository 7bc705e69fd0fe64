"""Every form of the Grouping scan plan against the CPU oracle, the way test_gpu_grouping.py compares the default one:
identical labels, bit-identical distances, identical numbers of scored codes and sub-groups.  The forms -- four wavefronts
per query (default), one (IVFHNSW_PLAN_GROUP4=0), neighbour centroids through the LDS hash set or not
(IVFHNSW_PLAN_DEDUPE=1 / 0) -- are chosen by knobs read once per process, so every (setting, case) runs in a child
process under a timeout; the corpora and the oracle's answers are computed once here and handed over as .npz files.

The cases take the paths the plan kernels have: more sub-groups than lanes (the chunked sub-group loop, the generic
phase C), nsubc = 64 (the readlane threshold chain, the pipelined phase C), more probes than lanes in phase 0, and a
max_codes that bites in both passes.  One more case, under IVFHNSW_PLAN_DEDUPE=1 only, gives every query more distinct
neighbour centroids than the hash set has slots, so pairs that find no slot are gathered directly.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import corpus
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SETTINGS = [{}, {"IVFHNSW_PLAN_GROUP4": "0"}, {"IVFHNSW_PLAN_DEDUPE": "1"}, {"IVFHNSW_PLAN_DEDUPE": "0"}]

CASES = {
    # corpus (test_gpu_grouping.py's, 64 queries), nprobe, max_codes, efSearch
    "nsubc80": (dict(seed=44, nc=256, d=128, M=8, n_base=20000, nq=64, nsubc=80, efConstruction=120), 4, 10 ** 9, 100),
    "nsubc64": (dict(seed=42, nc=128, d=128, M=16, n_base=20000, nq=64, nsubc=64), 8, 600, 80),
    "nprobe200": (dict(seed=48, nc=256, d=128, M=8, n_base=20000, nq=64, nsubc=8), 200, 10 ** 9, 220),
    "max_codes": (dict(seed=41, nc=256, d=128, M=16, n_base=30000, nq=64, nsubc=16), 16, 800, 40),
}
# more distinct neighbour centroids per query than the hash set's 2048 slots; the coarse stage comes from the oracle
OVERFLOW = (dict(seed=51, nc=8192, d=32, M=8, n_base=500000, nq=16, nsubc=16, hnsw_M=8, efConstruction=60, empty_frac=0.0),
            512, 10 ** 9, 600)
GH_SLOTS = 2048

CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_pkg()
z = np.load(%(npz)r)
g = pkg.GpuIndex(0)
g.upload_ivf(int(z["d"]), int(z["code_size"]), z["offsets"], z["ids"], z["codes"], z["norm_codes"], z["centroid_norms"],
             z["pq_centroids"], z["norm_table"], opq_A=None)
g.upload_grouping(int(z["nsubc"]), z["alphas"], z["nn_centroid_idxs"], z["subgroup_sizes"], z["inter_centroid_dists"])
g.upload_quantizer(z["g_counts"], z["g_links"], z["g_vectors"], int(z["g_enterpoint"]))
nprobe, max_codes, ef = int(z["nprobe"]), int(z["max_codes"]), int(z["ef"])
for p in z["prunings"]:
    p = int(p)
    ref_d, ref_l, cid, cd = z["ref_d_%%d" %% p], z["ref_l_%%d" %% p], z["cid_%%d" %% p], z["cd_%%d" %% p]
    counts = tuple(int(v) for v in z["counts_%%d" %% p])
    # host-supplied coarse stage
    dist, lab = g.search(z["queries"], 1, nprobe, max_codes, coarse_ids=cid, coarse_dists=cd, do_pruning=bool(p))
    assert np.array_equal(lab, ref_l), "pruning %%d: labels differ at %%s" %% (p, np.nonzero((lab != ref_l).any(1))[0][:10])
    assert np.array_equal(dist.view(np.uint32), ref_d.view(np.uint32)), "pruning %%d: distances differ" %% p
    assert g.last_scan_counts() == counts, "pruning %%d: %%s, oracle %%s" %% (p, g.last_scan_counts(), counts)
    if int(z["walk"]):  # whole path on the device
        dist, lab = g.search(z["queries"], 1, nprobe, max_codes, efSearch=ef, do_pruning=bool(p))
        assert np.array_equal(lab, ref_l), "pruning %%d, device coarse: labels differ" %% p
        assert np.array_equal(dist.view(np.uint32), ref_d.view(np.uint32)), "pruning %%d, device coarse: distances differ" %% p
        assert g.last_scan_counts() == counts, "pruning %%d, device coarse: %%s, oracle %%s" %% (p, g.last_scan_counts(), counts)
g.close()
print("PLAN FORMS OK")
'''


def _reference_file(path, c, nprobe, max_codes, ef, prunings, walk):
    """The corpus and the oracle's answers of one case as an .npz; returns (path, the oracle's coarse ids)."""
    gr = c["graph"]
    out = dict(d=c["d"], code_size=c["code_size"], nsubc=c["nsubc"], nprobe=nprobe, max_codes=max_codes, ef=ef, walk=int(walk),
               prunings=np.array(prunings), queries=c["queries"], g_counts=gr.counts, g_links=gr.links, g_vectors=gr.vectors,
               g_enterpoint=gr.enterpoint)
    for key in ("offsets", "ids", "codes", "norm_codes", "centroid_norms", "pq_centroids", "norm_table", "alphas",
                "nn_centroid_idxs", "subgroup_sizes", "inter_centroid_dists"):
        out[key] = c[key]
    ox = synth.oracle_index(c)
    cid = None
    for p in prunings:
        ox.set_params(nprobe, max_codes, ef, do_pruning=bool(p))
        ref_d, ref_l, cid, cd, st = ox.search_batch(c["queries"], k=1)
        out.update({"ref_d_%d" % p: ref_d, "ref_l_%d" % p: ref_l, "cid_%d" % p: cid, "cd_%d" % p: cd,
                    "counts_%d" % p: np.array([st.ncode, st.nseg], np.uint64)})
    np.savez(path, **out)
    return path, cid


@pytest.fixture(scope="module")
def references(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_forms")
    return {name: _reference_file(str(d / (name + ".npz")), corpus(**kw), nprobe, max_codes, ef, (0, 1), True)[0]
            for name, (kw, nprobe, max_codes, ef) in CASES.items()}


def _run_child(env, npz):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, npz=npz)], capture_output=True, text=True, env=e,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "PLAN FORMS OK" in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("env", SETTINGS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
def test_plan_form_matches_oracle(references, env, case):
    _run_child(env, references[case])


def distinct_neighbour_centroids(c, cid):
    """Per query: how many distinct neighbour centroids its non-empty probed groups name over their non-empty
    sub-groups -- what plan_grouping4_kernel<true> enters into its hash set."""
    nc = c["nc"]
    sizes = np.diff(c["offsets"].astype(np.int64))
    out = []
    for row in cid:
        groups = row[row < nc]
        groups = groups[sizes[groups] != 0]
        nn = c["nn_centroid_idxs"][groups]
        out.append(np.unique(nn[c["subgroup_sizes"][groups] != 0]).size)
    return np.array(out)


def test_hash_set_overflow_is_gathered_directly(tmp_path):
    kw, nprobe, max_codes, ef = OVERFLOW
    c = synth.make_corpus(**kw)  # used here only: not kept in the session's cache
    npz, cid = _reference_file(str(tmp_path / "overflow.npz"), c, nprobe, max_codes, ef, (1,), False)
    # with pruning on and max_codes out of reach, pass 1 covers every non-empty probed group: all of them enter the set
    distinct = distinct_neighbour_centroids(c, cid)
    assert (distinct > GH_SLOTS).all(), distinct
    _run_child({"IVFHNSW_PLAN_DEDUPE": "1"}, npz)
