"""tests/grouping_append_ref.py (the expected state of every ivfhnsw_gpu_append_grouping / add_groups test) pinned
without a GPU: against an independent formulation (one stable sort of all old and new rows), against itself in one and
in ten batches, and through the oracle's search: half the groups plus the other half added = the full corpus."""
import numpy as np
import pytest

import grouping_append_ref as gar
import synth

CASES = [dict(seed=97, nc=128, n_base=9000, nq=48, efConstruction=80, nsubc=8),
         dict(seed=97, nc=128, n_base=9000, nq=48, efConstruction=80, nsubc=64, opq=True),
         dict(seed=97, nc=128, d=32, M=4, n_base=9000, nq=48, efConstruction=80, nsubc=5)]
KEYS = ("offsets", "ids", "codes", "norm_codes", "subgroup_sizes")


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]).reshape(-1), np.asarray(b[k]).reshape(-1)) and
               np.asarray(a[k]).dtype == np.asarray(b[k]).dtype for k in KEYS)


def _merge(part, batch, sel=slice(None)):
    return gar.merge_lists(part["offsets"], part["ids"], part["codes"], part["norm_codes"], part["subgroup_sizes"],
                           batch["list_idx"][sel], batch["sub_idx"][sel], batch["ids"][sel], batch["codes"][sel],
                           batch["norm_codes"][sel])


def _by_one_sort(part, batch):
    """All rows, old then new in arrival order, stably sorted by (list, sub-group)."""
    lst, sub = gar.rows_of(part["offsets"], part["subgroup_sizes"])
    nc, nsubc = part["subgroup_sizes"].shape
    L = np.concatenate([lst, batch["list_idx"].astype(np.int64)])
    S = np.concatenate([sub, batch["sub_idx"].astype(np.int64)])
    order = np.argsort(L * nsubc + S, kind="stable")
    ids = np.concatenate([part["ids"], batch["ids"]])[order]
    codes = np.concatenate([part["codes"].reshape(len(part["ids"]), -1), batch["codes"]])[order]
    ncodes = np.concatenate([part["norm_codes"], batch["norm_codes"]])[order]
    sg = np.bincount(L * nsubc + S, minlength=nc * nsubc).reshape(nc, nsubc).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(sg.sum(1))]).astype(np.uint64)
    return dict(offsets=off, ids=ids, codes=np.ascontiguousarray(codes), norm_codes=ncodes, subgroup_sizes=sg)


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "nsubc%d" % kw["nsubc"])
def test_merge_equals_one_stable_sort_and_any_batching(kw):
    c = synth.make_corpus(**kw)
    rng = np.random.default_rng(5)
    part, batch = gar.split_corpus(c, gar.tail_mask(c, rng))
    # arrival order differs from CSR order: a shuffled batch must still land in ascending i inside every sub-group
    p = rng.permutation(len(batch["ids"]))
    shuffled = {k: v[p] for k, v in batch.items()}
    for b in (batch, shuffled):
        assert _same(_merge(part, b), _by_one_sort(part, b))
    assert _same(_merge(part, batch), c)           # tails held back and put back: the full corpus again
    assert not _same(part, c)
    cur = part
    for sel in np.array_split(np.arange(len(p)), 10):
        cur = dict(part, **_merge(cur, shuffled, sel))
    assert _same(cur, _merge(part, shuffled))


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "nsubc%d" % kw["nsubc"])
@pytest.mark.parametrize("pruning", [False, True])
def test_oracle_on_half_plus_added_half_equals_full(kw, pruning):
    c = synth.make_corpus(**kw)
    rng = np.random.default_rng(6)
    gone = rng.random(c["nc"]) < 0.5
    part, held = gar.without_groups(c, gone)
    _, batch = gar.split_corpus(c, held)
    merged = dict(c, **_merge(part, batch))
    assert _same(merged, c)
    full = synth.oracle_index(c)
    again = synth.oracle_index(merged)
    for ox in (full, again):
        ox.set_params(16, 2000, 40, do_pruning=pruning)
    a = full.search_batch(c["queries"], k=10)
    b = again.search_batch(c["queries"], k=10)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    lab = a[1].reshape(len(c["queries"]), -1)
    assert (lab >= 0).all()
    lst, _ = gar.rows_of(c["offsets"], c["subgroup_sizes"])
    list_of_id = np.empty(int(c["ids"].max()) + 1, np.int64)
    list_of_id[c["ids"]] = lst
    top1_added = gone[list_of_id[lab[:, 0]]]
    assert top1_added.any() and (~top1_added).any()
    # half the groups alone answer differently: the added half matters
    half = synth.oracle_index(dict(part, alphas=c["alphas"], nn_centroid_idxs=c["nn_centroid_idxs"],
                                   inter_centroid_dists=c["inter_centroid_dists"]))
    half.set_params(16, 2000, 40, do_pruning=pruning)
    assert not np.array_equal(half.search_batch(c["queries"], k=10)[1], a[1])
