"""tools/filter_recall.py --slots on a small corpus: its truth, one exact_search_slots call, equals the truth
of the single base filter slot by slot, and its recall at pass fraction 1/2 equals what the tool's per-fraction function
computes for the same set and queries."""
import os
import sys

import numpy as np
import pytest

from conftest import corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import filter_recall  # noqa: E402

pytestmark = pytest.mark.gpu

SETTING = ((8, 2000, 40),)


def _corpus():
    c = dict(corpus(seed=7, nc=128, d=128, M=16, n_base=8000, nq=99, efConstruction=100))
    gr = c["graph"]
    c.update(counts=gr.counts, links=gr.links, centroids=gr.vectors, enterpoint=gr.enterpoint,
             base=np.clip(np.rint(c["base"]), 0, 255).astype(np.uint8),
             queries=np.clip(np.rint(c["queries"]), 0, 255).astype(np.float32))
    return c


def test_the_slot_run_equals_the_single_filter_runs(gpu, pkg):
    c = _corpus()
    out = filter_recall.slots_recall(pkg, seed=5, corpus=c, settings=SETTING)
    qs, truth, sets = out["query_slots"], out["truth"], out["sets"]
    nq = len(c["queries"])
    assert len(sets) == 32 and set(qs.tolist()) == set(range(32)) | {0xff} and len(qs) == nq
    assert [len(s) for s in sets[:3]] == [8000 // 2, 8000 // 8, 8000 // 32]
    assert {r["pass_fraction"] for r in out["slots_recall"]} == {"1/1", "1/2", "1/8", "1/32"}
    assert sum(r["queries"] for r in out["slots_recall"]) == nq
    # the truth, slot by slot, from the single base filter
    g = gpu()
    g.upload_base(c["base"])
    q8 = c["queries"].astype(np.uint8)
    for b in list(range(32)) + [0xff]:
        idx = np.flatnonzero(qs == b)
        if b == 0xff:
            g.clear_base_filter()
        else:
            g.set_base_filter(sets[b])
        assert np.array_equal(g.exact_search(q8[idx], 10)[1], truth[idx]), b
    g.close()
    # slot 0 holds half the rows: the per-fraction function on the same set and queries
    idx = np.flatnonzero(qs == 0)
    one = filter_recall.filtered_recall(pkg, corpus=c, allow_sets=[("slot 0", sets[0])], query_idx=idx, settings=SETTING)
    row = one["filtered_recall"][0]
    assert (row["recall_at_1"], row["recall_at_10"]) == out["per_slot"][0][0]
    assert 0.0 < row["recall_at_10"] <= 1.0
