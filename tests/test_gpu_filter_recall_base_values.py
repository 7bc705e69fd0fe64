"""tools/filter_recall.py --base-values on a small corpus.  With its queries restricted to the ten sample
intervals it prints the recall figures --values prints -- two exact truths, ONE exact_search_values call and the
per-interval loop of set_base_filter + exact_search, agree to the digit -- and with an interval per query its truth equals
the loop's, interval by interval."""
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


def test_the_sample_intervals_give_the_figures_of_values_recall(pkg):
    c = _corpus()
    loop = filter_recall.values_recall(pkg, seed=5, corpus=c, settings=SETTING)
    one = filter_recall.base_values_recall(pkg, seed=5, corpus=c, settings=SETTING, sample_only=True)
    assert one["intervals"] == loop["intervals"] == 10
    assert one["base_values_recall"] == loop["values_recall"]  # every figure, to the digit
    assert all(r["queries"] > 0 and 0.0 <= r["recall_at_10"] <= 1.0 for r in one["base_values_recall"])


def test_the_one_call_truth_equals_the_per_interval_loop(gpu, pkg):
    c = _corpus()
    out = filter_recall.base_values_recall(pkg, seed=5, corpus=c, settings=SETTING)
    qr, truth, values = out["query_ranges"], out["truth"], out["values_of_rows"]
    nq = len(c["queries"])
    assert qr.shape == (nq, 2) and truth.shape == (nq, 10) and sorted(values.tolist()) == list(range(8000))
    assert out["intervals"] == np.unique(qr, axis=0).shape[0] > 30  # a batch of distinct intervals, not the ten samples
    assert sum(r["queries"] for r in out["base_values_recall"]) == nq
    g = gpu()
    g.upload_base(c["base"])
    q8 = c["queries"].astype(np.uint8)
    for lo, hi in np.unique(qr, axis=0):
        mine = np.flatnonzero((qr[:, 0] == lo) & (qr[:, 1] == hi))
        g.set_base_filter(np.flatnonzero((values >= lo) & (values <= hi)).astype(np.uint32))
        assert np.array_equal(g.exact_search(q8[mine], 10)[1], truth[mine]), (lo, hi)
    g.close()
