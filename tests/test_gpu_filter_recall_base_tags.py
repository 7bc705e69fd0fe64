"""tools/filter_recall.py --base-tags on a small corpus: its truth, ONE exact_search_tags call over queries
dealt over the tags, equals per tag of TAG_SAMPLE -- and per every other tag its queries name -- what the per-tag loop of
tags_recall gives: set_base_filter(rows of the tag) + exact_search on the tag's queries."""
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


def test_the_one_call_truth_equals_the_per_tag_loop(gpu, pkg):
    c = _corpus()
    out = filter_recall.base_tags_recall(pkg, seed=5, corpus=c, settings=SETTING)
    qt, truth, tags = out["query_tags"], out["truth"], out["tags_of_rows"]
    nq = len(c["queries"])
    assert len(qt) == nq and truth.shape == (nq, 10) and np.array_equal(tags, filter_recall.tag_assignment(8000, 5))
    assert np.unique(qt).size == nq  # every query its own tag: 99 of the 1 025
    assert set(filter_recall.TAG_SAMPLE) <= set(qt.tolist())
    assert sum(r["queries"] for r in out["base_tags_recall"]) == nq
    assert all(0.0 <= r["recall_at_10"] <= 1.0 for r in out["base_tags_recall"])
    # the truth, tag by tag, as tags_recall computes it
    g = gpu()
    g.upload_base(c["base"])
    q8 = c["queries"].astype(np.uint8)
    for t in list(filter_recall.TAG_SAMPLE) + sorted(set(qt.tolist()) - set(filter_recall.TAG_SAMPLE)):
        mine = np.flatnonzero(qt == t)
        if t == filter_recall.TAG_NONE:
            g.clear_base_filter()
        else:
            g.set_base_filter(np.flatnonzero(tags == t).astype(np.uint32))
        assert np.array_equal(g.exact_search(q8[mine], 10)[1], truth[mine]), t
    g.close()
