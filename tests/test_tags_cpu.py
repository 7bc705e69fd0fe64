"""Row tags without a GPU: the symbols are declared and exported, the helper the GPU tests take their
expected values from (tags_ref) is pinned, and the fixture conditions that keep a GPU test from passing vacuously hold on
every corpus those tests use."""
import os
import re

import numpy as np
import pytest

from conftest import corpus
import filter_ref
import tags_ref as tr
from test_gpu_remove import BASE, CODE_SIZES, GROUPING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ivfhnsw_gpu_set_tags", "ivfhnsw_gpu_set_tags_dev", "ivfhnsw_gpu_clear_tags", "ivfhnsw_gpu_tags_info",
           "ivfhnsw_gpu_tag_rows", "ivfhnsw_gpu_search_tags", "ivfhnsw_gpu_search_tags_dev",
           "ivfhnsw_gpu_range_search_tags", "ivfhnsw_gpu_range_search_tags_dev")


def base(**kw):
    return filter_ref.clipped(corpus(**kw))


def test_symbols_declared_and_listed(pkg):
    header = open(os.path.join(ROOT, "include", "ivfhnsw_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, header), s
        assert s in pkg.ABI_SYMBOLS, s
    assert re.search(r"#define\s+IVFHNSW_TAG_NONE\s+0xffffu\b", header)
    assert pkg.TAG_NONE == 0xffff == tr.NONE
    for m in ("set_tags", "set_tags_dev", "clear_tags", "tags_info", "tag_rows", "search_tags", "search_tags_dev",
              "range_search_tags", "range_search_tags_dev"):
        assert callable(getattr(pkg.GpuIndex, m)), m


def test_abi_version_is_still_9():
    src = open(os.path.join(ROOT, "ivf-hnsw_amd", "csrc", "capi_handle.cpp")).read()
    assert re.search(r"ivfhnsw_gpu_abi_version\s*\(\s*(void)?\s*\)\s*\{\s*return\s+9\s*;", src)


def test_pattern_and_partition():
    assert tr.PATTERN == [0, 0xfffe, 0xffff, 1, 255, 256, 4242, 1007, 0xfffe] and tr.ABSENT == 4242
    qt = tr.query_tags(20, first=3)
    assert qt.dtype == np.uint16 and list(qt[:7]) == [1, 255, 256, 4242, 1007, 0xfffe, 0]
    assert np.array_equal(tr.query_tags(64)[10:30], tr.query_tags(20, first=10))
    b = base(**BASE)
    labels, tags = tr.assignment(b)
    n = len(np.unique(b["ids"]))
    assert len(labels) == n and tags.dtype == np.uint16 and np.array_equal(labels, np.unique(b["ids"]))
    count = {t: int((tags == t).sum()) for t in (0, 1, 255, 256, 0xfffe, tr.NONE)}
    assert count == {0: n // 2, 1: n // 100, 255: n // 10, 256: n // 10, 0xfffe: n // 10, tr.NONE: n // 20}
    rest = ~np.isin(tags, list(count))
    assert rest.sum() == n - sum(count.values()) and np.array_equal(tags[rest], 1000 + labels[rest] % 1000)
    assert not (tags == tr.ABSENT).any()
    per = np.bincount(tags[rest] - 1000, minlength=1000)
    assert 3 <= per.mean() <= 5  # "about 4 rows each"
    assert np.array_equal(tr.assignment(b)[1], tags) and not np.array_equal(tr.assignment(b, seed=99)[1], tags)
    # rows: a tag's rows are the rows of its labels, NONE passes everything, an unknown id is untagged
    assert tr.passing_rows(b, (labels, tags), tr.NONE).all() and not tr.passing_rows(b, (labels, tags), tr.ABSENT).any()
    assert tr.passing_rows(b, (labels, tags), 255).sum() == np.isin(b["ids"], tr.labels_of((labels, tags), 255)).sum()
    assert list(tr.row_tags(np.array([labels[0], 10 ** 9], np.uint32), (labels, tags))) == [tags[0], tr.NONE]
    tl, tt = tr.tagged((labels, tags))
    assert len(tl) == n - n // 20 and not (tt == tr.NONE).any()


def test_reference_helper_is_pinned():
    """NONE equals the plain oracle, a tag every id carries equals it too, a tag no id carries returns only padding."""
    b = base(**BASE)
    q = b["queries"][:32]
    ids = np.unique(b["ids"]).astype(np.uint32)
    asg = (ids, np.full(len(ids), 9, np.uint16))
    for k in (1, 10):
        search = tr.oracle_search(tr.IVF_PARAMS, k)
        plain = search(b, q)
        refs = tr.per_tag(search, b, asg, q, k, tags=[tr.NONE, 9, tr.ABSENT])
        for t in (tr.NONE, 9):
            assert tr.same_bits(refs[t], (plain[0].reshape(32, k), plain[1].reshape(32, k))), t
        assert (refs[tr.ABSENT][1] == -1).all() and (refs[tr.ABSENT][0] == tr.FLT_MAX).all()
        qt = np.array([tr.NONE, tr.ABSENT, 9, tr.ABSENT] * 8, np.uint16)
        d, l = tr.compose(refs, qt)
        assert np.array_equal(l[0::4], plain[1].reshape(32, k)[0::4]) and (l[1::4] == -1).all()
        assert np.array_equal(l[2::4], plain[1].reshape(32, k)[2::4]) and (d[3::4] == tr.FLT_MAX).all()


# every corpus the GPU tests search with the common fixture, and the parameters they use
FIXTURE_CORPORA = [(kw, tr.IVF_PARAMS, False) for kw in CODE_SIZES] + \
                  [(GROUPING[0], tr.GROUPING_PARAMS, False), (GROUPING[0], tr.GROUPING_PARAMS, True),
                   (GROUPING[1], tr.GROUPING_PARAMS, False), (GROUPING[1], tr.GROUPING_PARAMS, True)]


def _cid(case):
    kw, _, pruning = case
    return "M%d%s%s" % (kw["M"], "-nsubc%d" % kw["nsubc"] if kw.get("nsubc") else "", "-pruned" if pruning else "")


@pytest.mark.parametrize("case", FIXTURE_CORPORA, ids=_cid)
def test_fixture_conditions(case):
    """At 128 queries, the smallest batch the GPU tests run, and k = 1: every tag of the pattern but 4242 gives one of its
    queries a label and 4242 gives none; for every tagged pattern entry one of its queries has an unfiltered winner that
    carries a different tag.  Where the GPU tests run k = 10 (BASE, Grouping): a query tagged 1 is left short of 10."""
    kw, params, pruning = case
    b = base(**kw)
    asg = tr.assignment(b)
    q = tr.tiled(b["queries"], 128)
    qt = tr.query_tags(128)
    refs = tr.per_tag(tr.oracle_search(params, 1, pruning), b, asg, q, 1)
    plain = refs[tr.NONE][1][:, 0]
    for t in set(tr.PATTERN) - {tr.NONE}:
        mine = qt == t
        assert mine.sum() >= 14
        got = refs[t][1][mine, 0]
        if t == tr.ABSENT:
            assert (got == -1).all()
        else:
            assert (got >= 0).any(), "tag %d: none of its queries returns a label" % t
            assert np.isin(got[got >= 0], tr.labels_of(asg, t)).all()
        w = plain[mine]
        w = w[w >= 0].astype(np.uint32)
        assert (tr.row_tags(w, asg) != t).any(), "tag %d: every unfiltered winner of its queries carries it" % t
    if kw == BASE or kw.get("nsubc"):
        r10 = tr.per_tag(tr.oracle_search(params, 10, pruning), b, asg, q, 10, tags=[1])[1][1]
        filled = (r10[qt == 1] >= 0).sum(1)
        assert (filled < 10).any(), "no query of the 1 % tag is left short of k = 10: padding is not exercised"


def test_fixture_conditions_redo_case():
    """The overflow fixture: under its tag the query still fills its k places, and its unfiltered nearest carries another."""
    b, q, qt, asg, (nprobe, max_codes, ef, k) = tr.redo_case(base)
    assert list(qt) == [0xfffe, tr.NONE, tr.ABSENT]
    refs = tr.per_tag(tr.oracle_search((nprobe, max_codes, ef), k), b, asg, q, k, tags=qt)
    other = tr.labels_of(asg, 255)
    assert (refs[0xfffe][1][0] >= 0).all() and not np.isin(refs[0xfffe][1][0], other).any()
    assert np.isin(refs[tr.NONE][1][1], other).any()
    assert (refs[tr.ABSENT][1] == -1).all()
