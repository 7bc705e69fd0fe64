"""Tag AND value without a GPU: the symbols are declared and exported, the helper the GPU tests take their
expected values from (tags_values_ref) is pinned, and the fixture conditions that keep a GPU test from passing vacuously
hold on every corpus those tests use.  These tests pin the fixture only; the symbol test fails without the feature."""
import math
import os
import re

import numpy as np
import pytest

from conftest import corpus
import filter_ref
import tags_ref as tr
import tags_values_ref as tv
import values_ref as vr
from test_gpu_remove import BASE, CODE_SIZES, GROUPING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ivfhnsw_gpu_search_tags_values", "ivfhnsw_gpu_search_tags_values_dev", "ivfhnsw_gpu_range_search_tags_values",
           "ivfhnsw_gpu_range_search_tags_values_dev", "ivfhnsw_gpu_tag_value_rows")
# rows that pass, over all corpora (the CPU check of the pattern's table), by pair
ROWS = {(0, tv.BAND31): (984, 7564), (255, (0, 0)): (38, 301), (256, tv.VALUED): (382, 2861), (0xfffe, tv.UPPER31): (105, 762),
        (0, tv.POINT): (18, 154), tv.FEW: (2, 6), (0, (tv.VALUE_NONE, tv.VALUE_NONE)): (92, 758)}


def base(**kw):
    return filter_ref.clipped(corpus(**kw))


def test_symbols_declared_and_listed(pkg):
    header = open(os.path.join(ROOT, "include", "ivfhnsw_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, header), s
        assert s in pkg.ABI_SYMBOLS, s
        getattr(pkg.lib(), s)
    for m in ("search_tags_values", "search_tags_values_dev", "range_search_tags_values", "range_search_tags_values_dev",
              "tag_value_rows"):
        assert callable(getattr(pkg.GpuIndex, m)), m
    # the argument order is the twins': the tags where _tags has them, the ranges behind them
    assert re.search(r"ivfhnsw_gpu_search_tags_values\s*\([^)]*params,\s*const uint16_t \*query_tags,\s*const uint32_t \*query_ranges,"
                     r"\s*float \*distances", header)
    assert re.search(r"ivfhnsw_gpu_tag_value_rows\s*\(ivfhnsw_gpu \*h, unsigned tag, uint32_t lo, uint32_t hi, uint64_t \*rows\)",
                     header)


def test_abi_version_is_still_9():
    src = open(os.path.join(ROOT, "ivf-hnsw_amd", "csrc", "capi_handle.cpp")).read()
    assert re.search(r"ivfhnsw_gpu_abi_version\s*\(\s*(void)?\s*\)\s*\{\s*return\s+9\s*;", src)


def test_pattern():
    assert len(tv.PATTERN) == 13 and all(math.gcd(13, n) == 1 for n in (64, 2048, 8192))
    assert len({tv.key(p) for p in tv.PATTERN}) == 13
    for p in [(0xffff, (0, 0xffffffff)), (0, (0, 0xffffffff)), (0xffff, (0x80000000, 0x800000ff)), (0, (0x7fffff00, 0x800000ff)),
              (255, (0, 0)), (256, (0, 0xfffffffe)), (0xfffe, (0x80000000, 0x800000ff)), (0, (77, 77)), (1007, (0, 0xffffffff)),
              (0, (0xffffffff, 0xffffffff)), (4242, (0, 0xffffffff)), (0, (5000, 4999)), (256, (0, 0))]:
        assert p in [tv.key(x) for x in tv.PATTERN], p
    qt, qr = tv.query_tags(30, first=5), tv.query_ranges(30, first=5)
    assert qt.dtype == np.uint16 and qt.shape == (30,) and qr.dtype == np.uint32 and qr.shape == (30, 2)
    assert qr.flags["C_CONTIGUOUS"]
    assert [(int(t), (int(r[0]), int(r[1]))) for t, r in zip(qt[:10], qr[:10])] == [tv.key(p) for p in tv.PATTERN[5:] + tv.PATTERN[:2]]
    assert np.array_equal(tv.query_tags(64)[10:30], tv.query_tags(20, first=10))
    assert np.array_equal(tv.query_ranges(64)[10:30], tv.query_ranges(20, first=10))


def test_assignment_is_the_two_with_one_change():
    b = base(**BASE)
    labels, tags, values = tv.assignment(b)
    lt, t0 = tr.assignment(b)
    lv, v0 = vr.assignment(b)
    assert np.array_equal(labels, lt) and np.array_equal(labels, lv) and np.array_equal(tags, t0)
    changed = values != v0
    assert changed.any() and (tags[changed] == 256).all() and (v0[changed] == 0).all() and (values[changed] == 1).all()
    assert not ((tags == 256) & (values == 0)).any()
    asg = (labels, tags, values)
    # the helper against the two it is made of: a wildcard on one side is the other side's rule
    for t in (0, 255, 1007, tv.ABSENT, tv.TAG_NONE):
        assert np.array_equal(tv.passing_rows(b, asg, (t, tv.FULL)), tr.passing_rows(b, tv.tag_asg(asg), t)), t
    for r in vr.PATTERN:
        assert np.array_equal(tv.passing_rows(b, asg, (tv.TAG_NONE, r)), vr.passing_rows(b, tv.value_asg(asg), r)), r
    for p in tv.PATTERN:
        m = tv.passing_rows(b, asg, p)
        assert np.array_equal(m, tr.passing_rows(b, tv.tag_asg(asg), p[0]) & vr.passing_rows(b, tv.value_asg(asg), p[1])), p
        assert m.sum() == np.isin(b["ids"], tv.labels_in(asg, p)).sum(), p
    none = tv.without(asg, tags=False)
    assert not tv.passing_rows(b, none, (0, tv.FULL)).any() and tv.passing_rows(b, none, (tv.TAG_NONE, tv.FULL)).all()
    none = tv.without(asg, values=False)
    assert not tv.passing_rows(b, none, (0, tv.VALUED)).any()
    assert np.array_equal(tv.passing_rows(b, none, (0, tv.FULL)), tv.passing_rows(b, asg, (0, tv.FULL)))


def test_reference_helper_is_pinned():
    """(NONE, FULL) equals the plain oracle, a pair every id passes equals it too, a pair no id passes returns padding."""
    b = base(**BASE)
    q = b["queries"][:32]
    ids = np.unique(b["ids"]).astype(np.uint32)
    asg = (ids, np.full(len(ids), 300, np.uint16), np.full(len(ids), 0x80000009, np.uint32))
    inside, outside = (300, (0x7fffffff, 0x80000009)), (301, (0x7fffffff, 0x80000009))
    for k in (1, 10):
        search = tv.oracle_search(tv.IVF_PARAMS, k)
        plain = search(b, q)
        refs = tv.per_pair(search, b, asg, q, k, pairs=[tv.UNFILTERED, inside, outside])
        for p in (tv.UNFILTERED, inside):
            assert tv.same_bits(refs[tv.key(p)], (plain[0].reshape(32, k), plain[1].reshape(32, k))), p
        assert (refs[outside][1] == -1).all() and (refs[outside][0] == tv.FLT_MAX).all()
        qt = np.array([0xffff, 301, 300, 301] * 8, np.uint16)
        qr = np.array([tv.FULL, inside[1], inside[1], inside[1]] * 8, np.uint32)
        d, l = tv.compose(refs, qt, qr)
        assert np.array_equal(l[0::4], plain[1].reshape(32, k)[0::4]) and (l[1::4] == -1).all()
        assert np.array_equal(l[2::4], plain[1].reshape(32, k)[2::4]) and (d[3::4] == tv.FLT_MAX).all()


# every corpus the GPU tests search with the common fixture, and the parameters they use
FIXTURE_CORPORA = [(kw, tv.IVF_PARAMS, False) for kw in CODE_SIZES] + \
                  [(GROUPING[0], tv.GROUPING_PARAMS, False), (GROUPING[0], tv.GROUPING_PARAMS, True),
                   (GROUPING[1], tv.GROUPING_PARAMS, False), (GROUPING[1], tv.GROUPING_PARAMS, True)]


def _cid(case):
    kw, _, pruning = case
    return "M%d%s%s" % (kw["M"], "-nsubc%d" % kw["nsubc"] if kw.get("nsubc") else "", "-pruned" if pruning else "")


@pytest.mark.parametrize("case", FIXTURE_CORPORA, ids=_cid)
def test_fixture_conditions(case):
    """Rows: every non-padding pair passes a row; (256, (0, 0)) passes none while tag 256 alone and (0, 0) alone pass some;
    (1007, FULL) passes fewer than 10.  Answers, at 128 queries (the smallest batch the GPU tests run) and k = 1: every
    non-padding pair gives one of its queries a label, every label returned passes the pair, and the padding pairs give
    none.  Where the GPU tests run k = 10 (BASE, Grouping): (1007, FULL) leaves its queries short of 10."""
    kw, params, pruning = case
    b = base(**kw)
    asg = tv.assignment(b)
    n = len(b["ids"])
    rows = {tv.key(p): int(tv.passing_rows(b, asg, p).sum()) for p in tv.PATTERN}
    assert rows[tv.key(tv.UNFILTERED)] == n
    assert 0.45 * n <= rows[(0, tv.FULL)] <= 0.55 * n
    assert 0.20 * n <= rows[(tv.TAG_NONE, tv.UPPER31)] <= 0.30 * n
    for p, (lo, hi) in ROWS.items():
        assert lo <= rows[tv.key(p)] <= hi, (p, rows[tv.key(p)])
    for p in tv.PATTERN:
        assert (rows[tv.key(p)] == 0) == (p in tv.PADDING), p
    assert tv.passing_rows(b, asg, (256, tv.FULL)).sum() > 0.05 * n
    assert tv.passing_rows(b, asg, (tv.TAG_NONE, (0, 0))).sum() > 0.05 * n
    assert rows[tv.key(tv.FEW)] < 10

    q = tv.tiled(b["queries"], 128)
    qt, qr = tv.query_tags(128), tv.query_ranges(128)
    refs = tv.per_pair(tv.oracle_search(params, 1, pruning), b, asg, q, 1)
    for p in tv.PATTERN:
        mine = tv.mine(qt, qr, p)
        assert mine.sum() >= 9
        got = refs[tv.key(p)][1][mine, 0]
        if p in tv.PADDING:
            assert (got == -1).all()
        else:
            assert (got >= 0).any(), "pair %r: none of its queries returns a label" % (p,)
            assert np.isin(got[got >= 0], tv.labels_in(asg, p)).all()
    if kw == BASE or kw.get("nsubc"):
        r10 = tv.per_pair(tv.oracle_search(params, 10, pruning), b, asg, q, 10, pairs=[tv.FEW])[tv.key(tv.FEW)][1]
        filled = (r10[tv.mine(qt, qr, tv.FEW)] >= 0).sum(1)
        assert (filled < 10).all() and (filled > 0).any()
