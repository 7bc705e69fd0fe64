"""Row values without a GPU: the symbols are declared and exported, the helper the GPU tests take their
expected values from (values_ref) is pinned, and the fixture conditions that keep a GPU test from passing vacuously hold on
every corpus those tests use."""
import os
import re

import numpy as np
import pytest

from conftest import corpus
import filter_ref
import values_ref as vr
from test_gpu_remove import BASE, CODE_SIZES, GROUPING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ivfhnsw_gpu_set_values", "ivfhnsw_gpu_set_values_dev", "ivfhnsw_gpu_clear_values", "ivfhnsw_gpu_values_info",
           "ivfhnsw_gpu_value_rows", "ivfhnsw_gpu_search_values", "ivfhnsw_gpu_search_values_dev",
           "ivfhnsw_gpu_range_search_values", "ivfhnsw_gpu_range_search_values_dev")


def base(**kw):
    return filter_ref.clipped(corpus(**kw))


def test_symbols_declared_and_listed(pkg):
    header = open(os.path.join(ROOT, "include", "ivfhnsw_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, header), s
        assert s in pkg.ABI_SYMBOLS, s
    assert re.search(r"#define\s+IVFHNSW_VALUE_NONE\s+0xffffffffu\b", header)
    assert pkg.VALUE_NONE == 0xffffffff == vr.NONE
    for m in ("set_values", "set_values_dev", "clear_values", "values_info", "value_rows", "search_values",
              "search_values_dev", "range_search_values", "range_search_values_dev"):
        assert callable(getattr(pkg.GpuIndex, m)), m


def test_abi_version_is_still_9():
    src = open(os.path.join(ROOT, "ivf-hnsw_amd", "csrc", "capi_handle.cpp")).read()
    assert re.search(r"ivfhnsw_gpu_abi_version\s*\(\s*(void)?\s*\)\s*\{\s*return\s+9\s*;", src)


def test_pattern_and_shares():
    assert vr.PATTERN == [(0, 0xffffffff), (0, 0xfffffffe), (0x80000000, 0x800000ff), (0x7fffff00, 0x800000ff), (77, 77),
                          (0, 0), (0x10000, 0x100ff), (5000, 4999), (1_000_007, 1_000_007)]
    qr = vr.query_ranges(20, first=3)
    assert qr.dtype == np.uint32 and qr.shape == (20, 2) and qr.flags["C_CONTIGUOUS"]
    assert [tuple(r) for r in qr[:7]] == vr.PATTERN[3:9] + vr.PATTERN[:1]
    assert np.array_equal(vr.query_ranges(64)[10:30], vr.query_ranges(20, first=10))
    b = base(**BASE)
    labels, values = vr.assignment(b)
    n = len(np.unique(b["ids"]))
    assert len(labels) == n and values.dtype == np.uint32 and np.array_equal(labels, np.unique(b["ids"]))
    v = values.astype(np.int64)
    band31 = (v >= 0x7fffff00) & (v <= 0x800000ff)
    band16 = (v >= 0xff00) & (v <= 0x100ff)
    rest = (v >= 1_000_000) & (v < 1_001_000)
    count = {"band31": int(band31.sum()), "zero": int((v == 0).sum()), "top": int((v == 0xfffffffe).sum()),
             "band16": int(band16.sum()), "point": int((v == 77).sum()), "none": int((v == vr.NONE).sum())}
    assert count == {"band31": n // 2, "zero": n // 10, "top": n // 10, "band16": n // 10, "point": n // 100, "none": n // 20}
    assert rest.sum() == n - sum(count.values())
    assert np.array_equal(v[band31], 0x7fffff00 + labels[band31].astype(np.int64) % 512)
    assert np.array_equal(v[band16], 0xff00 + labels[band16].astype(np.int64) % 512)
    assert np.array_equal(v[rest], 1_000_000 + labels[rest].astype(np.int64) % 1000)
    # both bands really straddle their boundary
    assert (v[band31] < 2 ** 31).any() and (v[band31] >= 2 ** 31).any()
    assert (v[band16] < 2 ** 16).any() and (v[band16] >= 2 ** 16).any()
    per = np.bincount(v[rest] - 1_000_000, minlength=1000)
    assert 3 <= per.mean() <= 5  # "about 4 rows each"
    assert np.array_equal(vr.assignment(b)[1], values) and not np.array_equal(vr.assignment(b, seed=99)[1], values)
    # rows: the full interval passes everything, (0, 0xfffffffe) everything but the rows without a value, the inverted one
    # nothing; an unknown id has no value
    asg = (labels, values)
    assert vr.passing_rows(b, asg, vr.FULL).all() and not vr.passing_rows(b, asg, vr.INVERTED).any()
    assert (~vr.passing_rows(b, asg, vr.VALUED)).sum() == np.isin(b["ids"], labels[values == vr.NONE]).sum() > 0
    assert vr.passing_rows(b, asg, vr.POINT).sum() == np.isin(b["ids"], vr.labels_in(asg, vr.POINT)).sum()
    assert list(vr.row_values(np.array([labels[0], 10 ** 9], np.uint32), asg)) == [values[0], vr.NONE]
    vl, vv = vr.valued(asg)
    assert len(vl) == n - n // 20 and not (vv == vr.NONE).any()


def test_reference_helper_is_pinned():
    """The full interval equals the plain oracle, an interval every id lies in equals it too, the inverted interval returns
    only padding."""
    b = base(**BASE)
    q = b["queries"][:32]
    ids = np.unique(b["ids"]).astype(np.uint32)
    asg = (ids, np.full(len(ids), 0x80000009, np.uint32))
    inside = (0x7fffffff, 0x80000009)
    for k in (1, 10):
        search = vr.oracle_search(vr.IVF_PARAMS, k)
        plain = search(b, q)
        refs = vr.per_range(search, b, asg, q, k, ranges=[vr.FULL, inside, vr.INVERTED])
        for r in (vr.FULL, inside):
            assert vr.same_bits(refs[r], (plain[0].reshape(32, k), plain[1].reshape(32, k))), r
        assert (refs[vr.INVERTED][1] == -1).all() and (refs[vr.INVERTED][0] == vr.FLT_MAX).all()
        qr = np.array([vr.FULL, vr.INVERTED, inside, vr.INVERTED] * 8, np.uint32)
        d, l = vr.compose(refs, qr)
        assert np.array_equal(l[0::4], plain[1].reshape(32, k)[0::4]) and (l[1::4] == -1).all()
        assert np.array_equal(l[2::4], plain[1].reshape(32, k)[2::4]) and (d[3::4] == vr.FLT_MAX).all()


# every corpus the GPU tests search with the common fixture, and the parameters they use
FIXTURE_CORPORA = [(kw, vr.IVF_PARAMS, False) for kw in CODE_SIZES] + \
                  [(GROUPING[0], vr.GROUPING_PARAMS, False), (GROUPING[0], vr.GROUPING_PARAMS, True),
                   (GROUPING[1], vr.GROUPING_PARAMS, False), (GROUPING[1], vr.GROUPING_PARAMS, True)]


def _cid(case):
    kw, _, pruning = case
    return "M%d%s%s" % (kw["M"], "-nsubc%d" % kw["nsubc"] if kw.get("nsubc") else "", "-pruned" if pruning else "")


@pytest.mark.parametrize("case", FIXTURE_CORPORA, ids=_cid)
def test_fixture_conditions(case):
    """At 128 queries, the smallest batch the GPU tests run, and k = 1: every non-empty interval of the pattern gives one of
    its queries a label, and every label returned has a value inside the interval; the inverted interval gives none;
    (0, 0xffffffff) and (0, 0xfffffffe) differ in one query's answer at least.  Where the GPU tests run k = 10 (BASE,
    Grouping): the 1 % point leaves one of its queries short of 10 and gives one a result."""
    kw, params, pruning = case
    b = base(**kw)
    asg = vr.assignment(b)
    q = vr.tiled(b["queries"], 128)
    qr = vr.query_ranges(128)
    search = vr.oracle_search(params, 1, pruning)
    refs = vr.per_range(search, b, asg, q, 1)
    for r in vr.PATTERN:
        mine = vr.mine(qr, r)
        assert mine.sum() >= 14
        got = refs[r][1][mine, 0]
        if r == vr.INVERTED:
            assert (got == -1).all()
        else:
            assert (got >= 0).any(), "interval %r: none of its queries returns a label" % (r,)
            assert np.isin(got[got >= 0], vr.labels_in(asg, r)).all()
    # the rows without a value decide an answer: the same queries under both intervals
    both = vr.per_range(search, b, asg, q, 1, ranges=[vr.FULL, vr.VALUED])
    assert (both[vr.FULL][1] != both[vr.VALUED][1]).any(), "(0, 0xffffffff) and (0, 0xfffffffe) answer alike"
    if kw == BASE or kw.get("nsubc"):
        r10 = vr.per_range(vr.oracle_search(params, 10, pruning), b, asg, q, 10, ranges=[vr.POINT])[vr.POINT][1]
        filled = (r10[vr.mine(qr, vr.POINT)] >= 0).sum(1)
        assert (filled < 10).any(), "no query of the 1 % point is left short of k = 10: padding is not exercised"
        assert (filled > 0).any()


def test_fixture_conditions_redo_case():
    """The overflow fixture: inside its interval the query still fills its k places, and its unfiltered nearest lies outside."""
    b, q, qr, asg, (nprobe, max_codes, ef, k) = vr.redo_case(base)
    assert [tuple(r) for r in qr] == [(100, 200), vr.FULL, vr.INVERTED]
    refs = vr.per_range(vr.oracle_search((nprobe, max_codes, ef), k), b, asg, q, k, ranges=qr)
    other = vr.labels_in(asg, (0x80000005, 0x80000005))
    assert (refs[(100, 200)][1][0] >= 0).all() and not np.isin(refs[(100, 200)][1][0], other).any()
    assert np.isin(refs[vr.FULL][1][1], other).any()
    assert (refs[vr.INVERTED][1] == -1).all()
