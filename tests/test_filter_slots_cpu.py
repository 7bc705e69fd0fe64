"""Filter slots without a GPU: the symbols are declared and exported, the helper the GPU tests take their
expected values from (filter_slots_ref) is pinned, and the fixture conditions that keep a GPU test from passing
vacuously hold on every corpus those tests use."""
import os
import re

import numpy as np
import pytest

from conftest import corpus
import filter_ref
import filter_slots_ref as fs
import synth
from test_gpu_remove import BASE, CODE_SIZES, GROUPING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ivfhnsw_gpu_set_filter_slot", "ivfhnsw_gpu_set_filter_slot_dev", "ivfhnsw_gpu_clear_filter_slot",
           "ivfhnsw_gpu_filter_slot_info", "ivfhnsw_gpu_search_slots", "ivfhnsw_gpu_search_slots_dev",
           "ivfhnsw_gpu_range_search_slots", "ivfhnsw_gpu_range_search_slots_dev")


def base(**kw):
    return filter_ref.clipped(corpus(**kw))


def test_symbols_declared_and_listed(pkg):
    header = open(os.path.join(ROOT, "include", "ivfhnsw_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, header), s
        assert s in pkg.ABI_SYMBOLS, s
    assert re.search(r"#define\s+IVFHNSW_FILTER_SLOTS\s+32\b", header)
    assert re.search(r"#define\s+IVFHNSW_SLOT_NONE\s+0xff\b", header)
    assert (pkg.FILTER_SLOTS, pkg.SLOT_NONE) == (32, 0xff) and fs.NONE == pkg.SLOT_NONE
    for m in ("set_filter_slot", "set_filter_slot_dev", "clear_filter_slot", "filter_slot_info", "search_slots",
              "search_slots_dev", "range_search_slots", "range_search_slots_dev"):
        assert callable(getattr(pkg.GpuIndex, m)), m


def test_abi_version_is_still_9():
    src = open(os.path.join(ROOT, "ivf-hnsw_amd", "csrc", "capi_handle.cpp")).read()
    assert re.search(r"ivfhnsw_gpu_abi_version\s*\(\s*(void)?\s*\)\s*\{\s*return\s+9\s*;", src)


def test_pattern_and_sets():
    assert fs.PATTERN == [0, 31, fs.NONE, 1, 7, 5, 31] and fs.UNSET == 5 and fs.UNSET not in fs.SPECS
    qs = fs.query_slots(20, first=3)
    assert qs.dtype == np.uint8 and list(qs[:5]) == [1, 7, 5, 31, 0]
    assert np.array_equal(fs.query_slots(64)[10:30], fs.query_slots(20, first=10))
    b = base(**BASE)
    assert len(b["ids"]) % 64 != 0 and len(b["ids"]) % 32 != 0  # the plane stride is rounded
    sets = fs.slot_sets(b)
    n = len(np.unique(b["ids"]))
    assert {s: (len(v[0]), v[1]) for s, v in sets.items()} == \
        {0: (n // 2, False), 1: (n // 100, False), 7: (n // 10, True), 31: (n // 10, False)}
    assert not np.array_equal(sets[7][0], sets[31][0])
    assert fs.passing_rows(b, sets, fs.NONE).all() and not fs.passing_rows(b, sets, fs.UNSET).any()
    assert fs.passing_rows(b, sets, 7).sum() == len(b["ids"]) - n // 10


def test_reference_helper_is_pinned():
    """NONE equals the plain oracle, a deny-nothing slot equals it too, an allow-nothing slot returns only padding."""
    b = base(**BASE)
    q = b["queries"][:32]
    for k in (1, 10):
        search = fs.oracle_search(fs.IVF_PARAMS, k)
        plain = search(b, q)
        sets = {2: (np.zeros(0, np.uint32), True), 3: (np.zeros(0, np.uint32), False)}
        refs = fs.per_slot(search, b, sets, q, k, slots=[fs.NONE, 2, 3, fs.UNSET])
        for s in (fs.NONE, 2):
            assert fs.same_bits(refs[s], (plain[0].reshape(32, k), plain[1].reshape(32, k))), s
        for s in (3, fs.UNSET):
            assert (refs[s][1] == -1).all() and (refs[s][0] == fs.FLT_MAX).all(), s
        qs = np.array([fs.NONE, 3, 2, fs.UNSET] * 8, np.uint8)
        d, l = fs.compose(refs, qs)
        assert np.array_equal(l[0::4], plain[1].reshape(32, k)[0::4]) and (l[1::4] == -1).all()
        assert np.array_equal(l[2::4], plain[1].reshape(32, k)[2::4]) and (d[3::4] == fs.FLT_MAX).all()
        # rows taken through base_index: query i of a tiled batch is base query i % 32
        d2, l2 = fs.compose(refs, np.full(64, 2, np.uint8), np.arange(64) % 32)
        assert np.array_equal(l2[32:], plain[1].reshape(32, k))


# every corpus the GPU tests search with the common fixture, and the parameters they use
FIXTURE_CORPORA = [(kw, fs.IVF_PARAMS, False) for kw in CODE_SIZES] + \
                  [(GROUPING[0], fs.GROUPING_PARAMS, False), (GROUPING[0], fs.GROUPING_PARAMS, True),
                   (GROUPING[1], fs.GROUPING_PARAMS, False), (GROUPING[1], fs.GROUPING_PARAMS, True)]


def _cid(case):
    kw, _, pruning = case
    return "M%d%s%s" % (kw["M"], "-nsubc%d" % kw["nsubc"] if kw.get("nsubc") else "", "-pruned" if pruning else "")


@pytest.mark.parametrize("case", FIXTURE_CORPORA, ids=_cid)
def test_fixture_conditions(case):
    """For each of slots 0, 1, 7 and 31: one of its queries returns a label, and one of its queries has an unfiltered
    winner that does not pass -- at 128 queries, the smallest batch the GPU tests run."""
    kw, params, pruning = case
    b = base(**kw)
    import test_gpu_filter
    assert test_gpu_filter.GROUPING == GROUPING[1]  # the Grouping corpus of test_gpu_filter is covered by this list
    sets = fs.slot_sets(b)
    q = fs.tiled(b["queries"], 128)
    qs = fs.query_slots(128)
    refs = fs.per_slot(fs.oracle_search(params, 1, pruning), b, sets, q, 1)
    plain = refs[fs.NONE][1][:, 0]
    for s in fs.SPECS:
        mine = qs == s
        assert mine.sum() >= 18
        assert (refs[s][1][mine, 0] >= 0).any(), "slot %d: none of its queries returns a label" % s
        passing_ids = b["ids"][fs.passing_rows(b, sets, s)]
        w = plain[mine]
        assert (~np.isin(w[w >= 0], passing_ids)).any(), "slot %d: every unfiltered winner of its queries passes" % s
        got = refs[s][1][mine, 0]
        assert np.isin(got[got >= 0], passing_ids).all()


def test_fixture_conditions_redo_case():
    """The overflow fixture: under the deny set the query still fills its k places, and its unfiltered nearest is denied."""
    b, q, qs, sets, (nprobe, max_codes, ef, k) = fs.redo_case(base)
    assert list(qs) == [31, fs.NONE, fs.UNSET]
    refs = fs.per_slot(fs.oracle_search((nprobe, max_codes, ef), k), b, sets, q, k, slots=qs)
    deny = sets[31][0]
    assert (refs[31][1][0] >= 0).all() and not np.isin(refs[31][1][0], deny).any()
    assert np.isin(refs[fs.NONE][1][1], deny).any()
    assert (refs[fs.UNSET][1] == -1).all()
