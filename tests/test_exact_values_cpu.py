"""tests/exact_values_ref.py (no GPU): the restatement of the exact _values calls is pinned to
exact_filter_ref run per distinct interval on that interval's queries, and the shared fixture is shown to hold what the GPU
tests rely on -- the descending tie block, a strip whose windows sit at the two ends of the value order, window edges in
the middle of a tile and on both sides of a split cut, a near-full window among narrow ones, single-row windows, absent
and inverted intervals, values on both sides of 2^31, 0, 0xfffffffe and valueless rows.  Also the new symbols in the
header, the library and the wrapper, and the host arithmetic under the sanitizers (tests/cpp/exact_values_tool.cpp)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import exact_filter_ref as fr
import exact_values_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ivfhnsw_gpu_set_base_values", "ivfhnsw_gpu_set_base_values_dev", "ivfhnsw_gpu_clear_base_values",
           "ivfhnsw_gpu_base_values_info", "ivfhnsw_gpu_base_value_rows", "ivfhnsw_gpu_exact_search_values",
           "ivfhnsw_gpu_exact_search_values_dev", "ivfhnsw_gpu_exact_range_search_values",
           "ivfhnsw_gpu_exact_range_search_values_dev")


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


def test_symbols_in_header_library_and_wrapper(pkg):
    header = open(os.path.join(ROOT, "include", "ivfhnsw_hip.h")).read()
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, header), s
        assert s in pkg.ABI_SYMBOLS, s
        assert getattr(raw, s) is not None
    assert pkg.VALUE_NONE == 0xffffffff == vr.NONE
    for m in ("set_base_values", "set_base_values_dev", "clear_base_values", "base_values_info", "base_value_rows",
              "exact_search_values", "exact_search_values_dev", "exact_range_search_values", "exact_range_search_values_dev"):
        assert callable(getattr(pkg.GpuIndex, m)), m
    src = open(os.path.join(ROOT, "ivf-hnsw_amd", "csrc", "capi_handle.cpp")).read()
    assert re.search(r"ivfhnsw_gpu_abi_version\s*\(\s*(void)?\s*\)\s*\{\s*return\s+9\s*;", src)


def test_exact_values_tool(tmp_path):
    exe = str(tmp_path / "exact_values_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "exact_values_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "exact_values ok" in r.stdout


@pytest.mark.parametrize("n,d,nq,assign", [(33, 16, 33, "each"), (33, 48, 20, "absent"), (601, 16, 40, "interleaved"), (601, 32, 97, "sizes"),
                                           (601, 16, 33, "gap")])
def test_restatement_is_exact_filter_ref_per_interval(n, d, nq, assign):
    base = vr.make_base(n, d)
    q = vr.make_queries(nq, d, base)
    bvals = vr.base_values(n)
    qr = vr.assignment(assign, n, nq)
    radius = np.float32(np.median(fr.search(base, q, min(10, n), np.ones(n, bool))[0][:, -1]))
    groups = {}
    for i, (lo, hi) in enumerate(qr.tolist()):
        groups.setdefault((lo, hi), []).append(i)

    def rows_of(lo, hi):  # the loop the one call replaces: the interval's rows as an allow set, in plain Python
        return np.array([r for r in range(n) if lo <= int(bvals[r]) <= hi], np.int64)

    for k in (1, 10, 100):
        want_d = np.full((nq, k), vr.FLT_MAX, np.float32)
        want_l = np.full((nq, k), -1, np.int64)
        for (lo, hi), idx in groups.items():
            want_d[idx], want_l[idx] = fr.search(base, q[idx], k, fr.pass_mask(n, rows_of(lo, hi)))
        _same(vr.search(base, q, k, bvals, qr), (want_d, want_l))
        _same(vr.search_blocked(base, q, k, bvals, qr), (want_d, want_l))
    for r in (np.float32(0), radius, np.float32(np.inf)):
        per_q = [None] * nq
        for (lo, hi), idx in groups.items():
            lims, dd, ll = fr.range_search(base, q[idx], r, fr.pass_mask(n, rows_of(lo, hi)))
            for j, qi in enumerate(idx):
                per_q[qi] = (dd[int(lims[j]):int(lims[j + 1])], ll[int(lims[j]):int(lims[j + 1])])
        lims = np.zeros(nq + 1, np.uint64)
        lims[1:] = np.cumsum([p[0].size for p in per_q], dtype=np.uint64)
        want = (lims, np.concatenate([p[0] for p in per_q]), np.concatenate([p[1] for p in per_q]))
        _same(vr.range_search(base, q, r, bvals, qr), want)
        _same(vr.range_blocked(base, q, r, bvals, qr), want)


def test_apply_sets_is_incremental():
    v = vr.apply_sets(10, [([1, 2, 3, 10, 99], [5, 5, 6, 7, 7]), ([2, 9], [vr.NONE, 8])])
    assert v.tolist() == [vr.NONE, 5, vr.NONE, 6] + [vr.NONE] * 5 + [8]


def test_windows_are_the_masks():
    for n in vr.NS:
        bvals = vr.base_values(n)
        order = vr.value_order(bvals)
        qr = np.array([(lo, hi) for lo in vr.EDGES for hi in vr.EDGES] + vr.pool(n).tolist(), np.uint32)
        for (a, b), (lo, hi) in zip(vr.windows(bvals, qr), qr):
            assert sorted(order[a:b].tolist()) == np.flatnonzero(vr.value_mask(bvals, lo, hi)).tolist(), (lo, hi)


@pytest.mark.parametrize("n", vr.NS)
def test_fixture_values(n):
    v = vr.base_values(n)
    assert v.dtype == np.uint32 and v.shape == (n,)
    # a band across 2^31, the value 0, 0xfffffffe, and rows without a value
    band = (v >= vr.BAND31) & (v < vr.BAND31 + 512)
    assert (v[band] < 0x80000000).any() and (v[band] >= 0x80000000).any()
    assert (v == 0).sum() > 1 and (v == 0xfffffffe).sum() > 1 and (v == vr.NONE).sum() > 1
    # intervals no row falls in
    assert not vr.value_mask(v, *vr.ABSENT).any() and vr.INVERTED[0] > vr.INVERTED[1]
    # the tie block: byte-identical rows whose values strictly descend with the row number, one row per value
    t0, tn = vr.tie_block(n)
    assert (np.diff(v[t0:t0 + tn].astype(np.int64)) < 0).all()
    assert (vr.value_mask(v, vr.TIE_TOP, vr.TIE_TOP + tn - 1) == ((np.arange(n) >= t0) & (np.arange(n) < t0 + tn))).all()
    for d in vr.DS:
        base = vr.make_base(n, d)
        assert (base[t0:t0 + tn] == base[t0]).all()
        assert (vr.make_queries(33, d, base)[vr.TIE_QUERY] == base[t0]).all()
    # in the holder's order the block is reversed: its highest row comes first
    order = vr.value_order(v)
    a, b = vr.windows(v, [(vr.TIE_TOP, vr.TIE_TOP + tn - 1)])[0]
    assert order[a:b].tolist() == list(range(t0 + tn - 1, t0 - 1, -1))


def test_fixture_tie_block_gap_and_edges():
    n = vr.BIG_N
    v = vr.base_values(n)
    t0, tn = vr.tie_block(n)
    # more tied rows than any compiled candidate buffer holds: under a strict '<' the first k to arrive, the HIGHEST rows, win
    assert tn >= 300 > 136
    # long runs of equal values
    cnt = {int(x): int(c) for x, c in zip(*np.unique(v, return_counts=True))}
    assert all(cnt[vr.RUN0 + i] > 64 for i in range(10))  # each more than two tiles of 32
    # the queries that equal the block search it, or an interval that holds it
    for a in vr.ASSIGNMENTS:
        qr = vr.assignment(a, n, 33)
        if a in ("one", "each", "wide", "single", "interleaved"):
            lo, hi = qr[vr.TIE_QUERY]
            assert lo <= vr.TIE_TOP and hi >= vr.TIE_TOP + tn - 1
    # the gap: one strip holds windows at both ends of the value order, and rows between them that no query of it counts
    dense, ws = vr.strips(v, vr.assignment("gap", n, 33))
    w = vr.windows(v, vr.assignment("gap", n, 33))
    assert dense == 0 and len(ws) == 2
    first = w[ws[0]]
    assert first[:, 0].min() == 0 and first[:, 1].max() > n - n // 5
    covered = np.zeros(n, bool)
    for a, b in first:
        covered[a:b] = True
    assert (~covered[:first[:, 1].max()]).sum() > n // 2
    # a near-full window among narrow ones in one strip
    qr = vr.assignment("wide", n, 33)
    w = vr.windows(v, qr)
    size = w[:, 1] - w[:, 0]
    assert (size > n * 8 // 10).sum() >= 1 and (size <= 200).sum() >= 30
    # single-row windows, and k larger than the window at k = 10 and k = 100
    w = vr.windows(v, vr.assignment("single", n, 300))
    assert (np.delete(w[:, 1] - w[:, 0], vr.TIE_QUERY) == 1).all()  # (the tie query searches the whole block)
    sizes = {int(b - a) for a, b in vr.windows(v, vr.pool(n))}
    assert any(0 < s < 10 for s in sizes) and any(10 <= s < 100 for s in sizes) and 0 in sizes and n in sizes
    # window edges: in the middle of a tile of 32, and windows that straddle the cuts of 3 splits of their strip's span
    w = vr.windows(v, vr.assignment("each", n, 300))
    assert (w[:, 0] % 32 != 0).any() and (w[:, 1] % 32 != 0).any()
    dense, ws = vr.strips(v, vr.assignment("interleaved", n, 300))
    w = vr.windows(v, vr.assignment("interleaved", n, 300))
    assert dense >= 1 and len(ws) >= 3
    straddles = 0
    for s in ws:
        A, B = w[s][:, 0].min(), w[s][:, 1].max()
        cps = ((B - A + 2) // 3 + 31) // 32 * 32
        for a, b in w[s]:
            straddles += any(a - A < c < b - A for c in (cps, 2 * cps))
    assert straddles >= 3
    # the strips of every assignment stay within the bound m / 32 + 2
    for a in vr.ASSIGNMENTS:
        for nq in vr.NQS:
            if vr.fits(a, n, nq):
                dense, ws = vr.strips(v, vr.assignment(a, n, nq))
                assert dense + len(ws) <= nq // 32 + 2


def test_grid_covers_every_axis():
    g = vr.grid()
    for i, vals in enumerate((vr.NS, vr.DS, vr.KS, vr.NQS, vr.ASSIGNMENTS, vr.SPLITS, vr.MAPS)):
        assert {c[i] for c in g} == set(vals)
    assert all(vr.fits(c[4], c[0], c[3]) for c in g)
