"""Every branch of the scan launchers' dispatch (csrc/scan_dispatch.h): code size x layout x filter x entry point.

The other suites sample this matrix -- code size 4 meets no filter, top-k, heap scan or range search there, and the bitmap
forms meet code size 16 only -- so a wrong constant in one branch of by_code_size / with_mask would pass them.  Every cell
compares labels and distance bits with the oracle (range search: with range_ref), the scored codes with the oracle's
ncode, and last_scan_kernel with NAMES.

Expected values of the filtered cells come from filter_ref's poisoned corpus, as in test_gpu_filter.  NAMES holds, cell by
cell, what the library reported for this matrix before the launchers were rewritten on scan_dispatch.h."""
import numpy as np
import pytest

from conftest import corpus
import filter_ref
import range_ref
import synth
from test_gpu_remove import _upload
from test_gpu_filter import same_bits, tiled

pytestmark = pytest.mark.gpu

CODE_SIZES = (4, 8, 16, 32, 12)  # dsub 24, 12, 6, 3, 8; 12 has no kernel of its own: the run-time form
NPROBE, MAX_CODES, EF = 16, 2000, 64
BIG = dict(nprobe=64, max_codes=10 ** 9, ef=80)  # k = 1100: every list, every code
ENTRIES = ("k1_split", "k1_whole", "k10", "k10_heap", "k1100_heap", "range")

# (code size, layout, filter) -> last_scan_kernel after each of ENTRIES, in that order
NAMES = {
    (4, "ivf", False): ("scan_k1_kernel", "scan_k1_kernel", "scan_topk_kernel", "scan_topk_kernel", "heap_scan_kernel",
                        "range_scan_kernel"),
    (4, "ivf", True): ("scan_k1_kernel+filter", "scan_k1_kernel+filter", "scan_topk_kernel+filter",
                       "scan_topk_kernel+filter", "heap_scan_kernel+filter", "range_scan_kernel+filter"),
    (4, "grouping", False): ("scan_k1_bitmap_kernel", "scan_k1_bitmap_kernel", "scan_topk_kernel", "scan_topk_kernel",
                             "heap_scan_kernel", "range_scan_bitmap_kernel"),
    (4, "grouping", True): ("scan_k1_bitmap_kernel+filter", "scan_k1_bitmap_kernel+filter", "scan_topk_kernel+filter",
                            "scan_topk_kernel+filter", "heap_scan_kernel+filter", "range_scan_bitmap_kernel+filter"),
    (8, "ivf", False): ("scan_k1_kernel", "scan_k1_kernel", "scan_topk_kernel", "scan_topk_kernel", "heap_scan_kernel",
                        "range_scan_kernel"),
    (8, "ivf", True): ("scan_k1_kernel+filter", "scan_k1_kernel+filter", "scan_topk_kernel+filter",
                       "scan_topk_kernel+filter", "heap_scan_kernel+filter", "range_scan_kernel+filter"),
    (8, "grouping", False): ("scan_k1_bitmap_kernel", "scan_k1_bitmap_kernel", "scan_topk_kernel", "scan_topk_kernel",
                             "heap_scan_kernel", "range_scan_bitmap_kernel"),
    (8, "grouping", True): ("scan_k1_bitmap_kernel+filter", "scan_k1_bitmap_kernel+filter", "scan_topk_kernel+filter",
                            "scan_topk_kernel+filter", "heap_scan_kernel+filter", "range_scan_bitmap_kernel+filter"),
    (16, "ivf", False): ("scan_k1_kernel", "scan_k1_kernel", "scan_topk_kernel", "scan_topk_kernel", "heap_scan_kernel",
                         "range_scan_kernel"),
    (16, "ivf", True): ("scan_k1_kernel+filter", "scan_k1_kernel+filter", "scan_topk_kernel+filter",
                        "scan_topk_kernel+filter", "heap_scan_kernel+filter", "range_scan_kernel+filter"),
    (16, "grouping", False): ("scan_k1_bitmap_kernel", "scan_k1_bitmap_kernel", "scan_topk_kernel", "scan_topk_kernel",
                              "heap_scan_kernel", "range_scan_bitmap_kernel"),
    (16, "grouping", True): ("scan_k1_bitmap_kernel+filter", "scan_k1_bitmap_kernel+filter", "scan_topk_kernel+filter",
                             "scan_topk_kernel+filter", "heap_scan_kernel+filter", "range_scan_bitmap_kernel+filter"),
    (32, "ivf", False): ("scan_k1_kernel", "scan_k1_kernel", "scan_topk_kernel", "scan_topk_kernel", "heap_scan_kernel",
                         "range_scan_kernel"),
    (32, "ivf", True): ("scan_k1_kernel+filter", "scan_k1_kernel+filter", "scan_topk_kernel+filter",
                        "scan_topk_kernel+filter", "heap_scan_kernel+filter", "range_scan_kernel+filter"),
    (32, "grouping", False): ("scan_k1_bitmap_kernel", "scan_k1_bitmap_kernel", "scan_topk_kernel", "scan_topk_kernel",
                              "heap_scan_kernel", "range_scan_bitmap_kernel"),
    (32, "grouping", True): ("scan_k1_bitmap_kernel+filter", "scan_k1_bitmap_kernel+filter", "scan_topk_kernel+filter",
                             "scan_topk_kernel+filter", "heap_scan_kernel+filter", "range_scan_bitmap_kernel+filter"),
    (12, "ivf", False): ("scan_k1_kernel (run-time code size)", "scan_k1_kernel (run-time code size)", "scan_topk_kernel",
                         "scan_topk_kernel", "heap_scan_kernel", "range_scan_kernel (run-time code size)"),
    (12, "ivf", True): ("scan_k1_kernel (run-time code size)+filter", "scan_k1_kernel (run-time code size)+filter",
                        "scan_topk_kernel+filter", "scan_topk_kernel+filter", "heap_scan_kernel+filter",
                        "range_scan_kernel (run-time code size)+filter"),
    (12, "grouping", False): ("scan_k1_kernel (run-time code size)", "scan_k1_kernel (run-time code size)",
                              "scan_topk_kernel", "scan_topk_kernel", "heap_scan_kernel",
                              "range_scan_kernel (run-time code size)"),
    (12, "grouping", True): ("scan_k1_kernel (run-time code size)+filter", "scan_k1_kernel (run-time code size)+filter",
                             "scan_topk_kernel+filter", "scan_topk_kernel+filter", "heap_scan_kernel+filter",
                             "range_scan_kernel (run-time code size)+filter"),
}


def shape(M, layout):
    kw = dict(nc=64, d=96, M=M, n_base=6000, nq=32, efConstruction=60)
    if layout == "grouping":
        kw.update(nc=128, nsubc=8)  # the mean sub-group holds 5.9 codes: the short-segment forms
    return kw


@pytest.fixture(scope="module")
def cells(pkg):
    """cell(M, layout, filt): one handle per (code size, layout, filter) and the corpus `e` whose unfiltered search is
    what it must return; built on first use, handles closed when the module is done."""
    made = {}

    def cell(M, layout, filt):
        key = (M, layout, filt)
        if key not in made:
            b = filter_ref.clipped(corpus(**shape(M, layout)))
            g = _upload(pkg.GpuIndex(0), b)
            made[key] = c = dict(b=b, e=b, g=g, allow=None, refs={}, key=key)
            if filt:
                c["allow"] = np.random.default_rng(M).choice(b["ids"], len(b["ids"]) // 2, replace=False).astype(np.uint32)
                g.set_filter(c["allow"])
                c["e"] = filter_ref.poisoned(b, filter_ref.passing(b["ids"], c["allow"]))
        return made[key]

    yield cell
    for c in made.values():
        c["g"].close()


def oracle(c, k, nprobe=NPROBE, max_codes=MAX_CODES, ef=EF):
    """(distances, labels, coarse ids, coarse distances, stats) of the oracle's search of c["e"], once per cell."""
    key = (k, nprobe, max_codes, ef)
    if key not in c["refs"]:
        ox = synth.oracle_index(c["e"])
        ox.set_params(nprobe, max_codes, ef)
        c["refs"][key] = ox.search_batch(c["b"]["queries"], k=k)
    return c["refs"][key]


def scored(c, which):
    return range_ref.scored_batch(c[which], c["b"]["queries"], NPROBE, MAX_CODES, EF,
                                  key=("scan_dispatch", c["key"][:2], which if c["allow"] is not None else "b"))


def run(c, entry):
    """-> the scored codes the oracle expects; asserts the cell's results."""
    g, q = c["g"], c["b"]["queries"]
    if entry in ("k1_split", "k1_whole"):
        # 32 queries: 32 workgroups per query meet in the atomic; 1024: one per query, and the scan writes the label itself
        rep = 1 if entry == "k1_split" else 32
        ref = oracle(c, 1)
        got = g.search(tiled(q, len(q) * rep), 1, NPROBE, MAX_CODES, efSearch=EF)
        assert same_bits(got, np.tile(ref[0], (rep, 1)), np.tile(ref[1], (rep, 1)))
        return ref[4].ncode * rep
    if entry == "k10":
        ref = oracle(c, 10)
        got = g.search(q, 10, NPROBE, MAX_CODES, efSearch=EF)
        # ascending by (distance, scan position): the oracle's heap array sorted; rows without a tie label for label
        assert np.array_equal(got[0].view(np.uint32), np.sort(ref[0], axis=1).view(np.uint32))
        for i in range(len(q)):
            assert sorted(got[1][i]) == sorted(ref[1][i]), i
            if len(np.unique(ref[0][i])) == 10:
                assert np.array_equal(got[1][i], ref[1][i][np.argsort(ref[0][i], kind="stable")]), i
        return ref[4].ncode
    if entry == "k10_heap":
        ref = oracle(c, 10)
        assert same_bits(g.search(q, 10, NPROBE, MAX_CODES, efSearch=EF, heap_order=True), ref[0], ref[1])
        return ref[4].ncode
    if entry == "k1100_heap":
        ref = oracle(c, 1100, **BIG)
        got = g.search(q, 1100, BIG["nprobe"], BIG["max_codes"], efSearch=BIG["ef"], heap_order=True)
        assert same_bits(got, ref[0], ref[1])
        assert ((ref[1] >= 0).sum(1) == 1100).any(), "fixture: some query must admit more than k codes"
        return ref[4].ncode
    assert entry == "range"
    d10, l10 = oracle(c, 10)[:2]
    r = np.float32(np.median(d10[l10 >= 0]))
    lims, dist, lab = got = g.range_search(q, r, NPROBE, MAX_CODES, efSearch=EF)
    sc_b, sc_e = scored(c, "b"), scored(c, "e")
    assert lims[0] == 0 and lims[-1] == len(dist) == len(lab) and 0 < len(lab) < sc_e["ncode"].sum()
    for i in range(len(q)):  # the scored set below the radius, labels with distance bits
        assert np.array_equal(range_ref.result_set(lims, dist, lab, i), range_ref.expected_set(sc_e, i, r)), i
    if c["key"][1] == "ivf":  # ... and in scan order, which range_ref restates for IVFADC
        want = range_ref.expected_ivf(c["b"], sc_b, MAX_CODES, r)
        assert range_ref.same_range(got, want if c["allow"] is None else range_ref.filtered(want, c["allow"]))
    assert np.array_equal(sc_b["ncode"], sc_e["ncode"])
    return int(sc_e["ncode"].sum())


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("filt", [False, True], ids=["plain", "filter"])
@pytest.mark.parametrize("layout", ["ivf", "grouping"])
@pytest.mark.parametrize("M", CODE_SIZES, ids=lambda M: "M%d" % M)
def test_cell(cells, M, layout, filt, entry):
    c = cells(M, layout, filt)
    ncode = run(c, entry)
    assert c["g"].last_scan_counts()[0] == ncode
    assert c["g"].last_scan_kernel() == NAMES[M, layout, filt][ENTRIES.index(entry)]
