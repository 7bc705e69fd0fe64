"""The label filter's surface (no GPU): the symbols are declared and exported, and the method the GPU tests take their
expected values from -- the oracle on a poisoned corpus (filter_ref) -- does what DESIGN.md 3.14 says it does."""
import os
import re

import numpy as np
import pytest

from conftest import corpus
import filter_ref
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ivfhnsw_gpu_set_filter", "ivfhnsw_gpu_set_filter_dev", "ivfhnsw_gpu_clear_filter", "ivfhnsw_gpu_filter_info")
FLT_MAX = np.finfo(np.float32).max


def test_symbols_declared_and_listed(pkg):
    header = open(os.path.join(ROOT, "include", "ivfhnsw_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, header), s
        assert s in pkg.ABI_SYMBOLS, s
    assert re.search(r"#define\s+IVFHNSW_FILTER_ALLOW\s+0", header) and re.search(r"#define\s+IVFHNSW_FILTER_DENY\s+1", header)
    assert (pkg.FILTER_ALLOW, pkg.FILTER_DENY) == (0, 1)
    for m in ("set_filter", "set_filter_dev", "clear_filter", "filter_info"):
        assert callable(getattr(pkg.GpuIndex, m))


CASES = [dict(seed=11, nc=256, d=128, M=16, n_base=30000, nq=64),
         dict(seed=43, nc=256, d=96, M=16, n_base=20000, nq=64, nsubc=8)]


@pytest.mark.parametrize("kw", CASES, ids=["ivfadc", "grouping"])
def test_poisoned_corpus_is_a_filtered_search(kw):
    """On p the oracle visits what it visits on b (equal ncode), returns passing labels only and FLT_MAX / -1 in unfilled
    slots; with nothing passing every query is empty; with everything passing p is b."""
    c = corpus(**kw)
    b = filter_ref.clipped(c)
    rng = np.random.default_rng(5)
    grp = bool(kw.get("nsubc"))
    ef = 64 if grp else 40
    short = empty = full = 0
    for pruning in ((False, True) if grp else (False,)):
        ob = synth.oracle_index(b)
        ob.set_params(16, 2000, ef, do_pruning=pruning)
        for frac in (1.0, 0.5, 0.1, 0.01, 0.0):
            allow = rng.choice(b["ids"], int(frac * len(b["ids"])), replace=False)
            rows = filter_ref.passing(b["ids"], allow)
            op = synth.oracle_index(filter_ref.poisoned(b, rows))
            op.set_params(16, 2000, ef, do_pruning=pruning)
            for k in (1, 10):
                rb = ob.search_batch(b["queries"], k=k)
                rp = op.search_batch(b["queries"], k=k)
                assert rp[4].ncode == rb[4].ncode
                lab, dist = rp[1], rp[0]
                assert np.isin(lab[lab >= 0], allow).all()
                assert (dist[lab < 0] == FLT_MAX).all() and np.isfinite(dist[lab >= 0]).all()
                if frac == 1.0:
                    assert np.array_equal(lab, rb[1]) and np.array_equal(dist.view(np.uint32), rb[0].view(np.uint32))
                if frac == 0.0:
                    assert (lab == -1).all()
                filled = (lab >= 0).sum(1)
                full += int((filled == k).sum())
                short += int(((filled > 0) & (filled < k)).sum())
                empty += int((filled == 0).sum())
    assert full and short and empty, (full, short, empty)
