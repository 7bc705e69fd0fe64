"""Tag AND interval on the float16 store without a GPU: the two entries are declared, listed and exported."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["exact_search_f16_tags_values", "exact_search_f16_tags_values_dev"])
def test_symbol_declared_listed_and_exported(pkg, name):
    header = open(os.path.join(ROOT, "include", "ivfhnsw_hip.h")).read()
    # the argument order is the siblings': the tags where _tags has them, the ranges behind them
    assert re.search(r"\bint ivfhnsw_gpu_%s\s*\([^)]*size_t k,\s*const uint16_t \*\w+,\s*const uint32_t \*\w+,\s*float \*" % name, header)
    assert "ivfhnsw_gpu_" + name in pkg.ABI_SYMBOLS
    getattr(pkg.lib(), "ivfhnsw_gpu_" + name)
    assert callable(getattr(pkg.GpuIndex, name))
