"""The upsert (ivfhnsw_gpu_upsert_ivf) on the host (no GPU): tests/cpp/upsert_math_tool.cpp, built here with
the address and undefined-behaviour sanitizers as a stand-alone program (as tests/test_update_math_cpu.py builds its tool),
emulates whole upserts with csrc/update_math.h -- the (source tile, list) segments of the fused compaction, the destinations
of kept rows and of batch rows -- at tiles of 8 and of 2048 rows and rows of 1, 3, 4 and 7 dwords against a serial
remove-then-append: empty lists, lists emptied and refilled, lists over several tiles, tiles over many lists, batches and
removals that touch disjoint lists.  Every element of the new arrays is written exactly once.  And the four entry points
are declared, exported and bound without a change of the ABI version."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ivfhnsw_gpu_upsert_ivf", "ivfhnsw_gpu_upsert_ivf_dev", "ivfhnsw_gpu_upsert", "ivfhnsw_gpu_upsert_dev")


def test_upsert_math_tool(tmp_path):
    exe = str(tmp_path / "upsert_math_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "upsert_math_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "upsert_math ok" in r.stdout


def test_names_in_header_and_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "ivfhnsw_hip.h")).read()
    declared = set(re.findall(r"^int (ivfhnsw_gpu_[a-z_0-9]+)\s*\(", hdr, re.M))
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.ABI_SYMBOLS, name
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    for method in ("upsert_ivf", "upsert_ivf_dev", "upsert", "upsert_dev"):
        assert callable(getattr(pkg.GpuIndex, method)), method


def test_abi_version_is_still_9(pkg):
    assert pkg.lib().ivfhnsw_gpu_abi_version() == 9
