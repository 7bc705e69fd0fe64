"""csrc/walk_bound.h on the host (no GPU): tests/cpp/walk_bound_tool.cpp, built here with the address and
undefined-behaviour sanitizers as a stand-alone program (as tests/test_walk_form_cpu.py builds its tool), checks on more
than 10^7 (query, row) pairs -- random, byte-exact, outlier and near-duplicate tables at d 16, 96 and 128, queries on rows,
a few ulps off them and far outside the byte range on both sides -- that the walk filter's lower bound, with both square
roots one ulp high, never exceeds the float distance in the reference's summation order; that a row's 9-bit error code
never under-states its error (zero and the table-wide maximum included) and that the 23-bit norm beside it survives
128 * 255^2."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_bound_tool(tmp_path):
    exe = str(tmp_path / "walk_bound_tool")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "walk_bound_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "walk_bound ok" in r.stdout
