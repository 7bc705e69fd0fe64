"""csrc/value_math.h on the host (no GPU): tests/cpp/value_math_tool.cpp, built here with the address and
undefined-behaviour sanitizers as a stand-alone program (as tests/test_walk_form_cpu.py builds its tool), runs the fill and
the pass predicate of the row values -- what filter_mask and filter_pass<4> compute on the device --
against the plain rule lo <= v <= hi over the cross product of {0, 1, 76, 77, 78, 0xffff, 0x10000, 0x7fffffff, 0x80000000,
0xfffffffe, 0xffffffff} for v, lo and hi, inverted intervals included, with and without a table."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_value_math_tool(tmp_path):
    exe = str(tmp_path / "value_math_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "value_math_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "value_math ok (2662 cases)" in r.stdout
