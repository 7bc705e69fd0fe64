"""csrc/tag_value_math.h on the host (no GPU): tests/cpp/tag_value_math_tool.cpp, built here with the address and
undefined-behaviour sanitizers as a stand-alone program (as tests/test_value_math_cpu.py builds its tool), runs the fill and
the pass predicate of "tag AND value"  -- what filter_mask and filter_pass<5> compute on the device --
against the plain rule (t == 0xffff || tag == t) && lo <= v <= hi written with 64-bit integers, over the cross product of
value_math_tool.cpp's boundary values for v, lo and hi, row tags and query tags {0, 255, 256, 0xfffe, 0xffff}, with and
without each row array: 2 * 2 * 5 * 11 * 11 * 5 * 11 = 133 100 cases."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tag_value_math_tool(tmp_path):
    exe = str(tmp_path / "tag_value_math_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "tag_value_math_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tag_value_math ok (133100 cases)" in r.stdout
