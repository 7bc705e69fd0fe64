"""csrc/update_math.h on the host (no GPU): tests/cpp/update_math_tool.cpp, built here with the address and
undefined-behaviour sanitizers as a stand-alone program (as tests/test_plan_math_cpu.py builds its tool), checks what the
kernels that update the resident lists share -- the 16-byte group copy against a serial copy (every head offset, row
widths of 1 to 8 dwords, 0 to 40 rows, five hole patterns; every destination dword written exactly once, nothing outside
the range, the 16-byte load exactly where the four sources are a run; the same for bytes), an IVFADC append, a Grouping
append and a removal emulated tile by tile at tiles of 8 and of 2048 rows against the naive result, list_of_row over runs
of empty lists, and the workspace sizes against what the emulation touches."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_update_math_tool(tmp_path):
    exe = str(tmp_path / "update_math_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "update_math_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "update_math ok" in r.stdout
