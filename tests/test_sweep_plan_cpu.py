"""csrc/sweep_plan_math.h on the host (no GPU): tests/cpp/sweep_plan_tool.cpp, built with the address and
undefined-behaviour sanitizers, checks the arithmetic the brute-force MFMA sweeps share -- columns per split, split
count, the range search's tile-map words and the dispatch on a row's length -- against literal restatements of the
formulas of the three launchers it replaced."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_plan_tool(tmp_path):
    exe = str(tmp_path / "sweep_plan_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "sweep_plan_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sweep_plan ok" in r.stdout
