"""The base filter's host arithmetic in csrc/sweep_plan_math.h (no GPU): tests/cpp/exact_filter_tool.cpp, built with the
address and undefined-behaviour sanitizers, checks the rule that picks the form of a filtered sweep, the pass-word count,
the splits and tile-map words of the compact column space and the tile -> pass word map against literal restatements."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_filter_tool(tmp_path):
    exe = str(tmp_path / "exact_filter_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "exact_filter_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "exact_filter ok" in r.stdout
