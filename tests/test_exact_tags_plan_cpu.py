"""The host arithmetic of the base tags in csrc/sweep_plan_math.h (no GPU): tests/cpp/exact_tags_tool.cpp, built with the
address and undefined-behaviour sanitizers, checks the strip bound against brute-force counts over random histograms, the
chunk rule of the k-search (within the partial tables' bytes, never below 128, a multiple of 128, the largest such), the
plan's layout restated on the host and the per-strip split cut."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_tags_tool(tmp_path):
    exe = str(tmp_path / "exact_tags_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "exact_tags_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "exact_tags ok" in r.stdout
