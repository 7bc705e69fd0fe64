"""csrc/plan_math.h on the host (no GPU): tests/cpp/plan_math_tool.cpp, built here with the address and
undefined-behaviour sanitizers as a stand-alone program (as tests/test_sweep_plan_cpu.py builds its tool), checks what the
kernels that build a scan plan share -- the three max_codes rules as functions of prefix sums against plain serial loops
(empty lists, max_codes 0 and 1, sums beyond 2^32), the layout of plan_grouping4_kernel's dynamic LDS against the
launcher's formula and the kernel's carving it replaced (no two arrays overlap), and the range of the hash of the
neighbour-centroid set."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_math_tool(tmp_path):
    exe = str(tmp_path / "plan_math_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "plan_math_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan_math ok" in r.stdout
