"""csrc/walk_shape.h on the host (no GPU): tests/cpp/walk_shape_tool.cpp, built here with the address and
undefined-behaviour sanitizers as a stand-alone program (as tests/test_plan_math_cpu.py builds its tool), checks the rule by
which launch_coarse picks a shaped instantiation of the walk or the generic one -- for the shapes tests/test_gpu_walk_shape.py
walks on the device (d 128 and 96 with maxM 32 shaped; maxM 16 and d 64 generic), the knob, and the forms that have no shaped
instantiation."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_shape_tool(tmp_path):
    exe = str(tmp_path / "walk_shape_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "walk_shape_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "walk_shape ok" in r.stdout
