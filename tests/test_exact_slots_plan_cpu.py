"""The host arithmetic of the base filter slots in csrc/sweep_plan_math.h (no GPU): tests/cpp/exact_slots_tool.cpp, built
with the address and undefined-behaviour sanitizers, checks the strip bound, the strip layout from the 34 counts (strips
slot-uniform, every query in exactly one row, the forms in contiguous ranges) and the per-strip split cut."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_slots_tool(tmp_path):
    exe = str(tmp_path / "exact_slots_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "exact_slots_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "exact_slots ok" in r.stdout
