"""csrc/scan_plan_math.h on the host (no GPU): tests/cpp/scan_steps_tool.cpp, built with the address and
undefined-behaviour sanitizers, checks the index arithmetic the ADC scan kernels share -- a query's slices, the three
segment seeks, the bitmap form's chunks and its segment lookup -- on seeded random plans against a linear reference."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_steps_tool(tmp_path):
    exe = str(tmp_path / "scan_steps_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "scan_steps_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scan_steps ok" in r.stdout
