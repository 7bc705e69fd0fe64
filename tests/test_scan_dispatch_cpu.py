"""csrc/scan_dispatch.h on the host (no GPU): tests/cpp/dispatch_tool.cpp, built with the address and
undefined-behaviour sanitizers, checks the constant by_code_size hands over for every code size 0..132, what the run-time
form accepts, and the arity with_mask calls with."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_tool(tmp_path):
    exe = str(tmp_path / "dispatch_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "dispatch_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scan_dispatch ok" in r.stdout
