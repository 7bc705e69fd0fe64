"""csrc/walk_form.h on the host (no GPU): tests/cpp/walk_form_tool.cpp, built here with the address and
undefined-behaviour sanitizers as a stand-alone program (as tests/test_plan_math_cpu.py builds its tool), checks the rule by
which launch_coarse picks the instantiation of the walk -- result-set class, visited-set tag width and buckets, filter form,
shape (for the shapes tests/test_gpu_walk_shape.py walks on the device: d 128 and 96 with maxM 32 shaped; maxM 16 and d 64
generic), the stamps build, the dynamic LDS of the bench's graphs -- and that the dispatcher has an instantiation for every
form the rule produces, with the form's own values, and none for a form that cannot occur."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_form_tool(tmp_path):
    exe = str(tmp_path / "walk_form_tool")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "ivf-hnsw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "walk_form_tool.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "walk_form ok" in r.stdout
