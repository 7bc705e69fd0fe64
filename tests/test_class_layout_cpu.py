"""The classes' object layout is part of the drop-in surface: a driver compiled against these headers allocates
IndexIVF_HNSW / IndexIVF_HNSW_Grouping with ITS idea of their size and hands the object to libivfhnsw.so.  A library
whose classes grew data members writes past such an allocation (a driver built before the change aborts in malloc).
So extensions add member functions only, and the sizes stay those the classes have had (x86-64, g++, LP64)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_class_sizes_are_unchanged(tmp_path):
    src = tmp_path / "sz.cpp"
    src.write_text('#include <ivf-hnsw/IndexIVF_HNSW_Grouping.h>\n#include <cstdio>\n'
                   'int main() { printf("%zu %zu\\n", sizeof(ivfhnsw::IndexIVF_HNSW), '
                   'sizeof(ivfhnsw::IndexIVF_HNSW_Grouping)); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.run(["g++", "-std=c++11", "-w", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [440, 576]
