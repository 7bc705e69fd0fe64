#!/bin/bash
# What the compiler made of every instantiation of the throughput walk: compiles kernels_hnsw.hip device-only with the
# Makefile's flags and prints, per hnsw_walk_kernel instantiation, the resource fields of the code object's own metadata
# (registers, spills, scratch) and the code length from the symbol table.  Needs no GPU.
#   bash tools/walk_resources.sh [csrc directory, default this tree's]
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=${1:-$ROOT/ivf-hnsw_amd/csrc}
ROCM=${ROCM_PATH:-/opt/rocm}
HIPCC=${HIPCC:-$ROCM/bin/hipcc}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
# WALK_CO: a code object compiled earlier (skips the compile)
FLAGS=$(make -s -C "$ROOT/ivf-hnsw_amd/csrc" -pn 2>/dev/null | sed -n 's/^CXXFLAGS = //p' | head -1)
[ -n "$WALK_CO" ] && cp "$WALK_CO" "$T/walk.co" ||
"$HIPCC" $FLAGS --offload-arch=gfx950 --cuda-device-only --no-gpu-bundle-output -c "$SRC/kernels_hnsw.hip" -I"$SRC" -o "$T/walk.co"
"$ROCM/llvm/bin/llvm-readelf" --notes "$T/walk.co" > "$T/notes.txt"
"$ROCM/llvm/bin/llvm-readelf" -sW "$T/walk.co" > "$T/syms.txt"
python3 - "$T/notes.txt" "$T/syms.txt" <<'PY'
import re, subprocess, sys
notes, syms = open(sys.argv[1]).read(), open(sys.argv[2]).read()
size = {}
for line in syms.splitlines():
    f = line.split()
    if len(f) >= 8 and f[3] == "FUNC":
        size[f[7]] = int(f[2], 0)
want = (".private_segment_fixed_size", ".sgpr_count", ".sgpr_spill_count", ".vgpr_count", ".vgpr_spill_count")
rows = []
for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
    m = re.search(r"\.symbol:\s+(\S+)\.kd", blk)
    if not m or "hnsw_walk_kernel" not in m.group(1):
        continue
    sym = m.group(1)
    v = {k: int(re.search(re.escape(k) + r":\s+(\d+)", blk).group(1)) for k in want}
    name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"^void ivfhnsw_gpu_impl::|\(.*$", "", name)
    rows.append((name, v, size.get(sym, 0)))
print("%-64s %7s %5s %10s %5s %10s %8s" % ("instantiation <NCH, MINW, TAGW, FMODE, STAMPS, SPILL, D, MAXM, MERGE>", "scratch",
                                           "sgpr", "sgpr_spill", "vgpr", "vgpr_spill", "code B"))
for name, v, sz in sorted(rows):
    print("%-64s %7d %5d %10d %5d %10d %8d" % (name, v[want[0]], v[want[1]], v[want[2]], v[want[3]], v[want[4]], sz))
PY
