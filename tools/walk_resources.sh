#!/bin/bash
# What the compiler made of every kernel of the throughput walk's file: compiles kernels_hnsw.hip device-only with the
# Makefile's flags and prints, per kernel (every hnsw_walk_kernel instantiation among them), the resource fields of the
# code object's own metadata (registers, spills, scratch), the code length from the symbol table and a SHA-256 of the
# code bytes -- the symbol's range in .text, as llvm-readelf -sW gives it.  Two trees whose rows agree run the same
# device code (profiles/r13_walk_form.md).  Needs no GPU.
#   bash tools/walk_resources.sh [csrc directory, default this tree's] [source file, default kernels_hnsw.hip]
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=${1:-$ROOT/ivf-hnsw_amd/csrc}
FILE=${2:-kernels_hnsw.hip}
ROCM=${ROCM_PATH:-/opt/rocm}
HIPCC=${HIPCC:-$ROCM/bin/hipcc}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
# WALK_CO: a code object compiled earlier (skips the compile)
FLAGS=$(make -s -C "$ROOT/ivf-hnsw_amd/csrc" -pn 2>/dev/null | sed -n 's/^CXXFLAGS = //p' | head -1)
[ -n "$WALK_CO" ] && cp "$WALK_CO" "$T/walk.co" ||
"$HIPCC" $FLAGS --offload-arch=gfx950 --cuda-device-only --no-gpu-bundle-output -c "$SRC/$FILE" -I"$SRC" -o "$T/walk.co"
"$ROCM/llvm/bin/llvm-readelf" --notes "$T/walk.co" > "$T/notes.txt"
"$ROCM/llvm/bin/llvm-readelf" -sW "$T/walk.co" > "$T/syms.txt"
"$ROCM/llvm/bin/llvm-readelf" -SW "$T/walk.co" > "$T/sections.txt"
"$ROCM/llvm/bin/llvm-objcopy" -O binary --only-section=.text "$T/walk.co" "$T/text.bin"
python3 - "$T/notes.txt" "$T/syms.txt" "$T/sections.txt" "$T/text.bin" <<'PY'
import hashlib, re, subprocess, sys
notes, syms, sections = (open(a).read() for a in sys.argv[1:4])
text = open(sys.argv[4], "rb").read()
text_addr = int(re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)", sections).group(1), 16)
span = {}
for line in syms.splitlines():
    f = line.split()
    if len(f) >= 8 and f[3] == "FUNC":
        span[f[7]] = (int(f[1], 16) - text_addr, int(f[2], 0))
want = (".private_segment_fixed_size", ".sgpr_count", ".sgpr_spill_count", ".vgpr_count", ".vgpr_spill_count")
rows = []
for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
    m = re.search(r"\.symbol:\s+(\S+)\.kd", blk)
    if not m:
        continue
    sym = m.group(1)
    v = {k: int(re.search(re.escape(k) + r":\s+(\d+)", blk).group(1)) for k in want}
    name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"^void ivfhnsw_gpu_impl::|\(.*$", "", name.replace("(anonymous namespace)::", ""))
    off, sz = span.get(sym, (0, 0))
    assert 0 <= off and off + sz <= len(text), sym
    rows.append((name, v, sz, hashlib.sha256(text[off:off + sz]).hexdigest()))
print("%-64s %7s %5s %10s %5s %10s %8s  %s" % ("kernel (hnsw_walk_kernel<NCH, TAGW, FMODE, STAMPS, SPILL, D, MAXM, MERGE>)", "scratch",
                                               "sgpr", "sgpr_spill", "vgpr", "vgpr_spill", "code B", "sha256 of the code bytes"))
for name, v, sz, h in sorted(rows):
    print("%-64s %7d %5d %10d %5d %10d %8d  %s" % (name, v[want[0]], v[want[1]], v[want[2]], v[want[3]], v[want[4]], sz, h))
PY
