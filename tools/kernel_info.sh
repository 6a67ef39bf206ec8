#!/bin/bash
# VGPR / scratch / LDS / code size of every kernel of one source file (compiles it for gfx950 with
# the Makefile's flags and prints the compiler's resource remarks).
#   tools/kernel_info.sh finenv_cashpenalty.hip [extra -D flags]
# ISA digests, for diffing the device code of two trees (one line per kernel: hash, symbol):
#   tools/kernel_info.sh --isa finenv_stock_np32.hip [extra -D flags]
#   tools/kernel_info.sh --isa <other tree>/finrl_amd/csrc/finenv_stock_np32.hip
set -e
isa=0
if [ "$1" = "--isa" ]; then isa=1; shift; fi
src=$1; shift
case "$src" in
  */*) cd "$(dirname "$src")"; src=$(basename "$src") ;;
  *) cd "$(dirname "$0")/../finrl_amd/csrc" ;;
esac
if [ $isa = 1 ]; then
  # gfx950 assembly of the device side; per kernel, hash its code (label .. .Lfunc_end) and its
  # .amdhsa_kernel descriptor block (registers, LDS, scratch, launch bounds).  The per-build
  # __hip_cuid_<hash> symbol and the function index inside local labels are masked and the comments
  # dropped, so a kernel keeps its digest when another one joins or leaves the file.
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. "$@" \
      --cuda-device-only -S -o - "$src" |
    python3 -c '
import sys, re, hashlib
t = sys.stdin.read()
t = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", t)
t = re.sub(r"[ \t]*;.*$", "", t, flags=re.M)      # comments name blocks by function index, at a column that moves with it
t = re.sub(r"\.LBB\d+_", ".LBB_", t)
t = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", t)
for m in sorted(re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n.*?\.end_amdhsa_kernel", t, re.M | re.S), key=lambda m: m.group(1)):
    k = m.group(1)
    code = re.search(r"^%s:.*?^\.Lfunc_end:" % re.escape(k), t, re.M | re.S).group(0)
    print(hashlib.sha256((code + m.group(0)).encode()).hexdigest()[:16], k)
'
  exit 0
fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. "$@" \
    -c -o /dev/null "$src" -Rpass-analysis=kernel-resource-usage 2>&1 |
  python3 -c '
import sys, re
name = None; d = {}
for ln in sys.stdin:
    m = re.search(r"remark:\s*(.*?)\s*\[-Rpass", ln)
    if not m: continue
    t = m.group(1).strip()
    if t.startswith("Function Name:"):
        name = t.split(":", 1)[1].strip(); d = {}
    for k, lab in (("VGPRs:", "vgpr"), ("AGPRs:", "agpr"), ("ScratchSize [bytes/lane]:", "scratch"),
                   ("LDS Size [bytes/block]:", "lds"), ("Occupancy [waves/SIMD]:", "occ"),
                   ("SGPRs Spill:", "sspill")):
        if t.startswith(k): d[lab] = t.split(":", 1)[1].strip()
    if t.startswith("LDS Size") and name:
        print("%-84s vgpr %3s agpr %3s scratch %4s sgpr-spill %3s lds %6s occ %s" % (name[:84], d.get("vgpr"), d.get("agpr"), d.get("scratch"), d.get("sspill"), d.get("lds"), d.get("occ")))
'
# code sizes (bytes) of the same kernels: compile to an object, unbundle the gfx950 code object
tmp=$(mktemp -d); trap 'rm -rf $tmp' EXIT
B=/opt/rocm/lib/llvm/bin
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -I. "$@" \
    -c -o $tmp/x.o "$src" >/dev/null 2>&1
$B/llvm-objcopy --dump-section .hip_fatbin=$tmp/fb.bin $tmp/x.o
$B/clang-offload-bundler --unbundle --type=o --input=$tmp/fb.bin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$tmp/co.elf
$B/llvm-readelf -s $tmp/co.elf | awk '$4=="FUNC" && !seen[$8]++ {printf "  code %6d B  %s\n", $3, substr($8,1,100)}'
