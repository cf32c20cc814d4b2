#!/bin/bash
# Is the device code of two builds the same?  For every object file of the second build directory (pykg2vec_amd/csrc/build of a
# checkout) the gfx950 code object is taken out of its fat binary, disassembled, and compared with the same file of the first
# directory: instruction text and the kernel metadata notes (registers, LDS, arguments).  Host-only changes must print
# "identical" for every file that has device code.
#   usage: tools/device_code_diff.sh <build dir A> <build dir B>        (exit status 1 when a file differs)
B=${ROCM_LLVM_BIN:-/opt/rocm/lib/llvm/bin}
T=$(mktemp -d)
rc=0
for o in "$2"/*.o; do
  f=$(basename "$o" .o)
  n=0
  for side in "$1" "$2"; do
    n=$((n+1))
    [ -f "$side/$f.o" ] || { echo "$f: not in $side"; continue 2; }
    $B/llvm-objcopy --dump-section=.hip_fatbin=$T/$f.$n.fatbin "$side/$f.o" $T/scrap.o 2>/dev/null || { echo "$f: no device code"; continue 2; }
    $B/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$T/$f.$n.fatbin --output=$T/$f.$n.co || exit 2
    $B/llvm-objdump -d --no-show-raw-insn $T/$f.$n.co | grep -v "file format" > $T/$f.$n.s
    $B/llvm-readelf --notes $T/$f.$n.co | grep -v "^File:" > $T/$f.$n.notes
  done
  if cmp -s $T/$f.1.s $T/$f.2.s && cmp -s $T/$f.1.notes $T/$f.2.notes; then
    echo "$f: identical ($(wc -l < $T/$f.2.s) lines)"
  else
    echo "$f: DIFFERS"; rc=1
  fi
done
rm -rf $T
exit $rc
