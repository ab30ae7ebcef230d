#!/bin/bash
# Is the device code of this tree, instruction for instruction, that of another checkout?  Compiles every translation unit of
# poreseq_amd/csrc/Makefile's SRCS to gfx950 assembly (device side only, no GPU needed) in both trees with the Makefile's flags and
# compares the files, the per-build `__hip_cuid_<hash>` symbol apart.
# usage: tools/devasm_diff.sh <other checkout> [scratch dir]
set -u
here=$(cd "$(dirname "$0")/.." && pwd); other=$(cd "$1" && pwd); out=${2:-$(mktemp -d)}
mkdir -p "$out"
flags=$(make -s -C "$here/poreseq_amd/csrc" --eval='show: ; @echo $(CXXFLAGS)' show)
srcs=$(make -s -C "$here/poreseq_amd/csrc" --eval='show: ; @echo $(SRCS)' show)
rc=0
for f in $srcs; do
  for t in here other; do
    ( cd "${!t}/poreseq_amd/csrc" && hipcc $flags --cuda-device-only -S -x hip "$f" -o "$out/$t.$f.s" 2> "$out/$t.$f.err" ) || { echo "$f: does not compile in $t ($out/$t.$f.err)"; rc=1; }
    sed -E -i 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$out/$t.$f.s"
  done
  if cmp -s "$out/here.$f.s" "$out/other.$f.s"; then echo "$f identical"; else echo "$f DIFFERS"; rc=1; fi
done
exit $rc
