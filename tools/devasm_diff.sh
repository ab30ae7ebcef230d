#!/bin/bash
# Is the device code of this tree, instruction for instruction, that of another checkout?  Compiles every translation unit of
# poreseq_amd/csrc/Makefile's SRCS to gfx950 assembly (device side only, no GPU needed) in both trees with the Makefile's flags and
# compares the files, the per-build `__hip_cuid_<hash>` symbol apart.  Host code may be cut into other files between the two: a .cpp
# unit that only one of the trees has passes when its device assembly defines no kernel (no .amdhsa_kernel).
# usage: tools/devasm_diff.sh <other checkout> [scratch dir]
set -u
here=$(cd "$(dirname "$0")/.." && pwd); other=$(cd "$1" && pwd); out=${2:-$(mktemp -d)}
mkdir -p "$out"
flags=$(make -s -C "$here/poreseq_amd/csrc" --eval='show: ; @echo $(CXXFLAGS)' show)
srcs=$(for t in here other; do make -s -C "${!t}/poreseq_amd/csrc" --eval='show: ; @echo $(SRCS)' show; done | tr ' ' '\n' | awk 'NF && !seen[$0]++')
rc=0
for f in $srcs; do
  has=""
  for t in here other; do
    [ -f "${!t}/poreseq_amd/csrc/$f" ] || continue
    has="$has $t"
    ( cd "${!t}/poreseq_amd/csrc" && hipcc $flags --cuda-device-only -S -x hip "$f" -o "$out/$t.$f.s" 2> "$out/$t.$f.err" ) || { echo "$f: does not compile in $t ($out/$t.$f.err)"; rc=1; }
    sed -E -i 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$out/$t.$f.s"
  done
  if [ "$has" != " here other" ]; then
    t=${has# }
    if [ "${f##*.}" = cpp ] && [ -s "$out/$t.$f.s" ] && ! grep -q '\.amdhsa_kernel' "$out/$t.$f.s"; then echo "$f only in $t: no kernel"; else echo "$f only in $t: NOT a kernel-free host unit"; rc=1; fi
  elif cmp -s "$out/here.$f.s" "$out/other.$f.s"; then echo "$f identical"; else echo "$f DIFFERS"; rc=1; fi
done
exit $rc
