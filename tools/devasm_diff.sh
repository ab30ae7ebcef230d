#!/bin/bash
# Is the device code of this tree, kernel for kernel, that of another checkout?  Compiles every translation unit of
# poreseq_amd/csrc/Makefile's SRCS to gfx950 assembly (device side only, no GPU needed) in both trees with the Makefile's flags, cuts
# the assembly into kernels and compares them by symbol across all units — so a kernel may move between units, and host code may be
# cut into other files.  Per kernel: its instruction text (label to .size, jump tables included), its .amdhsa_kernel block (LDS,
# scratch, register blocks) and its resource `.set` lines (VGPRs, SGPRs, scratch).  Assembler comments go first (they embed the
# function's ordinal in its unit, `Header=BB12_8`), and the ordinal in local labels (.LBB<n>_, .Lfunc_end<n>, .LJTI<n>_) becomes `n`.
# A plain diff: every kernel of either tree is listed as identical, DIFFERS, or present in one tree only; exit 0 when all are identical.
# usage: tools/devasm_diff.sh <other checkout> [scratch dir]
set -u
here=$(cd "$(dirname "$0")/.." && pwd); other=$(cd "$1" && pwd); out=${2:-$(mktemp -d)}
mkdir -p "$out"
flags=$(make -s -C "$here/poreseq_amd/csrc" --eval='show: ; @echo $(CXXFLAGS)' show)
rc=0
for t in here other; do
  rm -rf "$out/$t.k"; mkdir -p "$out/$t.k"
  for f in $(make -s -C "${!t}/poreseq_amd/csrc" --eval='show: ; @echo $(SRCS)' show); do
    ( cd "${!t}/poreseq_amd/csrc" && hipcc $flags --cuda-device-only -S -x hip "$f" -o "$out/$t.$f.s" 2> "$out/$t.$f.err" ) || { echo "$f: does not compile in $t ($out/$t.$f.err)"; rc=1; continue; }
    # one file per kernel symbol (a symbol that two units define is appended to: the units come in the Makefile's order in both trees)
    awk -v dir="$out/$t.k" '
      NR == FNR { if ($1 == ".amdhsa_kernel") kern[$2] = 1; next }
      cur == "" && /^[A-Za-z_$][A-Za-z0-9_$]*:/ { n = $1; sub(/:.*/, "", n); if (n in kern) cur = n }
      cur != "" { print >> (dir "/" cur); if ($1 == ".size" && $2 == cur ",") cur = ""; next }
      $1 == ".set" { n = $2; sub(/\.[a-z_]+,$/, "", n); if (n in kern) print >> (dir "/" n) }
    ' "$out/$t.$f.s" "$out/$t.$f.s"
  done
  for k in "$out/$t.k"/*; do
    [ -f "$k" ] || continue
    sed -E -i -e 's/[[:space:]]*;.*$//' -e '/^[[:space:]]*$/d' -e 's/\.LBB[0-9]+_/.LBBn_/g' -e 's/\.Lfunc_(begin|end)[0-9]+/.Lfunc_\1n/g' -e 's/\.LJTI[0-9]+_/.LJTIn_/g' "$k"
  done
done
[ $rc = 0 ] || exit $rc
same=0; total=0
for k in $( (ls "$out/here.k"; ls "$out/other.k") | sort -u ); do
  total=$((total + 1))
  name=$(echo "$k" | c++filt 2>/dev/null || echo "$k")
  if [ ! -f "$out/other.k/$k" ]; then echo "ONLY HERE   $name"; rc=1
  elif [ ! -f "$out/here.k/$k" ]; then echo "ONLY OTHER  $name"; rc=1
  elif cmp -s "$out/here.k/$k" "$out/other.k/$k"; then echo "identical   $name"; same=$((same + 1))
  else echo "DIFFERS     $name  (diff $out/here.k/$k $out/other.k/$k)"; rc=1; fi
done
echo "$same of $total kernels identical in instructions and resources"
exit $rc
