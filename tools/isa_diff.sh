#!/usr/bin/env bash
# usage: bash tools/isa_diff.sh TREE_A TREE_B  — is the device code of two checkouts the same?
# For every .hip in SRC of spicey_amd/csrc/Makefile (TREE_B's list) each tree's copy is compiled to device assembly with
# its own Makefile's HIPCC, ARCH and CXXFLAGS, and the two are diffed without the lines that name the per-compile
# __hip_cuid_<hash>.  Prints the count of differing lines per file; exit status 1 if any count is not 0.  Compiles and
# diffs only: no GPU.  The assembly is kept in $ISA_DIFF_OUT (default: a fresh temporary directory) as <file>.{a,b}.s.
set -u
[ $# -eq 2 ] || { echo "usage: $0 TREE_A TREE_B" >&2; exit 2; }
A=$(cd "$1" && pwd) || exit 2
B=$(cd "$2" && pwd) || exit 2
OUT=${ISA_DIFF_OUT:-$(mktemp -d)}
mkdir -p "$OUT"

mkvar() {  # mkvar TREE NAME: the value of a variable of that tree's csrc Makefile
  make -s --no-print-directory -C "$1/spicey_amd/csrc" --eval 'isa-diff-print-%: ; @echo $($*)' "isa-diff-print-$2"
}
to_asm() {  # to_asm TREE FILE.hip OUT.s
  (cd "$1/spicey_amd/csrc" && $(mkvar "$1" HIPCC) --offload-arch="$(mkvar "$1" ARCH)" $(mkvar "$1" CXXFLAGS) --cuda-device-only -S -o "$3" "$2")
}

bad=0
for f in $(mkvar "$B" SRC); do
  case "$f" in *.hip) ;; *) continue ;; esac
  to_asm "$A" "$f" "$OUT/$f.a.s" & pa=$!
  to_asm "$B" "$f" "$OUT/$f.b.s" & pb=$!
  wait $pa; ra=$?
  wait $pb; rb=$?
  [ $ra -eq 0 ] && [ $rb -eq 0 ] || { echo "$f: compile failed"; bad=1; continue; }
  n=$(diff <(grep -v __hip_cuid_ "$OUT/$f.a.s") <(grep -v __hip_cuid_ "$OUT/$f.b.s") | grep -c '^[<>]')
  echo "$f: $n differing lines ($(wc -l < "$OUT/$f.b.s") lines of assembly)"
  [ "$n" -eq 0 ] || bad=1
done
echo "assembly kept in $OUT"
exit $bad
