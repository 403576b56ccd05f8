#!/usr/bin/env bash
# usage: bash tools/vmem_waits.sh <unit> <kernel> [-k out.s] [extra hipcc flags...]
#        unit   = a translation unit of orbit_amd/csrc (make -C orbit_amd/csrc print-units), e.g. meshlet_eval_blocks
#        kernel = a piece of the kernel's demangled name, e.g. meshlet_eval_blocks_kernel (the first kernel that has it)
# Where does a kernel wait for its vector memory?  Compiles orbit_amd/csrc/<unit>.hip device-only to gfx950 assembly with
# the Makefile's HIPFLAGS (asked of the Makefile itself, as tools/kernel_asm_diff.sh does) and prints, in order and with
# their line numbers in the assembly file, the kernel's vector-memory instructions (global_ / buffer_ / flat_ / scratch_
# loads, stores and atomics) and its s_waitcnt lines — nothing else.  Vector loads return in order: an `s_waitcnt vmcnt(n)`
# lets at most the n youngest of the lines above it stay in flight.  -k keeps the assembly file, to read around a line.
# Needs hipcc, no GPU.
set -u -o pipefail
[ $# -ge 2 ] || { sed -n '2,4p' "$0" >&2; exit 2; }
unit=$1; kernel=$2; shift 2
keep=""
if [ "${1:-}" = "-k" ]; then keep=$2; shift 2; fi
root=$(cd "$(dirname "$0")/.." && pwd)
dir=$root/orbit_amd/csrc
hipcc=$(make -C "$dir" -s --no-print-directory --eval='print-hipcc: ; @echo $(HIPCC)' print-hipcc) || exit 2
flags=$(make -C "$dir" -s --no-print-directory --eval='print-hipflags: ; @echo $(HIPFLAGS)' print-hipflags) || exit 2
tmp=$(mktemp -d) || exit 2
trap 'rm -rf "$tmp"' EXIT
(cd "$dir" && $hipcc $flags -Wno-unused-command-line-argument "$@" --cuda-device-only -S "$unit.hip" -o "$tmp/u.s") || exit 2
[ -z "$keep" ] || cp "$tmp/u.s" "$keep"
# the kernels' symbols are the names of the metadata's records; the first whose demangled name has <kernel>
sym=$(awk '$1 == ".symbol:" { s = $2; sub(/\.kd$/, "", s); print s }' "$tmp/u.s" | while read -r s; do
        case "$(echo "$s" | c++filt)" in *"$kernel"*) echo "$s"; break ;; esac
      done)
[ -n "$sym" ] || { echo "no kernel of $unit has '$kernel' in its name" >&2; exit 2; }
echo "# $(echo "$sym" | c++filt)"
awk -v sym="$sym" '
  !in_k && $1 == sym ":" { in_k = 1; next }
  in_k && /^\.Lfunc_end[0-9]+:/ { exit }
  in_k && /^\t(global|buffer|flat|scratch)_(load|store|atomic)|^\ts_waitcnt/ { sub(/^\t/, ""); printf "%6d  %s\n", NR, $0 }
' "$tmp/u.s"
