#!/usr/bin/env bash
# usage: bash tools/kernel_asm_diff.sh <revision> <unit> [<unit>...]
#        unit = a translation unit of orbit_amd/csrc (make -C orbit_amd/csrc print-units), e.g. raster_depth_clip
# Did a change move a kernel?  Compiles orbit_amd/csrc/<unit>.hip device-only to gfx950 assembly twice — from <revision>,
# exported to a temporary directory (the tree is not touched), and from the working tree —, each with its own Makefile's
# HIPFLAGS, and compares the two files.  Both compiles run inside their csrc directory on a relative file name, so no
# path reaches the output; the one thing normalised is the compilation unit id (__hip_cuid_<hash>, a symbol that no code
# refers to), which hashes the absolute path.  Prints per unit `identical` or the number of differing lines, and per
# kernel of the working tree's file four keys of its metadata (VGPRs, spilled SGPRs, spilled VGPRs, scratch bytes).
# Exit status 1 if a unit differs, 2 on a usage or build error.  Needs git history and hipcc, no GPU.
# Only orbit_amd/csrc and include are exported from <revision>: a unit that includes a file outside these two
# directories reports `did not compile at <revision>` for that reason (add the directory to the archive line below).
set -u -o pipefail
[ $# -ge 2 ] || { sed -n '2,3p' "$0" >&2; exit 2; }
rev=$1; shift
root=$(git rev-parse --show-toplevel) || exit 2
git -C "$root" rev-parse --verify --quiet "$rev^{commit}" >/dev/null || { echo "no such revision: $rev" >&2; exit 2; }
tmp=$(mktemp -d) || exit 2
trap 'rm -rf "$tmp"' EXIT
mkdir "$tmp/rev" "$tmp/asm"
git -C "$root" archive "$rev" orbit_amd/csrc include | tar -x -C "$tmp/rev" || exit 2

# <tree> <unit> <out.s>: the Makefile's compiler and flags, asked of the Makefile itself
compile() {
  local dir=$1/orbit_amd/csrc
  local hipcc flags
  hipcc=$(make -C "$dir" -s --no-print-directory --eval='print-hipcc: ; @echo $(HIPCC)' print-hipcc) || return 1
  flags=$(make -C "$dir" -s --no-print-directory --eval='print-hipflags: ; @echo $(HIPFLAGS)' print-hipflags) || return 1
  (cd "$dir" && $hipcc $flags -Wno-unused-command-line-argument --cuda-device-only -S "$2.hip" -o "$3") || return 1
  sed -i 's/__hip_cuid_[0-9a-f]*/__hip_cuid_/g' "$3"
}

differ=0
for u in "$@"; do
  compile "$tmp/rev" "$u" "$tmp/asm/$u.rev.s" || { echo "$u: did not compile at $rev" >&2; exit 2; }
  compile "$root" "$u" "$tmp/asm/$u.tree.s" || { echo "$u: did not compile in the working tree" >&2; exit 2; }
  if cmp -s "$tmp/asm/$u.rev.s" "$tmp/asm/$u.tree.s"; then
    echo "$u: identical"
  else
    echo "$u: $(diff "$tmp/asm/$u.rev.s" "$tmp/asm/$u.tree.s" | grep -c '^[<>]') differing lines"
    differ=1
  fi
  # the kernels' records of the amdhsa metadata: the keys are sorted, .wavefront_size closes a record
  awk '$1 == ".symbol:" || $1 == ".vgpr_count:" || $1 == ".sgpr_spill_count:" || $1 == ".vgpr_spill_count:" || $1 == ".private_segment_fixed_size:" { k[$1] = $2 }
       $1 == ".wavefront_size:" { printf "  %s .vgpr_count %s .sgpr_spill_count %s .vgpr_spill_count %s .private_segment_fixed_size %s\n", k[".symbol:"], k[".vgpr_count:"], k[".sgpr_spill_count:"], k[".vgpr_spill_count:"], k[".private_segment_fixed_size:"] }' "$tmp/asm/$u.tree.s" | sed 's/\.kd / /' | c++filt -p
done
exit $differ
