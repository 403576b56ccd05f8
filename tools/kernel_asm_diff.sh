#!/usr/bin/env bash
# usage: bash tools/kernel_asm_diff.sh <revision> <unit> [<unit>...]
#        unit = a translation unit of orbit_amd/csrc (make -C orbit_amd/csrc print-units), e.g. raster_depth_clip
# Did a change move a kernel?  Compiles orbit_amd/csrc/<unit>.hip device-only to gfx950 assembly twice — from <revision>,
# exported to a temporary directory (the tree is not touched), and from the working tree —, each with its own Makefile's
# HIPFLAGS, and compares the two files.  Both compiles run inside their csrc directory on a relative file name, so no
# path reaches the output; the one thing normalised is the compilation unit id (__hip_cuid_<hash>, a symbol that no code
# refers to), which hashes the absolute path.  Prints per unit `identical` or the number of differing lines, and per
# kernel of the working tree's file `identical` or the differing lines of its body (the two files split at the kernels'
# symbols, local labels without their function's number), five keys of its metadata (VGPRs, spilled SGPRs, spilled VGPRs,
# scratch bytes, LDS bytes) and its instruction count; under a kernel that differs, the same figures at <revision>.
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

# <file.s> <dir>: the kernels' bodies as <dir>/<n>.s and <dir>/index: one line `<symbol> <n> <instructions> <five keys>` per
# kernel.  (The metadata's records come last in the file, so it is read twice; their keys are sorted, .wavefront_size
# closes a record.)
split() {
  mkdir "$2" || return 1
  awk -v dir="$2" '
    NR == FNR { if ($1 == ".symbol:") { s = $2; sub(/\.kd$/, "", s); id[s] = ++kernels } next }
    $1 == ".group_segment_fixed_size:" || $1 == ".vgpr_count:" || $1 == ".sgpr_spill_count:" || $1 == ".vgpr_spill_count:" || $1 == ".private_segment_fixed_size:" { k[$1] = $2 }
    $1 == ".symbol:" { sym = $2; sub(/\.kd$/, "", sym) }
    $1 == ".wavefront_size:" { print sym, id[sym], count[sym], k[".vgpr_count:"], k[".sgpr_spill_count:"], k[".vgpr_spill_count:"], k[".private_segment_fixed_size:"], k[".group_segment_fixed_size:"] > (dir "/index") }
    cur == "" && /^[^ \t.;][^ \t]*:/ { s = $1; sub(/:$/, "", s); if (s in id) { cur = s; out = dir "/" id[s] ".s" } next }
    cur != "" && /^\.Lfunc_end[0-9]+:/ { close(out); cur = ""; next }
    cur != "" { line = $0; gsub(/BB[0-9]+_/, "BB_", line); gsub(/\.LJTI[0-9]+_/, ".LJTI_", line); print line > out
                if (line ~ /^\t[a-z]/) count[cur]++ }
  ' "$1" "$1"
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
  split "$tmp/asm/$u.rev.s" "$tmp/asm/$u.rev" && split "$tmp/asm/$u.tree.s" "$tmp/asm/$u.tree" || exit 2
  [ -e "$tmp/asm/$u.tree/index" ] || continue # (a unit without kernels)
  while read -r sym n count v ss vs priv lds; do
    was=$(awk -v s="$sym" '$1 == s' "$tmp/asm/$u.rev/index" 2>/dev/null)
    if [ -z "$was" ]; then verdict="not at $rev"
    elif cmp -s "$tmp/asm/$u.rev/$(echo "$was" | cut -d' ' -f2).s" "$tmp/asm/$u.tree/$n.s"; then verdict=identical
    else verdict="$(diff "$tmp/asm/$u.rev/$(echo "$was" | cut -d' ' -f2).s" "$tmp/asm/$u.tree/$n.s" | grep -c '^[<>]') differing lines"
    fi
    echo "  $sym: $verdict .vgpr_count $v .sgpr_spill_count $ss .vgpr_spill_count $vs .private_segment_fixed_size $priv .group_segment_fixed_size $lds instructions $count"
    if [ -n "$was" ] && [ "$verdict" != identical ]; then
      echo "$was" | { read -r _ _ count v ss vs priv lds
        echo "    at $rev: .vgpr_count $v .sgpr_spill_count $ss .vgpr_spill_count $vs .private_segment_fixed_size $priv .group_segment_fixed_size $lds instructions $count"; }
    fi
  done < "$tmp/asm/$u.tree/index" | c++filt -p
done
exit $differ
