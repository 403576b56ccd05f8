"""Inputs for orbit_visibility_compact (include/orbit_abi_ext.h C1-C6).  As in raster_cases, the expected bytes are never
computed here: the GPU tests' reference is the host mirror (orbit_amd.raster.host_visibility_compact), which
tests/test_visibility_compact_cpu.py holds to the numpy restatement tests/visibility_compact_ref.py; what a case
CLAIMS (`expect`, counters known in closed form) is checked against the restatement there.

Census — rasterised (a buffer from ONE ORBIT_RASTER_CLEAR call of the list, so C6 applies):
  every case of raster_vis_cases.all_cases()   ties between and inside commands, nt = 256, the 257-triangle and the R9
                                               commands the raster skipped (they own nothing: not visible), count 0 and
                                               count > max_commands, command_base at the top of the 24 bits
  two_lists, compacted once per base           the other list's pixels are foreign (C6 (a) does not apply: two calls)
Hand-built (no raster; the smallest inputs at which each kernel can go wrong).  CHUNK = 256 is the commands per block of
the scan and the emit (kCompactChunk):
  tiles_WxH              1 x 1, 7 x 5, 64 x 1, 65 x 9, 13 x 11: partial 8 x 8 tiles on both edges, uncovered pixels,
                         ids at base - 1, base, base + n - 1, base + n in turn (the two outer ones foreign)
  one_key_per_tile       one (command, triangle) for a whole wave: one atomic
  64_keys_in_a_tile      64 distinct keys in one tile: 64 rounds of the aggregation
  mask_word_edges        t in {0, 31, 32, 63, 64, 255} of one 256-triangle, 255-vertex command: the mask-word and the
                         emit-round boundaries
  m_1_2_3_4              four commands with 1, 2, 3, 4 visible triangles (3m mod 4 = 3, 2, 1, 0), vcount 3, and
                         cmd_first_index % 4 = 0, 1, 2, 3
  m_256                  every triangle of a 256-triangle command: 192 corner words, the largest region (255 + 192)
  list_N_third           N in {63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1}: every third command visible
  list_65_none / _all    nothing visible; everything visible
  three_chunks           3 * CHUNK + 5 commands, none of the first chunk visible, all of the last two: the carry across
                         the block totals is 0, then CHUNK, and non-zero in both words
  count_zero             a count of 0 over a covered buffer: all foreign
  count_above_max        count 1000, max_commands 3: the device clamps; ids 3, 4 are foreign
  ids_in_n_to_max        count 3 of max_commands 6: ids in [n, max_commands) are foreign (the resolve would own them)
  base_top_of_24_bits    command_base = 2^24 - 3
  inconsistent           a mask bit at t = nt, and a 257-triangle command, each between good neighbours: two
                         range_errors, ORBIT_E_RANGE, the neighbours written
  data_checks_flag_only  commands whose corner bytes reach beyond meshlet_data_words, with vcount 256, and with
                         cmd_first_index / 4 < cmd_vertex_offset: range_errors only with ORBIT_COMPACT_TRIANGLES
Capacities (capacity_variants): visible_capacity exact, one less, 0; visible_data_words exact and one less."""
from dataclasses import dataclass, field

import numpy as np

import raster_cases as rc
import raster_vis_cases as vc
from orbit_amd import layouts as L
from raster_vis_cases import _word

CHUNK = 256
F = np.float32


@dataclass
class CompactCase:
    name: str
    visibility: np.ndarray   # (h, w) uint64
    words: np.ndarray        # {count; commands} as uint32
    max_commands: int
    meshlet_data: np.ndarray
    command_base: int = 0
    meshlet_data_words: int = None
    expect: dict = field(default_factory=dict)      # claimed counters, both modes
    expect_cut: dict = field(default_factory=dict)  # ... with ORBIT_COMPACT_TRIANGLES only
    expect_plain: dict = field(default_factory=dict)
    packed: object = None    # the rc.Packed it was rasterised from (C6 applies), or None
    one_clear_call: bool = True

    def args(self, triangles, **over):
        kw = dict(command_base=self.command_base, meshlet_data=self.meshlet_data, triangles=triangles,
                  meshlet_data_words=self.meshlet_data_words)
        kw.update(over)
        return (self.visibility, self.words, self.max_commands), kw


# -------------------------------------------------------------------------------------------------- rasterised
def rasterised_cases():
    out = []
    for case in vc.all_cases():
        pk = rc.Packed(case)
        vis = vc.host(pk)[0]
        out.append(CompactCase(case.name, vis, pk.words, pk.max_commands, pk.meshlet_data, case.command_base,
                               pk.meshlet_data_words, packed=pk))
    a, b, cap = vc.two_lists()
    pa, pb = rc.Packed(a), rc.Packed(b)
    both = vc.host(pb, visibility=vc.host(pa)[0], clear=False)[0]
    # (list A's capacity is 4, it holds 2: its words are padded to the capacity)
    words_a = np.concatenate([pa.words, np.zeros(7 * (cap - len(pa.commands)), np.uint32)])
    out.append(CompactCase("two_lists_base_0", both, words_a, cap, pa.meshlet_data, 0, pa.meshlet_data_words,
                           expect=dict(visible_commands=2), packed=pa, one_clear_call=False))
    out.append(CompactCase("two_lists_base_cap", both, pb.words, len(pb.commands), pb.meshlet_data, cap, pb.meshlet_data_words,
                           expect=dict(visible_commands=2), packed=pb, one_clear_call=False))
    return out


# -------------------------------------------------------------------------------------------------- hand-built
def build_list(shapes, seed=3):
    """shapes: [(nt, vcount, misalign)] -> ({count; commands} words, meshlet_data).  A command's index words and corner
    bytes are random (no raster reads them); its corner bytes start `misalign` bytes into their first word."""
    rng = np.random.default_rng(seed)
    data, cmds, words = [rng.integers(0, 2**32, 5, dtype=np.uint32)], [], 5
    for k, (nt, vcount, misalign) in enumerate(shapes):
        corner_words = (misalign + 3 * nt + 3) // 4
        cmd = np.zeros((), L.MESHLET_DRAW_COMMAND)
        cmd["cmd_index_count"], cmd["cmd_instance_count"] = 3 * nt, 1
        cmd["cmd_vertex_offset"], cmd["cmd_first_index"] = words, 4 * (words + vcount) + misalign
        cmd["cmd_first_instance"], cmd["meshlet_vertex_offset"], cmd["meshlet_index"] = k % 7, 1000 + k, 5000 + k
        cmds.append(cmd)
        data.append(rng.integers(0, 2**32, vcount + corner_words, dtype=np.uint32))
        words += vcount + corner_words
    cmds = np.array(cmds, L.MESHLET_DRAW_COMMAND) if cmds else np.zeros(0, L.MESHLET_DRAW_COMMAND)
    buf = np.zeros(1 + 7 * len(cmds), np.uint32)
    buf[0] = len(cmds)
    buf[1:] = cmds.view(np.uint32).reshape(-1)
    return buf, np.concatenate(data)


def buffer_of(keys, w, h, holes=0):
    """A (h, w) buffer whose pixel p holds keys[p % len(keys)] = (command id, triangle), 0 where p % holes == holes - 1."""
    p = np.arange(w * h, dtype=np.int64)
    if len(keys) == 0:
        return np.zeros((h, w), np.uint64)
    keys = np.asarray(keys, np.int64).reshape(-1, 2)[p % len(keys)]
    words = _word((F(0.25) + (p % 7).astype(F) / F(16)).astype(F), keys[:, 0], keys[:, 1])
    if holes:
        words[p % holes == holes - 1] = 0
    return words.reshape(h, w)


def hand_cases():
    out = []

    def add(name, keys, size, shapes, base=0, max_commands=None, count=None, holes=0, data_words=None, **expect):
        words, data = build_list(shapes)
        if count is not None:
            words[0] = count
        out.append(CompactCase(name, buffer_of(keys, *size, holes=holes), words, len(shapes) if max_commands is None else max_commands,
                               data, base, data_words, expect=expect.pop("both", {}), expect_cut=expect.pop("cut", {}),
                               expect_plain=expect.pop("plain", {})))
        assert not expect

    small = [(8, 4, 0)] * 5
    for w, h in ((1, 1), (7, 5), (64, 1), (65, 9), (13, 11)):
        base, n = 1000, 5
        keys = [(base - 1, 0), (base, 1), (base + n - 1, 7), (base + n, 2), (base + 2, 3), (base + 2, 5)]
        add(f"tiles_{w}x{h}", keys, (w, h), small, base=base, holes=0 if w * h == 1 else 5)
    add("one_key_per_tile", [(1, 3)], (16, 8), small, both=dict(visible_commands=1, visible_triangles=1, covered_pixels=128))
    add("64_keys_in_a_tile", [(q % 4, q // 4) for q in range(64)], (8, 8), [(16, 9, 0)] * 4,
        both=dict(visible_commands=4, visible_triangles=64))
    add("mask_word_edges", [(0, t) for t in (0, 31, 32, 63, 64, 255)], (7, 5), [(256, 255, 0)],
        both=dict(visible_commands=1, visible_triangles=6), cut=dict(data_words_needed=255 + 5))
    add("m_1_2_3_4", [(k, t) for k in range(4) for t in range(0, 2 * (k + 1), 2)], (13, 11), [(10, 3, k) for k in range(4)],
        both=dict(visible_commands=4, visible_triangles=10), cut=dict(data_words_needed=4 * 3 + 1 + 2 + 3 + 3))
    add("m_256", [(0, t) for t in range(256)], (65, 9), [(256, 255, 0)],
        both=dict(visible_commands=1, visible_triangles=256), cut=dict(data_words_needed=255 + 192))
    for n in (63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1):
        add(f"list_{n}_third", [(k, k % 2) for k in range(0, n, 3)], (64, 4), [(2, 3, k % 4) for k in range(n)],
            both=dict(visible_commands=(n + 2) // 3, foreign_pixels=0))
    add("list_65_none", [], (16, 8), [(2, 3, 0)] * 65, both=dict(visible_commands=0, written_commands=0, covered_pixels=0))
    add("list_65_all", [(k, 1) for k in range(65)], (65, 1), [(2, 3, 0)] * 65, both=dict(visible_commands=65, visible_triangles=65))
    n = 3 * CHUNK + 5
    add("three_chunks", [(k, k % 3) for k in range(CHUNK, n)], (64, 9), [(3, 3 + k % 5, k % 4) for k in range(n)],
        both=dict(visible_commands=n - CHUNK, visible_triangles=n - CHUNK, range_errors=0))
    add("count_zero", [(0, 0), (1, 1)], (7, 5), small, count=0,
        both=dict(visible_commands=0, written_commands=0, covered_pixels=35, foreign_pixels=35))
    add("count_above_max", [(k, k) for k in range(5)], (7, 5), small, count=1000, max_commands=3,
        both=dict(visible_commands=3, foreign_pixels=14))
    add("ids_in_n_to_max", [(k, 1) for k in range(6)], (6, 2), small + [(8, 4, 0)], count=3, max_commands=6,
        both=dict(visible_commands=3, foreign_pixels=6))
    top = (1 << 24) - 3
    add("base_top_of_24_bits", [(top + k, 7 - k) for k in range(3)] + [(top - 1, 0)], (8, 1), small[:3], base=top,
        both=dict(visible_commands=3, foreign_pixels=2))
    add("inconsistent", [(0, 0), (1, 5), (2, 1), (3, 0), (4, 2)], (5, 1), [(8, 4, 0), (5, 4, 1), (8, 4, 2), (257, 4, 3), (8, 4, 0)],
        both=dict(visible_commands=3, range_errors=2, written_commands=3, visible_triangles=3))
    shapes = [(8, 4, 0), (8, 256, 0), (8, 4, 0), (8, 4, 0), (8, 4, 0)]
    words, data = build_list(shapes)
    cmds = words[1:].reshape(-1, 7)
    cmds[2, 3] = cmds[2, 2] // 4 + 1        # cmd_first_index / 4 < cmd_vertex_offset
    cut_words = int(cmds[4, 2]) // 4 + 5    # the last command's corner bytes (6 words) reach one word beyond
    assert cut_words == len(data) - 1
    out.append(CompactCase("data_checks_flag_only", buffer_of([(k, 1) for k in range(5)], 5, 1), words, 5, data, 0, cut_words,
                           expect_plain=dict(visible_commands=5, range_errors=0),
                           expect_cut=dict(visible_commands=2, range_errors=3)))
    return out


def capacity_variants(stats):
    """From a case's uncapped stats (with ORBIT_COMPACT_TRIANGLES) -> [(name, keyword overrides, triangles)]."""
    n, words = int(stats["visible_commands"]), int(stats["data_words_needed"])
    out = [("capacity_exact", dict(visible_capacity=n, visible_data_words=words), True),
           ("capacity_one_less", dict(visible_capacity=n - 1, visible_data_words=words), True),
           ("capacity_zero", dict(visible_capacity=0, visible_data_words=words), True),
           ("data_words_one_less", dict(visible_capacity=n, visible_data_words=words - 1), True),
           ("plain_capacity_exact", dict(visible_capacity=n), False),
           ("plain_capacity_one_less", dict(visible_capacity=n - 1), False),
           ("plain_capacity_zero", dict(visible_capacity=0), False)]
    return out


def c6_misses(name, vis_in, command_base, got, triangles, vis_out, raster_stats, pixels_out, resolve_stats, out_base=0,
              whole=True):
    """C6 of one list: `vis_in` the buffer that was compacted with `command_base`, `got` the compaction's outputs (the
    dict of host_visibility_compact), `vis_out` the buffer the OUTPUT list gave (rasterised with out_base),
    raster_stats its counters (or None), pixels_out / resolve_stats its resolve over [out_base, + written).
    -> list of what does not hold.  Pixels of vis_in that belong to another list are left out of (b) and (c)."""
    import visibility_compact_ref as ref

    missed = []
    vis_in, vis_out = np.asarray(vis_in, np.uint64), np.asarray(vis_out, np.uint64)
    written = int(got["commands"][0])
    if int(got["stats"]["dropped_commands"]) or written != int(got["stats"]["visible_commands"]):
        missed.append("something was dropped: C6 does not apply")
    id_in = ((vis_in >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64)
    k = id_in - command_base
    own = (vis_in != 0) & (k >= 0) & (k < len(got["masks"]) // 8)
    if whole and not own[vis_in != 0].all():
        missed.append("a covered pixel is foreign in a buffer said to be this list's alone")
    both = np.ones_like(own) if whole else own
    if (vis_out[both] >> np.uint64(32) != vis_in[both] >> np.uint64(32)).any():
        missed.append("(a) the high halves differ")
    j = ((vis_out[own] >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64) - out_base
    t, r = (vis_in[own] & np.uint64(255)).astype(np.int64), (vis_out[own] & np.uint64(255)).astype(np.int64)
    if ((j < 0) | (j >= written)).any() or (got["ids"][np.clip(j, 0, max(written - 1, 0))] != id_in[own]).any():
        missed.append("(b) visible_ids[j] is not the pixel's old command")
    want_r = ref.ranks(got["masks"], k[own], t) if triangles else t
    if (r != want_r).any():
        missed.append("(c) the new triangle index is not the rank of the old one")
    if raster_stats is not None and triangles:
        if int(raster_stats["triangles"]) != int(got["stats"]["visible_triangles"]):
            missed.append(f"(d) {int(raster_stats['triangles'])} triangles rasterised, {int(got['stats']['visible_triangles'])} visible")
        skipped = {q: int(raster_stats[q]) for q in ("clip_skipped", "guard_skipped", "back_facing", "no_coverage", "range_errors")}
        if any(skipped.values()):
            missed.append(f"(d) skip counters {skipped}")
    if resolve_stats is not None and int(resolve_stats["visible_commands"]) != written:
        missed.append(f"the resolve sees {int(resolve_stats['visible_commands'])} commands of {written} written")
    if pixels_out is not None and not np.asarray(pixels_out)[:written].all():
        missed.append("a written command owns no pixel")
    return [f"{name}: {q}" for q in missed]


CAPACITY_CASES =("m_1_2_3_4", "list_257_third", "three_chunks")
