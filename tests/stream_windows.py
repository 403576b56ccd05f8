"""Meshlet streams that start past meshlet 0: the windows, the update scripts and a census of what they exercise.

A stream (include/orbit_abi_ext.h "Derived meshlet streams") may cover any range [first, first + capacity) of global meshlet
indices — a rank of the sharded engine holds only its shard — and all of its addressing is written for that: arrays
biased by `first`, bit planes and base32 / block bounds aligned to global index 0, partial words and blocks guarded at
both ends.  Shared by tests/test_stream_windows_cpu.py (conditions on these INPUTS and on the reference) and
tests/test_stream_windows_gpu.py (the library against tests/stream_ref.py and the oracle).

Scenes are scenes.make_scene(..., shuffle=False, lods=1): entity draw i draws entity i and mesh i, meshes are consecutive.
A `Window` is a draw range [b, e) plus `before` / `after` extra meshlets of the neighbouring meshes, so that `first` can
be unaligned while the records stay where their meshes put them; the windows of a scene partition its draws.  `shift`
moves every LOD offset of the scene by K (the high windows: indices around 2^31 and up to 2^32 - 1); the oracle always runs
on the unshifted scene and its commands are expected with meshlet_index + K.

The device buffer of a window (`window_buffer`) is scene.meshlets[m0:m1] between GUARD guard meshlets on either side: NaN
spheres, and offsets that chain with the window's first and last meshlet — a read that strays invalidates a bound or sets
a link bit, and stays inside the allocation.

Scripts are lists of steps (`steps`): ("update", source, lo, n), ("materials", table key or None), ("rewrite", index).
`replay` plays one on the reference and yields after every step; the GPU test applies the same step to the library.
"""
import zlib

import numpy as np

import scenes as sc
from orbit_amd import layouts as L
from stream_ref import StreamRef, data_words

GUARD = 64
FIRST_RESIDUES = (0, 1, 27, 32, 59, 63)   # first % 64 (0: with first != 0)
END_RESIDUES = (0, 1, 32, 33, 63)         # (first + capacity) % 64
SCRIPTS = ("a", "b", "c", "d", "e", "f")
TINY = ("tiny_capacity_1", "tiny_5_at_33", "tiny_64_at_32", "last_record_ends_at_end")
FEATURES = ("whole_update", "cuts_at_word_boundaries", "two_orders", "gap_of_blocks", "second_source_inside_blocks",
            "rewrite_first", "rewrite_last", "rewrite_mod64_0", "rewrite_mod64_31", "rewrite_mod64_32", "rewrite_mod64_63",
            "materials_before_update", "materials_after_update", "materials_none", "materials_beyond_and_mode3",
            "partial_update_with_materials")

_cache = {}


def far_camera():
    """test_block_cull_gpu.far_camera: nearly every aligned record is sparse from here."""
    return sc.default_camera(position=(0.0, 2.0, 600.0), rot=(1.0, 0.0))


# ------------------------------------------------------------------------------------------------------------ scenes
# name -> (scene key, draws [b, e), before, after); the comments give first % 64 and (first + capacity) % 64.  A window
# begins on a multiple of 32 draws (orbit_entity_cull_range asks that of draw_first), so only a scene's last window is short.
_PLAN = {
    "a32": [("a32_head_33", 0, 32, 0, 33),            # first 0, end 1057: 33
            ("a32_59_to_0", 32, 64, 5, 0),            # first 1019: 59, end 2048: 0 — the last record ends the stream
            ("a32_63_to_63", 64, 96, 1, 63),          # first 2047: 63, end 3135: 63
            ("a32_27_to_1", 96, 128, 37, 1),          # first 3035: 27, end 4097: 1
            ("a32_1_to_32", 128, 160, 63, 32),        # first 4033: 1, end 5152: 32
            ("a32_aligned", 160, 192, 0, 0),          # first 5120: 0 and not meshlet 0, end 6144: 0
            ("a32_tiny_64_at_32", 192, 194, 0, 0)],   # two meshes moved up by 32: first 6176: 32, capacity 64
    "a64": [("a64_head_33", 0, 32, 0, 33),            # first 0, end 2081: 33
            ("a64_27_to_0", 32, 64, 37, 0),           # first 2011: 27, end 4096: 0
            ("a64_63_tail", 64, 96, 1, 0)],           # first 4095: 63
}
_DRAWS = {"a32": 194, "a64": 96, "ragged": 65, "ragged2": 33}  # the last draw of the ragged scenes: a tiny stream


def _finish(scene):
    """Alpha modes 0, 1, 2 in turn (every filter of the culls has something to decide), and the counts again."""
    scene.materials["alpha_mode"] = np.arange(len(scene.materials)) % 3
    scene.lod0_meshlets = int(scene.mesh_infos["mesh_lods"][scene.entity_draws["mesh_index"], 0, 1].sum())
    return scene


def scene(key):
    """"a32" / "a64": block-aligned scenes, 194 meshes of 32 and 96 meshes of 64 meshlets, three materials; the second draw
    of every window draws a mesh that begins one meshlet late (its records sit at y % 32 == 1: dense, not covered, whatever
    the camera); the last two meshes of "a32" lie 32 meshlets further up (the meshlets of a 195th mesh are there for
    that).  "ragged" / "ragged2": 65 and 33 meshes of 1..70 meshlets; the last mesh of "ragged" is carved down to one
    meshlet, that of "ragged2" to three meshlets that begin at x + 1 with x % 64 == 33."""
    if key in _cache:
        return _cache[key]
    n = _DRAWS[key]
    if key.startswith("ragged"):
        s = sc.make_scene({"ragged": 211, "ragged2": 229}[key], n, meshlets_per_mesh=(1, 70), shuffle=False, lods=1)
        lod0 = s.mesh_infos["mesh_lods"][:, 0]
        d = n - 1
        if key == "ragged":
            lod0[d, 1] = 1
        else:
            x = int(lod0[d, 0])
            x -= (x - 33) % 64  # (downwards: the scene ends with this mesh)
            assert x >= 0
            lod0[d] = (x + 1, 3)
        # the tiny stream draws something: its entity stands in front of the camera, its cones cull nothing
        s.entities["model_matrix"][d, 12:15] = (1.5, 2.0, -12.0)
        s.meshlets["cone_cutoff"][int(lod0[d, 0]):int(lod0[d, 0] + lod0[d, 1])] = 127
    else:
        per = {"a32": 32, "a64": 64}[key]
        s = sc.make_scene({"a32": 223, "a64": 227}[key], n, n_meshes=n + 1, meshlets_per_mesh=(per, per), n_materials=3,
                          shuffle=False, lods=1)
        for name, b, e, before, _ in _PLAN[key]:
            d = b + 1
            late = 1
            if name == "a64_27_to_0":
                # this window's late mesh begins where (y - first) % 32 == 0 — a pre-test that took the stream's first
                # meshlet for a block's would think its records covered — and its first record runs on into the mesh's
                # second block, whose meshlets are far above every view with cones that cull nothing: drawn by whoever
                # decides them from the first block's bound, culled by the planes
                late = (per * b - before) % 32
                assert late == 27
                away = slice(per * d + 32, per * d + 64)
                s.meshlets["bounding_sphere"][away, 1] += np.float32(1e6)
                s.meshlets["cone_cutoff"][away] = 127
            if name == "a32_tiny_64_at_32":
                s.mesh_infos["mesh_lods"][b:e, 0, 0] += 32
            s.mesh_infos["mesh_lods"][d, 0, 0] += late
            s.mesh_infos["mesh_lods"][d, 0, 1] -= late
    _cache[key] = _finish(s)
    return _cache[key]


def camera(key):
    return sc.default_camera() if key.startswith("ragged") else far_camera()


def cull_info(key, alpha=L.ALPHA_ALL):
    cam = camera(key)
    return sc.make_cull_info(cam.view, cam.planes, alpha_mode_flag=alpha)


# ----------------------------------------------------------------------------------------------------------- windows
class Window:
    def __init__(self, name, key, b, e, before=0, after=0, shift=0, capacity=None):
        self.name, self.key, self.b, self.e, self.shift = name, key, b, e, int(shift)
        lod0 = scene(key).mesh_infos["mesh_lods"][b:e, 0].astype(np.int64)
        self.m0 = int(lod0[:, 0].min()) - before                      # scene-local meshlet indices
        self.m1 = int((lod0[:, 0] + lod0[:, 1]).max()) + after
        if capacity is not None:                                      # a stream shorter than its draws
            self.m1 = self.m0 + capacity
        assert 0 <= self.m0 < self.m1 <= len(scene(key).meshlets), name
        self.first, self.capacity = self.m0 + self.shift, self.m1 - self.m0
        assert self.first + self.capacity <= 0xFFFFFFFF

    def __repr__(self):
        return self.name

    @property
    def scene(self):
        return scene(self.key)

    def meshlets(self):
        """The Meshlets of [first, first + capacity) (a copy)."""
        return self.scene.meshlets[self.m0:self.m1].copy()

    def mesh_infos(self):
        """The scene's MeshInfos with every LOD offset moved by `shift` (mod 2^32: meshes outside the window may wrap;
        they are not drawn)."""
        mi = self.scene.mesh_infos.copy()
        mi["mesh_lods"][:, :, 0] = ((mi["mesh_lods"][:, :, 0].astype(np.uint64) + np.uint64(self.shift)) & np.uint64(0xFFFFFFFF))
        return mi

    def records(self, all_records):
        """The window's share of the scene's dispatch records (entity i is draw i), offsets moved by `shift`."""
        r = all_records[(all_records["entity_index"] >= self.b) & (all_records["entity_index"] < self.e)].copy()
        r["meshlet_offset"] += np.uint32(self.shift)
        return r

    def commands(self, all_commands):
        """The window's slice of the scene's draw commands, meshlet_index moved by `shift`."""
        c = all_commands[(all_commands["cmd_first_instance"] >= self.b) & (all_commands["cmd_first_instance"] < self.e)].copy()
        c["meshlet_index"] += np.uint32(self.shift)
        return c


KEYS = ("a32", "a64", "ragged", "ragged2")


def _ragged_windows(key):
    lod0 = scene(key).mesh_infos["mesh_lods"][:, 0].astype(np.int64)

    def fit(name, b, e, first_mod=None, end_mod=None):
        """before / after so that first % 64 == first_mod and (first + capacity) % 64 == end_mod."""
        m0, m1 = int(lod0[b:e, 0].min()), int((lod0[b:e, 0] + lod0[b:e, 1]).max())
        before = 0 if first_mod is None else (m0 - first_mod) % 64
        after = 0 if end_mod is None else (end_mod - m1) % 64
        return Window(name, key, b, e, before, after)

    if key == "ragged":
        return [fit("ragged_head_32", 0, 32, None, 32), fit("ragged_32_mid", 32, 64, 32, None), Window("ragged_tiny_1", key, 64, 65)]
    return [fit("ragged2_head", 0, 32), Window("ragged2_tiny_5_at_33", key, 32, 33, 1, 1)]


def windows(key=None):
    """The named windows of scene `key` (all scenes: None), in draw order."""
    if key is None:
        return [w for k in KEYS for w in windows(k)]
    if ("windows", key) not in _cache:
        _cache["windows", key] = _ragged_windows(key) if key.startswith("ragged") else \
            [Window(n, key, b, e, bf, af) for n, b, e, bf, af in _PLAN[key]]
    return _cache["windows", key]


def window(name):
    return {w.name: w for w in windows() + high_windows() + [short_window()]}[name]


def high_windows():
    """The draws [32, 64) of "a32" with every LOD offset moved by K (a multiple of 32: the records stay aligned)."""
    if "high" not in _cache:
        b, e = 32, 64
        _cache["high"] = [Window("high_2^31_plus_27", "a32", b, e, 5, 0, shift=(1 << 31) + 27 - (32 * b - 5)),
                          Window("high_ends_at_FFFFFFE0", "a32", b, e, 5, 0, shift=0xFFFFFFE0 - 32 * e),
                          Window("high_ends_at_FFFFFFFF", "a32", b, e, 5, 31, shift=0xFFFFFFE0 - 32 * e)]
        assert all(w.shift % 32 == 0 for w in _cache["high"])
    return _cache["high"]


def short_window():
    """"a32_59_to_0" cut so that the records of its last two draws fall outside the stream."""
    w = {w.name: w for w in windows("a32")}["a32_59_to_0"]
    return Window("a32_59_short", "a32", w.b, w.e, 5, 0, capacity=32 * (w.e - 2) - w.m0)


def window_buffer(w, meshlets=None):
    """GUARD guard meshlets, the window's Meshlets, GUARD guard meshlets: Meshlet[GUARD + capacity + GUARD].  The guards
    have NaN spheres and material 0xFFFF; the one in front of the window chains into its first meshlet (a build that read
    it would set the first link bit), the one behind it continues its last."""
    m = w.meshlets() if meshlets is None else meshlets
    buf = np.zeros(GUARD + len(m) + GUARD, dtype=L.MESHLET)
    buf["bounding_sphere"] = np.nan
    buf["material_index"] = 0xFFFF
    buf["vertex_count"], buf["triangle_count"] = 3, 1  # 4 words of data each
    buf[GUARD:GUARD + len(m)] = m
    front, back = buf[:GUARD], buf[GUARD + len(m):]
    front["vertex_offset"] = m["vertex_offset"][0]
    front["data_offset"] = (np.uint32(m["data_offset"][0]) - np.arange(GUARD, 0, -1, dtype=np.uint32) * np.uint32(4))
    back["vertex_offset"] = m["vertex_offset"][-1]
    last = np.uint32(m["data_offset"][-1]) + data_words(m["vertex_count"][-1:], m["triangle_count"][-1:])[0]
    back["data_offset"] = last + np.arange(GUARD, dtype=np.uint32) * np.uint32(4)
    return buf


# -------------------------------------------------------------------------------------------------------- large case
LARGE_FIRST, LARGE_CAPACITY = 59, (1 << 21) + 64 + 37  # every 8192-workgroup launch takes a second round


def large_meshlets():
    """LARGE_CAPACITY meshlets seeded as record_lists.meshlet_buffer seeds its 4096 (arbitrary words everywhere)."""
    from record_lists import SEED, _u32

    i = np.arange(LARGE_CAPACITY)
    m = np.zeros(LARGE_CAPACITY, dtype=L.MESHLET)
    for a in range(4):
        m["bounding_sphere"][:, a] = sc.rnd_range(SEED, 1 + a, i, -50.0, 50.0)
    m["cone_axis"] = _u32(SEED, 5, i).view(np.int8).reshape(-1, 4)[:, :3]
    m["cone_cutoff"] = sc.rnd_int(SEED, 6, i, -128, 127).astype(np.int8)
    m["vertex_offset"] = _u32(SEED, 7, i)
    near = (np.uint64(1 << 32) - np.uint64(1) - sc.rnd_int(SEED, 9, i, 0, 999).astype(np.uint64)).astype(np.uint32)
    m["data_offset"] = np.where(i % 8 == 3, near, _u32(SEED, 8, i))
    m["material_index"] = sc.rnd_int(SEED, 10, i, 0, 65535).astype(np.uint16)
    m["vertex_count"] = np.where(i % 4 == 1, 255, sc.rnd_int(SEED, 11, i, 0, 255)).astype(np.uint8)
    m["triangle_count"] = np.where(i % 4 == 2, 255, sc.rnd_int(SEED, 12, i, 0, 255)).astype(np.uint8)
    # (three blocks in four without a negative radius: their bounds are valid)
    m["bounding_sphere"][:, 3] = np.where((i + LARGE_FIRST) // 32 % 4 != 0, np.abs(m["bounding_sphere"][:, 3]), m["bounding_sphere"][:, 3])
    # a chain here and there, so that link bits of both values occur: every 5th meshlet continues its predecessor
    c = np.flatnonzero(i % 5 == 4)
    m["vertex_offset"][c] = m["vertex_offset"][c - 1]
    m["data_offset"][c] = m["data_offset"][c - 1] + data_words(m["vertex_count"][c - 1], m["triangle_count"][c - 1])
    return m


def large_materials():
    """300 materials of alpha modes 0..3: indices up to 65535 lie beyond the table, every class occurs."""
    t = np.zeros(300, dtype=L.MATERIAL)
    t["alpha_mode"] = np.arange(300) % 4
    return t


# ----------------------------------------------------------------------------------------------------------- scripts
def materials(w, key):
    """-> (table as the device buffer holds it, count handed to set_materials).  "M0": the scene's.  "M1": the same with
    alpha_mode 3 in entry 1 and the count one short — the last material index lies beyond the table."""
    t = w.scene.materials.copy()
    if key == "M0":
        return t, len(t)
    assert key == "M1"
    t["alpha_mode"][1] = 3
    return t, len(t) - 1


def _rewrite_targets(w):
    """The stream's first and last meshlet, and the meshlets nearest its middle at 0, 31, 32 and 63 mod 64."""
    F, C = w.first, w.capacity
    out = [("rewrite_first", F), ("rewrite_last", F + C - 1)]
    mid = F + C // 2
    for r in (0, 31, 32, 63):
        g = mid + (r - mid) % 64
        if g >= F + C:
            g -= 64
        if F <= g < F + C:
            out.append((f"rewrite_mod64_{r}", g))
    return out


def _cuts(w):
    """40 seeded cuts, and every word boundary and its two neighbours inside the first and last 128 meshlets."""
    F, C = w.first, w.capacity
    rng = np.random.default_rng(zlib.crc32(w.name.encode()))
    cuts = {F, F + C}
    if C > 1:
        cuts |= set(int(x) for x in rng.integers(F + 1, F + C, 40))
    for lo, hi in ((F, min(F + 128, F + C)), (max(F + C - 128, F), F + C)):
        for b in range((lo + 31) // 32 * 32, hi + 1, 32):
            cuts |= {c for c in (b - 1, b, b + 1) if F < c < F + C}
    cuts = sorted(cuts)
    pieces = list(zip(cuts[:-1], cuts[1:]))
    one, two = list(pieces), list(pieces)
    rng.shuffle(one)
    rng.shuffle(two)
    return one, two


def _inside(g, residue):
    """The smallest index >= g that is `residue` mod 32."""
    return g + (residue - g) % 32


def applies(w, script):
    """(c) needs room for two pieces and a gap of several blocks, (d) for a sub-range that begins and ends inside blocks."""
    return w.capacity >= {"c": 12 * 32, "d": 4 * 32}.get(script.split("_")[0], 1)


def steps(w, script):
    """The steps of `script` on window `w`; every stream is created WITHOUT an initial update.
    a   one whole update, then the materials
    b   the materials, then the range in pieces (`_cuts`) in one shuffled order and again in another
    c   the materials, then two pieces that leave several blocks between them ("c_fill": and then the gap)
    d   the materials, source A whole, source B over a sub-range that begins and ends inside blocks, B whole
    e   a whole update and the materials, then in-place rewrites, each followed by the update of that one meshlet
    f   materials before any update, the update, the materials again, None, and a table with class-3 meshlets"""
    F, C = w.first, w.capacity
    whole = ("update", "A", F, C)
    if script == "a":
        return [whole, ("materials", "M0")]
    if script == "b":
        one, two = _cuts(w)
        return [("materials", "M0")] + [("update", "A", a, b - a) for a, b in one + two]
    if script in ("c", "c_fill"):
        p = _inside(F + C // 4, 7)
        q = _inside(p + 4 * 32, 13)
        assert F < p < q < F + C
        out = [("materials", "M0"), ("update", "A", F, p - F), ("update", "A", q, F + C - q)]
        return out + ([("update", "A", p, q - p)] if script == "c_fill" else [])
    if script == "d":
        s = _inside(F + 1, 13)
        t = _inside(s + 2 * 32, 11)
        assert F < s < t < F + C
        return [("materials", "M0"), whole, ("update", "B", s, t - s), ("update", "B", F, C)]
    if script == "e":
        out = [whole, ("materials", "M0")]
        for _, g in _rewrite_targets(w):
            out += [("rewrite", g), ("update", "A", g, 1)]
        return out
    if script == "f":
        return [("materials", "M0"), whole, ("materials", "M0"), ("materials", None), ("materials", "M1")]
    raise ValueError(script)


def rewrite(meshlets, i, n_materials):
    """The in-place rewrite of script (e): sphere, offsets and material index of meshlets[i]."""
    m = meshlets
    m["bounding_sphere"][i, :3] += np.float32(3.0)
    m["bounding_sphere"][i, 3] *= np.float32(1.5)
    m["data_offset"][i] += np.uint32(17)
    m["vertex_offset"][i] ^= np.uint32(0x55)
    m["material_index"][i] = (int(m["material_index"][i]) + 1) % n_materials


def replay(w, script, meshlets=None, tables=None, plan=None):
    """Plays `script` (or the steps of `plan`) on a StreamRef of the window: yields (step, ref, meshlets) after every step —
    `meshlets` being the window's Meshlets as BOTH source buffers hold them then (a rewrite reaches both)."""
    m = w.meshlets() if meshlets is None else meshlets
    ref = StreamRef(w.first, w.capacity)
    for st in steps(w, script) if plan is None else plan:
        if st[0] == "update":
            _, src, lo, n = st
            ref.update(src, m[lo - w.first:lo - w.first + n], lo, n)
        elif st[0] == "materials":
            if st[1] is None:
                ref.set_materials(None)
            else:
                t, count = materials(w, st[1]) if tables is None else tables[st[1]]
                ref.set_materials(t[:count])
        else:
            rewrite(m, st[1] - w.first, len(w.scene.materials))
        yield st, ref, m


def mirrors(ref, meshlets):
    """Does the stream hold, over its hull, what the buffer holds?  (What orbit_meshlet_stream_validate must find: clean
    if so, ORBIT_E_STALE if not — a gap no update reached, a rewrite without its update.)"""
    from stream_ref import meshlet_words

    lo, hi = ref.lo - ref.first, ref.hi - ref.first
    w = meshlet_words(meshlets[lo:hi])
    return bool(ref.derived[lo:hi].all() and np.array_equal(ref.sphere[lo:hi], w[:, :4]) and np.array_equal(ref.cone[lo:hi], w[:, 4])
                and np.array_equal(ref.cmd[lo:hi], w[:, 5:8]))


def stream_meshlets(ref):
    """The Meshlets a cull of the stream evaluates: rebuilt from the reference's arrays (never-derived ones are zero)."""
    w = np.zeros((ref.capacity, 8), np.uint32)
    w[:, :4], w[:, 4], w[:, 5:8] = ref.sphere, ref.cone, ref.cmd
    return w.reshape(-1).view(L.MESHLET)


# ------------------------------------------------------------------------------------------------------------ census
def census(w, script=None):
    """What a (window, script) pair exercises: "first%64=r" / "end%64=r" for the residues above, "unaligned", the TINY
    streams, and the FEATURES of the script."""
    F, C = w.first, w.capacity
    out = set()
    if F % 64 in FIRST_RESIDUES and (F % 64 != 0 or F != 0):
        out.add(f"first%64={F % 64}")
    if (F + C) % 64 in END_RESIDUES:
        out.add(f"end%64={(F + C) % 64}")
    if F % 32:
        out.add("unaligned")
    if C == 1:
        out.add("tiny_capacity_1")
    if C == 5 and F % 64 == 33:
        out.add("tiny_5_at_33")
    if C == 64 and F % 64 == 32:
        out.add("tiny_64_at_32")
    lod0 = w.scene.mesh_infos["mesh_lods"][w.e - 1, 0].astype(np.int64)
    if int(lod0[0] + lod0[1]) + w.shift == F + C:
        out.add("last_record_ends_at_end")
    if script is None or not applies(w, script):
        return out
    st = steps(w, script)
    ups = [s for s in st if s[0] == "update"]
    mats = [i for i, s in enumerate(st) if s[0] == "materials"]
    first_up = min(i for i, s in enumerate(st) if s[0] == "update")
    if any(s[2] == F and s[3] == C for s in ups):
        out.add("whole_update")
    if script == "b":
        ends = {s[2] for s in ups} | {s[2] + s[3] for s in ups}
        near = [b for b in range((F + 31) // 32 * 32, F + C + 1, 32) if b - F <= 128 or F + C - b <= 128]
        if all({c for c in (b - 1, b, b + 1) if F < c < F + C} <= ends for b in near):
            out.add("cuts_at_word_boundaries")
        half = len(ups) // 2
        if sorted(ups[:half]) == sorted(ups[half:]) and ups[:half] != ups[half:]:
            out.add("two_orders")
    if script == "c" and ups[1][2] - (ups[0][2] + ups[0][3]) >= 3 * 32:
        out.add("gap_of_blocks")
    if script == "d" and any(s[1] == "B" and s[2] % 32 and (s[2] + s[3]) % 32 for s in ups) and ups[-1][1:] == ("B", F, C):
        out.add("second_source_inside_blocks")
    if script == "e":
        out |= {name for name, g in _rewrite_targets(w) if ("rewrite", g) in st and ("update", "A", g, 1) in st}
    if mats and mats[0] < first_up:
        out.add("materials_before_update")
        if any(s[3] < C for s in ups):
            out.add("partial_update_with_materials")
    if any(i > first_up and st[i][1] == "M0" for i in mats):
        out.add("materials_after_update")
    if ("materials", None) in st:
        out.add("materials_none")
    if ("materials", "M1") in st:
        out.add("materials_beyond_and_mode3")
    return out
