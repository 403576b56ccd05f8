"""Conditions on the inputs of tests/test_stream_windows_gpu.py and on its reference, checked without a GPU: the windows
and scripts of tests/stream_windows.py reach every residue, tiny stream and script feature they are meant to; the windows
partition their scenes and the oracle's commands; the aligned windows take the per-block path from their camera and have a
record that does not; and tests/stream_ref.py gives one answer for one buffer however the updates were cut."""
import numpy as np
import pytest

import stream_windows as sw
from orbit_amd import layouts as L
from stream_ref import data_words, meshlet_words
from test_block_pipeline_gpu import record_sparse_flags
from test_gpu_parity import run_oracle

KEYS = sw.KEYS


def test_census_floors():
    """Every residue of first and end, every tiny stream, every script feature occurs, and each script runs on an unaligned
    window."""
    ws = sw.windows()
    seen = set().union(*(sw.census(w) for w in ws))
    want = {f"first%64={r}" for r in sw.FIRST_RESIDUES} | {f"end%64={r}" for r in sw.END_RESIDUES} | set(sw.TINY)
    assert want <= seen, sorted(want - seen)
    assert len({w.name for w in ws + sw.high_windows() + [sw.short_window()]}) == len(ws) + 4, "every window is named"
    features = set()
    for script in sw.SCRIPTS:
        on = [w for w in ws if sw.applies(w, script)]
        assert any("unaligned" in sw.census(w) for w in on), f"script {script} runs on no unaligned window"
        features |= set().union(*(sw.census(w, script) for w in on))
    assert set(sw.FEATURES) <= features, sorted(set(sw.FEATURES) - features)
    # the tiny streams take every script that fits them, the whole-range ones at least
    for name in ("ragged_tiny_1", "ragged2_tiny_5_at_33", "a32_tiny_64_at_32"):
        assert all(sw.applies(sw.window(name), s) for s in "abef")
    hi = sw.high_windows()
    assert hi[0].first == (1 << 31) + 27 and hi[1].first + hi[1].capacity == 0xFFFFFFE0
    assert hi[2].first + hi[2].capacity == 0xFFFFFFFF
    assert sw.LARGE_CAPACITY > 1 << 21 and sw.LARGE_FIRST % 64 == 59


@pytest.mark.parametrize("key", KEYS)
def test_windows_partition_their_scene(key):
    ws = sw.windows(key)
    assert ws[0].b == 0 and ws[-1].e == sw.scene(key).entity_draw_count
    assert all(a.e == b.b for a, b in zip(ws, ws[1:]))
    s = sw.scene(key)
    assert np.array_equal(s.entity_draws["entity_index"], np.arange(s.entity_draw_count))
    assert np.array_equal(s.entity_draws["mesh_index"], np.arange(s.entity_draw_count))
    for w in ws:  # the stream holds every meshlet its draws dispatch
        lod0 = s.mesh_infos["mesh_lods"][w.b:w.e, 0].astype(np.int64)
        assert (lod0[:, 0] >= w.m0).all() and (lod0[:, 0] + lod0[:, 1] <= w.m1).all()


@pytest.mark.parametrize("key", KEYS)
def test_oracle_commands_split_into_the_windows(oracle, key):
    ref = run_oracle(oracle, sw.scene(key), sw.cull_info(key))
    n, cmds = L.draw_buffer_commands(ref[1])
    _, recs = L.dispatch_buffer_records(ref[0])
    parts = [w.commands(cmds) for w in sw.windows(key)]
    assert n > 50 and all(len(p) for p in parts)
    assert np.array_equal(np.concatenate(parts).view(np.uint32), cmds.view(np.uint32))
    assert np.array_equal(np.concatenate([w.records(recs) for w in sw.windows(key)]).view(np.uint32), recs.view(np.uint32))


@pytest.mark.parametrize("w", sw.windows("a32") + sw.windows("a64") + sw.high_windows() + [sw.short_window()], ids=repr)
def test_aligned_windows_take_the_block_path_and_leave_it(oracle, w):
    """From the far camera at least half of the window's records are sparse, and at least one is dense because it is not
    covered: it sits at y % 32 != 0 (the window's late mesh) or ends behind the stream (the short window)."""
    scene, cam = w.scene, sw.camera(w.key)
    _, recs = L.dispatch_buffer_records(run_oracle(oracle, scene, sw.cull_info(w.key))[0])
    recs = recs[(recs["entity_index"] >= w.b) & (recs["entity_index"] < w.e)]  # unshifted: the pre-test runs on the scene
    assert len(recs) >= 2
    flags = record_sparse_flags(scene, cam, recs, stream_count=w.capacity, stream_first=w.m0)
    off, cnt = recs["meshlet_offset"].astype(np.int64), recs["meshlet_count"].astype(np.int64)
    uncovered = (off % 32 != 0) | (off < w.m0) | (off + cnt > w.m1)
    assert flags.mean() >= 0.5, f"{flags.mean():.2f} of the records sparse"
    assert uncovered.any() and not flags[uncovered].any()
    if w.name == "a32_59_short":
        assert (off + cnt > w.m1).sum() == 2


def _final(w, script):
    last = None
    for _, ref, m in sw.replay(w, script):
        last = ref
    return last.views()


@pytest.mark.parametrize("name", ["a32_59_to_0", "a64_27_to_0", "ragged_32_mid", "high_ends_at_FFFFFFFF"])
def test_reference_gives_one_answer_however_the_updates_are_cut(name):
    """One whole update; the range in pieces, twice, in two orders; two pieces and then the gap between them."""
    w = sw.window(name)
    a, b, c = _final(w, "a"), _final(w, "b"), _final(w, "c_fill")
    assert a["hull"] == (w.first, w.first + w.capacity)
    assert (a["link_cared"] == a["inside"]).all(), "everything was derived: every link bit counts"
    for k in a:
        for other in (b, c):
            assert np.array_equal(a[k], other[k]) if isinstance(a[k], np.ndarray) else a[k] == other[k], k
    # ... and the answer states the buffer: the re-layout, the chain bits and the classes, meshlet by meshlet
    m = w.meshlets()
    words = meshlet_words(m)
    assert np.array_equal(a["sphere"], words[:, :4]) and np.array_equal(a["cone"], words[:, 4])
    assert np.array_equal(a["mat"], m["material_index"]) and np.array_equal(a["cmd"], words[:, 5:])
    assert np.array_equal(a["cnt"], m["vertex_count"].astype(np.uint16) | m["triangle_count"].astype(np.uint16) << 8)
    g = np.arange(w.first, w.first + w.capacity)
    bit = lambda plane: (a[plane][(g >> 5) - (w.first >> 5)] >> (g & 31).astype(np.uint32)) & 1  # noqa: E731
    chain = np.zeros(len(m), bool)
    chain[1:] = (m["vertex_offset"][1:] == m["vertex_offset"][:-1]) & \
        (m["data_offset"][1:] == m["data_offset"][:-1] + data_words(m["vertex_count"][:-1], m["triangle_count"][:-1]))
    assert np.array_equal(bit("link").astype(bool), chain) and 0 < chain.sum() < len(chain)
    assert np.array_equal(bit("cls0") | bit("cls1") << 1, w.scene.materials["alpha_mode"][m["material_index"]])
    at32 = g % 32 == 0
    assert np.array_equal(a["base32"][(g[at32] >> 5) - (w.first >> 5)], words[at32][:, 5:7])


def test_reference_keeps_what_an_update_does_not_reach():
    """Another source starts the hull over and leaves the arrays outside the new range alone; a partial update re-derives
    the classes of its range only; the link bits around a never-derived meshlet are not compared."""
    w = sw.window("a32_59_to_0")
    seen = [(st, ref.views()) for st, ref, _ in sw.replay(w, "d")]
    (_, whole), (st, sub), (_, again) = seen[1], seen[2], seen[3]
    lo, n = st[2], st[3]
    assert sub["hull"] == (lo, lo + n) and again["hull"] == whole["hull"]
    for k in ("sphere", "cone", "mat", "cmd", "cnt", "cls0", "cls1", "base32", "blk"):
        assert np.array_equal(sub[k], whole[k]) and np.array_equal(again[k], whole[k]), k
    cared = np.unpackbits(sub["link_cared"].view(np.uint8), bitorder="little")
    g0 = (w.first >> 5) * 32
    assert cared.sum() == n - 1 and cared[lo + 1 - g0:lo + n - g0].all()
    gap = [ref.views() for st, ref, _ in sw.replay(w, "c")][-1]
    p, q = sw.steps(w, "c")[1], sw.steps(w, "c")[2]
    hole = slice(p[2] + p[3] - w.first, q[2] - w.first)
    assert not gap["sphere"][hole].any() and not gap["cmd"][hole].any() and gap["hull"] == whole["hull"]
    cls = np.unpackbits(gap["cls0"].view(np.uint8), bitorder="little") | np.unpackbits(gap["cls1"].view(np.uint8), bitorder="little") << 1
    assert (cls[w.first - g0:][hole] == w.scene.materials["alpha_mode"][0]).all(), "set_materials reached the whole capacity"
    assert not np.array_equal(gap["blk"], whole["blk"]) and (gap["blk"]["valid"][(p[2] + p[3]) // 32 + 1 - (w.first >> 5)] == 0)
