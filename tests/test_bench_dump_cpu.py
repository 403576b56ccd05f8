"""bench.py --dump-outputs: the buffers of the last timed step as float64 arrays (bench.last_step_outputs), on host-built
buffers — whole lists below the size budget, a fixed sample of rows with their indices above it."""
import os

import numpy as np
import torch

import bench
from orbit_amd import layouts as L


def _draw_buffer(n, capacity, seed):
    cmds = np.zeros(n, dtype=L.MESHLET_DRAW_COMMAND)
    rng = np.random.default_rng(seed)
    for f in L.MESHLET_DRAW_COMMAND.names:
        cmds[f] = rng.integers(0, 2 ** 31, n)
    cmds["cmd_vertex_offset"] = -cmds["cmd_vertex_offset"]  # the one signed field keeps its sign
    cmds["meshlet_index"][: min(n, 3)] = 0xFFFFFFF0  # above 2**24 and 2**31: exact in float64
    buf = np.full(L.DRAW_HEADER + 28 * capacity, 0xAB, dtype=np.uint8)
    buf[:4].view("<u4")[0] = n
    buf[L.DRAW_HEADER:L.DRAW_HEADER + 28 * n] = cmds.view(np.uint8)
    return torch.from_numpy(buf), cmds


def _dispatch_buffer(n, capacity):
    recs = np.zeros(n, dtype=L.MESHLET_DISPATCH)
    recs["entity_index"] = np.arange(n) // 8
    recs["meshlet_offset"] = (np.arange(n) % 8) * 32
    recs["meshlet_count"] = 32
    recs["visibility_offset"] = np.arange(n)
    buf = np.zeros(L.DISPATCH_HEADER + 16 * capacity, dtype=np.uint8)
    buf[:12].view("<u4")[:] = (n, 1, 1)
    buf[L.DISPATCH_HEADER:L.DISPATCH_HEADER + 16 * n] = recs.view(np.uint8)
    return torch.from_numpy(buf), recs


def test_whole_lists_below_the_budget():
    draw, cmds = _draw_buffer(1000, 1500, 1)
    disp, recs = _dispatch_buffer(300, 400)
    out = bench.last_step_outputs([("dispatch", disp, L.DISPATCH_HEADER, L.MESHLET_DISPATCH),
                                   ("draw_commands", draw, L.DRAW_HEADER, L.MESHLET_DRAW_COMMAND)])
    assert sorted(out) == ["dispatch", "dispatch_header", "draw_commands", "draw_commands_header"]
    assert all(a.dtype == np.float64 for a in out.values())
    assert list(out["dispatch_header"]) == [300, 1, 1] and list(out["draw_commands_header"]) == [1000]
    assert out["draw_commands"].shape == (1000, 7) and out["dispatch"].shape == (300, 4)
    for j, f in enumerate(L.MESHLET_DRAW_COMMAND.names):  # nothing behind the count is read
        assert np.array_equal(out["draw_commands"][:, j], cmds[f].astype(np.float64)), f
    assert out["draw_commands"][0, 6] == 0xFFFFFFF0 and (out["draw_commands"][:, 3] <= 0).all()
    for j, f in enumerate(L.MESHLET_DISPATCH.names):
        assert np.array_equal(out["dispatch"][:, j], recs[f].astype(np.float64)), f


def test_a_list_over_its_share_is_a_fixed_sample_with_its_rows():
    draw, cmds = _draw_buffer(5000, 5000, 2)
    budget = 2 * 64 * 1024
    a = bench.last_step_outputs([("draw_commands", draw, L.DRAW_HEADER, L.MESHLET_DRAW_COMMAND)], max_bytes=budget)
    b = bench.last_step_outputs([("draw_commands", draw.clone(), L.DRAW_HEADER, L.MESHLET_DRAW_COMMAND)], max_bytes=budget)
    rows = a["draw_commands_rows"].astype(np.int64)
    assert 0 < len(rows) < 5000 and np.all(np.diff(rows) > 0) and rows[-1] < 5000
    assert sum(x.nbytes for x in a.values()) <= budget
    assert all(np.array_equal(a[k], b[k]) for k in a) and sorted(a) == sorted(b)  # the same rows every time
    want = np.stack([cmds[f].astype(np.float64) for f in L.MESHLET_DRAW_COMMAND.names], axis=1)[rows]
    assert np.array_equal(a["draw_commands"], want) and list(a["draw_commands_header"]) == [5000]


def test_a_count_past_the_capacity_reads_only_the_buffer():
    draw, _ = _draw_buffer(10, 10, 3)
    draw[:4].view(torch.int32)[0] = 1 << 30  # an overflowed count: the rows stop at the buffer's end
    out = bench.last_step_outputs([("draw_commands", draw, L.DRAW_HEADER, L.MESHLET_DRAW_COMMAND)])
    assert out["draw_commands"].shape == (10, 7) and out["draw_commands_header"][0] == 1 << 30


def test_the_full_size_bench_frame_fits_in_64_mb(tmp_path):
    """The default bench scene's last step — 195 313 entities x 8 dispatch records, 4 752 422 surviving draw commands —
    written as bench.py writes it: both lists sampled, every file together at most 64 MB."""
    n_rec, n_draw = 195_313 * 8, 4_752_422
    disp = torch.zeros(L.DISPATCH_HEADER + 16 * (n_rec + 8), dtype=torch.uint8)
    disp[:4].view(torch.int32)[0] = n_rec
    draw = torch.zeros(L.DRAW_HEADER + 28 * (195_313 * 256 // 2 + 1024), dtype=torch.uint8)
    draw[:4].view(torch.int32)[0] = n_draw
    out = bench.last_step_outputs([("dispatch", disp, L.DISPATCH_HEADER, L.MESHLET_DISPATCH),
                                   ("draw_commands", draw, L.DRAW_HEADER, L.MESHLET_DRAW_COMMAND)])
    assert "dispatch_rows" in out and "draw_commands_rows" in out
    for name, a in out.items():
        np.save(tmp_path / f"{name}.npy", a)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64_000_000
