"""orbit_meshlet_bounds and orbit_mesh_bounds on the MI355X (include/orbit_abi_ext.h): the bounds the
device computes from the vertex buffer equal the host mirror's — the meshlets' byte for byte on every case of
tests/meshlet_bounds_cases.py (the reference is the host export on the same buffers, never a restatement), the meshes'
as float values — nothing else is written, nothing out of range is read, and a refit feeds the culls."""
import importlib.util
import os

import numpy as np
import pytest

import meshlet_bounds_cases as mc
import scenes as sc
from orbit_amd import _lib, assets, gltf
from orbit_amd import layouts as L
from test_gpu_parity import dev, host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL, GUARD = mc.SENTINEL, mc.GUARD


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def engine(torch_mod):
    from orbit_amd.engine import Engine

    e = Engine(0, max_entities=4096, max_dispatches=100000, max_draws=200000)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    return mc.build_cases()


class Guarded:
    """A device copy of `a` between two guard regions of SENTINEL bytes; `ptr` is the address of the copy itself, so
    the byte behind the buffer's last is a guard byte."""

    def __init__(self, torch, a, nbytes=None):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.n = len(a) if nbytes is None else nbytes
        buf = np.full(self.n + 2 * GUARD, SENTINEL, np.uint8)
        buf[GUARD:GUARD + len(a)] = a
        self.t = torch.from_numpy(buf).cuda()
        self.ptr = self.t.data_ptr() + GUARD

    def read(self):
        """the buffer's bytes, after checking both guards"""
        b = host(self.t)
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + self.n:] == SENTINEL).all(), "a guard byte was written"
        return b[GUARD:GUARD + self.n].copy()


def run(torch, engine, pk, records=None, data=None, vertex_count=None, first=0, count=None, indices=None, keep=False,
        with_full=True, capacity=None):
    """One orbit_meshlet_bounds call on guarded copies of pk's buffers -> (records after, full rows after)."""
    records = pk.records if records is None else records
    n = (len(indices) if indices is not None else count)
    rec = Guarded(torch, records)
    dat = Guarded(torch, pk.meshlet_data if data is None else data)
    vb = Guarded(torch, pk.vertices)
    idx = None if indices is None else Guarded(torch, np.asarray(indices, np.uint32))
    full = Guarded(torch, np.zeros(0, np.uint8), nbytes=48 * n) if with_full else None
    engine.meshlet_bounds(rec.ptr, dat.ptr, vb.ptr, pk.vertex_count if vertex_count is None else vertex_count,
                          vertex_stride=pk.stride, position_offset=pk.offset, first_meshlet=first, meshlet_count=n,
                          meshlet_indices=None if idx is None else idx.ptr, full=None if full is None else full.ptr,
                          keep_records=keep, meshlet_capacity=len(records) if capacity is None else capacity,
                          meshlet_data_words=dat.n // 4)
    torch.cuda.synchronize()
    for g in (dat, vb) + (() if idx is None else (idx,)):  # inputs: unchanged, guards included
        g.read()
    return rec.read().view(L.MESHLET), None if full is None else full.read().view(L.MESHLET_BOUNDS_FULL)


def assert_rows_equal(names, got, want, what):
    for k, name in enumerate(names):
        assert got[k].tobytes() == want[k].tobytes(), f"{what} of {name}: device {got[k]} != host {want[k]}"


# -- 1. every census case, byte for byte
@pytest.mark.parametrize("stride,offset", [(12, 0), (32, 0), (32, 20), (16, 4)])
def test_every_case_equals_the_host_export(torch_mod, engine, cases, stride, offset):
    pk = mc.Packed(cases, stride, offset, vertex_offset=3)
    n = pk.count
    want_full, err, _ = pk.host(count=n)
    assert not err.any()
    got_rec, got_full = run(torch_mod, engine, pk, count=n)
    engine.status()
    assert_rows_equal(pk.names, got_full, want_full, "full bounds")
    want_rec = mc.expected_records(pk.records, want_full, err, range(n))
    assert_rows_equal(pk.names + ["spare"] * 3, got_rec, want_rec, "record")  # bytes 20..31 and the spare records included


# -- 2. range form against index-list form; KEEP_RECORDS
def test_index_list_equals_the_range_and_keep_records_writes_no_record(torch_mod, engine, cases):
    pk = mc.Packed(cases, 32, 8)
    n = pk.count
    rng = np.random.default_rng(5)
    sel = rng.permutation(n)[:n // 2]
    sel = np.concatenate([sel, sel[:5], sel[-1:]]).astype(np.uint32)  # sparse, unsorted, with duplicates
    range_rec, range_full = run(torch_mod, engine, pk, count=n)
    list_rec, list_full = run(torch_mod, engine, pk, indices=sel, first=999)  # first_meshlet is not used
    engine.status()
    assert list_full.tobytes() == range_full[sel].tobytes()
    chosen = np.zeros(len(pk.records), bool)
    chosen[sel] = True
    assert list_rec[chosen].tobytes() == range_rec[chosen].tobytes()
    assert list_rec[~chosen].tobytes() == pk.records[~chosen].tobytes()
    # a sub-range in the middle, without `full`
    sub_rec, none = run(torch_mod, engine, pk, first=4, count=9, with_full=False)
    engine.status()
    inside = np.zeros(len(pk.records), bool)
    inside[4:13] = True
    assert none is None and sub_rec[inside].tobytes() == range_rec[inside].tobytes()
    assert sub_rec[~inside].tobytes() == pk.records[~inside].tobytes()
    keep_rec, keep_full = run(torch_mod, engine, pk, count=n, keep=True)
    engine.status()
    assert keep_rec.tobytes() == pk.records.tobytes() and keep_full.tobytes() == range_full.tobytes()


# -- 3. the four range errors, each alone inside a batch of good meshlets
@pytest.mark.parametrize("error", ["index", "data", "vertex", "corner"])
def test_a_range_error_is_latched_and_leaves_its_meshlet_alone(torch_mod, engine, cases, error):
    torch = torch_mod
    from orbit_amd.engine import Engine

    sub = cases[:12]
    pk = mc.Packed(sub, spare_records=0)
    n, bad = pk.count, 5
    good_full, err, _ = pk.host(count=n)
    records, data, vertex_count, indices = pk.records.copy(), pk.meshlet_data.copy(), pk.vertex_count, None
    if error == "index":  # the first record behind the (guard-tight) record buffer
        indices = np.arange(n, dtype=np.uint32)
        indices[bad] = n
    elif error == "data":  # the corners' last word is the first word behind the data buffer
        words = int(records[bad]["vertex_count"]) + (3 * int(records[bad]["triangle_count"]) + 3) // 4
        records[bad]["data_offset"] = len(data) - words + 1
    elif error == "vertex":  # the meshlet's last vertex is the first one behind the vertex buffer
        d0, nv = int(records[bad]["data_offset"]), int(records[bad]["vertex_count"])
        data[d0 + nv - 1] = pk.vertex_count - int(records[bad]["vertex_offset"])
    else:  # a corner names the vertex behind the meshlet's last
        d0, nv = int(records[bad]["data_offset"]), int(records[bad]["vertex_count"])
        data.view(np.uint8)[(d0 + nv) * 4 + 3 * int(records[bad]["triangle_count"]) - 1] = nv
    want_full, want_err, _ = assets.meshlet_bounds(records, data, pk.vertices, vertex_count, count=n, indices=indices)
    assert want_err.tolist() == [int(k == bad) for k in range(n)]  # the reference applies the same checks
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # its own latch
    try:
        got_rec, got_full = run(torch, eng, pk, records=records, data=data, count=n, indices=indices)
        with pytest.raises(_lib.OrbitError) as e:
            eng.status()
        assert e.value.code == _lib.E_RANGE
    finally:
        eng.close()
    assert not got_full[bad].tobytes().strip(b"\0")
    assert_rows_equal(pk.names, got_full, want_full, "full bounds")
    for k in range(n):
        if k != bad:
            assert want_full[k].tobytes() == good_full[k].tobytes()
    want_rec = mc.expected_records(records, want_full, want_err, range(n) if indices is None else indices)
    assert got_rec.tobytes() == want_rec.tobytes()  # the offender keeps its sentinel bytes
    if indices is None:
        assert got_rec[bad].tobytes() == records[bad].tobytes()


# -- 4. argument errors, the empty call, capture on the first call
def test_argument_errors_and_the_empty_call(torch_mod, engine, cases):
    torch = torch_mod
    lib, ctx = engine._lib, engine._ctx
    pk = mc.Packed(cases[:4])
    rec, dat, vb = Guarded(torch, pk.records), Guarded(torch, pk.meshlet_data), Guarded(torch, pk.vertices)
    full = Guarded(torch, np.zeros(0, np.uint8), nbytes=48 * 4)

    def call(**over):
        kw = dict(meshlets=rec.ptr, meshlet_data=dat.ptr, vertices=vb.ptr, vertex_count=pk.vertex_count, meshlet_count=4,
                  full=full.ptr, meshlet_capacity=len(pk.records), meshlet_data_words=dat.n // 4)
        kw.update(over)
        engine.meshlet_bounds(kw.pop("meshlets"), kw.pop("meshlet_data"), kw.pop("vertices"), kw.pop("vertex_count"), **kw)

    assert lib.orbit_meshlet_bounds(ctx, None, None) == _lib.E_INVALID
    for over in (dict(meshlets=None), dict(meshlet_data=None), dict(vertices=None), dict(vertex_stride=8),
                 dict(vertex_stride=32, position_offset=24), dict(vertex_stride=14), dict(vertex_stride=32, position_offset=6),
                 dict(meshlets=rec.ptr + 8), dict(meshlet_data=dat.ptr + 2), dict(vertices=vb.ptr + 1),
                 dict(meshlet_indices=dat.ptr + 2), dict(full=full.ptr + 2), dict(full=None, keep_records=True)):
        with pytest.raises(_lib.OrbitError) as e:
            call(**over)
        assert e.value.code == _lib.E_INVALID, over
    call(meshlet_count=0)
    call(meshlet_count=0, meshlets=None, meshlet_data=None, vertices=None)
    ranges = Guarded(torch, np.zeros(1, L.MESH_BOUNDS_RANGE))
    infos = Guarded(torch, np.zeros(1, L.MESH_INFO))
    for over in (dict(ranges=None), dict(vertices=None), dict(mesh_infos=None), dict(vertex_stride=8),
                 dict(vertex_stride=18), dict(position_offset=2), dict(ranges=ranges.ptr + 2), dict(mesh_infos=infos.ptr + 4)):
        kw = dict(ranges=ranges.ptr, vertices=vb.ptr, vertex_count=pk.vertex_count, mesh_infos=infos.ptr, range_count=1,
                  mesh_capacity=1)
        kw.update(over)
        with pytest.raises(_lib.OrbitError) as e:
            engine.mesh_bounds(kw.pop("ranges"), kw.pop("vertices"), kw.pop("vertex_count"), kw.pop("mesh_infos"), **kw)
        assert e.value.code == _lib.E_INVALID, over
    engine.mesh_bounds(None, None, 0, None, range_count=0, mesh_capacity=0)
    torch.cuda.synchronize()
    engine.status()
    for g in (rec, dat, vb, full, ranges, infos):  # nothing was launched
        g.read()
    assert rec.read().tobytes() == pk.records.tobytes() and (full.read() == SENTINEL).all()


def test_the_first_call_captures_into_a_graph(torch_mod, cases):
    torch = torch_mod
    from orbit_amd.engine import Engine

    sub = cases[:20]
    pk = mc.Packed(sub, 32, 8)
    n = pk.count
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)  # a context that never ran the call
    try:
        rec, dat, vb = dev(torch, pk.records), dev(torch, pk.meshlet_data), dev(torch, pk.vertices)
        full = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
        ranges = dev(torch, np.array([(0, 0, pk.vertex_count)], L.MESH_BOUNDS_RANGE))
        infos = torch.zeros(128, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.meshlet_bounds(rec, dat, vb, pk.vertex_count, vertex_stride=32, position_offset=8, meshlet_count=n, full=full)
            eng.mesh_bounds(ranges, vb, pk.vertex_count, infos, vertex_stride=32, position_offset=8)
        for frame in range(2):
            if frame == 1:  # the vertices move; the graph reads them on replay
                moved = [(c[0], c[1] * np.float32(1.5) + np.float32(0.25), c[2], c[3]) for c in sub]
                pk = mc.Packed(moved, 32, 8)
                vb.copy_(dev(torch, pk.vertices))
            g.replay()
            torch.cuda.synchronize()
            eng.status()
            want_full, err, _ = pk.host(count=n)
            assert_rows_equal(pk.names, host(full).view(L.MESHLET_BOUNDS_FULL), want_full, f"frame {frame}: full bounds")
            assert host(rec).tobytes() == mc.expected_records(pk.records, want_full, err, range(n)).tobytes()
    finally:
        eng.close()


# -- 6. orbit_mesh_bounds
def _mesh_positions(n, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.normal(size=(n, 3)) * (1.0, 3.0, 0.5) + (4.0, -2.0, 0.25)).astype(np.float32)
    if n >= 3:  # the extreme vertex several times, at both ends and in the middle
        far = np.array([40.0, -35.0, 22.0], np.float32)
        pos[0] = pos[n // 2] = pos[n - 1] = far
    return pos


def _assert_mesh_equal(info, pos):
    mn, mx, sp = assets.compute_mesh_bounds(pos)
    # values, not bytes: +0 == -0 (fmin / fmax leave the sign of a zero open); NaN where the host has NaN
    assert np.array_equal(info["aabb_min"][:3], mn) and np.array_equal(info["aabb_max"][:3], mx)
    assert np.array_equal(info["bounding_sphere"], sp, equal_nan=True), (info["bounding_sphere"], sp)


def test_mesh_bounds_equal_the_host_at_every_size(torch_mod, engine):
    torch = torch_mod
    sizes = [0, 1, 63, 64, 65, 4097, 300_001]
    parts = [_mesh_positions(n, 10 + k) for k, n in enumerate(sizes)]
    parts[2][5] = (0.0, -0.0, 0.0)
    stride, offset = 32, 16
    allpos = np.concatenate(parts)
    vbytes = np.full(len(allpos) * stride, SENTINEL, np.uint8)
    np.lib.stride_tricks.as_strided(vbytes[offset:], (len(allpos), 12), (stride, 1))[:] = allpos.view(np.uint8).reshape(-1, 12)
    firsts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    meshes = [9, 0, 3, 4, 1, 7, 5]  # unordered, mesh 2, 6 and 8 unnamed
    ranges = np.array(list(zip(meshes, firsts, sizes)), np.uint32).view(L.MESH_BOUNDS_RANGE).reshape(-1)
    infos0 = np.full(10 * 128, SENTINEL, np.uint8)
    for several in (False, True):  # all ranges in one call, and one call each
        infos, vb, rg = Guarded(torch, infos0), Guarded(torch, vbytes), Guarded(torch, ranges)
        if several:
            engine.mesh_bounds(rg.ptr, vb.ptr, len(allpos), infos.ptr, stride, offset, range_count=len(sizes), mesh_capacity=10)
        else:
            for k in range(len(sizes)):
                engine.mesh_bounds(rg.ptr + 12 * k, vb.ptr, len(allpos), infos.ptr, stride, offset, range_count=1, mesh_capacity=10)
        torch.cuda.synchronize()
        engine.status()
        vb.read(), rg.read()
        out = infos.read()
        rows = out.view(L.MESH_INFO)
        for mesh, pos in zip(meshes, parts):
            _assert_mesh_equal(rows[mesh], pos)
        untouched = np.ones((10, 128), bool)
        for mesh in meshes:  # 3 + 1 + 3 + 3 floats are written: the two w words and bytes 48..127 are not
            untouched[mesh, :12] = untouched[mesh, 12:16] = untouched[mesh, 16:28] = untouched[mesh, 32:44] = False
        assert (out.reshape(10, 128)[untouched] == SENTINEL).all()
    assert np.isnan(rows[9]["bounding_sphere"][:3]).all() and rows[9]["bounding_sphere"][3] == 0  # the empty range
    assert np.isposinf(rows[9]["aabb_min"][:3]).all() and np.isneginf(rows[9]["aabb_max"][:3]).all()


@pytest.mark.parametrize("count", [100, 1500])
def test_mesh_bounds_of_many_ranges(torch_mod, engine, count):
    """100 ranges are cut into 10 slices each; 1500 are not cut and take two batches of the context's scratch."""
    torch = torch_mod
    rng = np.random.default_rng(count)
    sizes = rng.integers(0, 90, count)
    sizes[::7] = 300
    firsts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    pos = (rng.normal(size=(int(sizes.sum()), 3)) * 5).astype(np.float32)
    meshes = rng.permutation(count)
    ranges = np.array(list(zip(meshes, firsts, sizes)), np.uint32)
    infos, vb, rg = Guarded(torch, np.full(count * 128, SENTINEL, np.uint8)), Guarded(torch, pos), Guarded(torch, ranges)
    engine.mesh_bounds(rg.ptr, vb.ptr, len(pos), infos.ptr, range_count=count, mesh_capacity=count)
    torch.cuda.synchronize()
    engine.status()
    rows = infos.read().view(L.MESH_INFO)
    for mesh, first, size in ranges:
        _assert_mesh_equal(rows[mesh], pos[first:first + size])
    raw = rows.view(np.uint8).reshape(count, 128)  # the two w words and bytes 48..127 of every mesh
    assert (raw[:, 28:32] == SENTINEL).all() and (raw[:, 44:] == SENTINEL).all()


@pytest.mark.parametrize("error", ["vertices", "mesh"])
def test_mesh_bounds_range_errors(torch_mod, error):
    torch = torch_mod
    from orbit_amd.engine import Engine

    pos = _mesh_positions(500, 3)
    ranges = np.array([(0, 0, 200), (1, 200, 200), (2, 400, 100)], np.uint32)
    if error == "vertices":
        ranges[1] = (1, 200, 301)  # one vertex behind the buffer
    else:
        ranges[1] = (3, 200, 200)  # the mesh behind the last
    eng = Engine(0, max_entities=1024, max_dispatches=1024, max_draws=1024)
    try:
        infos, vb, rg = Guarded(torch, np.full(3 * 128, SENTINEL, np.uint8)), Guarded(torch, pos), Guarded(torch, ranges)
        eng.mesh_bounds(rg.ptr, vb.ptr, 500, infos.ptr, range_count=3, mesh_capacity=3)
        torch.cuda.synchronize()
        with pytest.raises(_lib.OrbitError) as e:
            eng.status()
        assert e.value.code == _lib.E_RANGE
    finally:
        eng.close()
    rows = infos.read().view(L.MESH_INFO)
    _assert_mesh_equal(rows[0], pos[:200])
    _assert_mesh_equal(rows[2], pos[400:])
    assert (rows[1:2].view(np.uint8) == SENTINEL).all()


# -- 5. end to end: deformed asset, refit on the device, culled from the buffer and from the streams
def test_refit_feeds_the_culls(torch_mod, tmp_path, oracle):
    torch = torch_mod
    from orbit_amd.engine import Engine, depth_pyramid_desc

    spec = importlib.util.spec_from_file_location("make_test_glb", os.path.join(ROOT, "tools", "make_test_glb.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    glb = str(tmp_path / "scene.glb")
    tool.write(glb, instances=120)
    b = gltf.to_scene_buffers(gltf.load(glb))
    pos0, meshlets0, infos0 = b["vertex_positions"], b["meshlets"], b["mesh_infos"]
    # every mesh's vertices: from its vertex_offset to the next mesh's
    order = np.argsort(infos0["vertex_offset"], kind="stable")
    ends = np.append(infos0["vertex_offset"][order][1:], len(pos0))
    ranges = np.zeros(len(infos0), L.MESH_BOUNDS_RANGE)
    for k, m in enumerate(order):
        ranges[m] = (m, infos0["vertex_offset"][m], ends[k] - infos0["vertex_offset"][m])
        mn, mx, sp = assets.compute_mesh_bounds(pos0[ranges[m]["first_vertex"]:ends[k]])
        assert np.array_equal(sp, infos0[m]["bounding_sphere"])  # these are the ranges the loader bounded
    # a smooth, finite deformation: a bend and a swell
    p = pos0.astype(np.float64)
    pos1 = np.stack([p[:, 0] * (1.2 + 0.3 * np.sin(2.0 * p[:, 1])) + 0.4 * np.sin(1.5 * p[:, 2]),
                     p[:, 1] * 1.3 + 0.3 * np.cos(1.1 * p[:, 0]), p[:, 2] * 0.8 + 0.25 * p[:, 0] * p[:, 1]], axis=1).astype(np.float32)
    # the reference: host-recomputed records and mesh infos
    full, err, _ = assets.meshlet_bounds(meshlets0, b["meshlet_data"], pos1, len(pos1))
    assert not err.any()
    meshlets1 = mc.expected_records(meshlets0, full, err, range(len(meshlets0)))
    infos1 = infos0.copy()
    for m in range(len(infos1)):
        r = ranges[m]
        mn, mx, sp = assets.compute_mesh_bounds(pos1[r["first_vertex"]:r["first_vertex"] + r["vertex_count"]])
        infos1[m]["aabb_min"][:3], infos1[m]["aabb_max"][:3], infos1[m]["bounding_sphere"] = mn, mx, sp

    n = int(b["entity_draws"][:4].view(np.uint32)[0])
    draws = b["entity_draws"][4:4 + 12 * n].view(L.ENTITY_DRAW)
    per_draw_max = infos0["mesh_lods"][draws["mesh_index"]][:, :, 1].max(axis=1)
    cap_d, cap_c = int((per_draw_max // 32 + 1).sum()) + 8, int(per_draw_max.sum()) + 8
    vis_words = int(draws["visibility_offset"].max()) + int(per_draw_max.max()) // 32 + 2
    g = {k: dev(torch, b[k]) for k in ("entity_draws", "entities", "materials", "meshlet_data")}
    g_meshlets, g_infos, g_pos = dev(torch, meshlets0), dev(torch, infos0), dev(torch, pos1)
    eng = Engine(0, max_entities=n + 256, max_dispatches=cap_d, max_draws=cap_c, validate_streams=1)
    cam = sc.default_camera(position=(0.0, 1.0, 6.0))
    W, H = 640, 360
    depth = sc.make_depth(5, W, H, cam, n_occluders=12)
    pd = depth_pyramid_desc(W, H)
    ps = (pd.width, pd.height)
    gpyr = torch.zeros(pd.total_texels, dtype=torch.float32, device="cuda")
    eng.depth_reduce(dev(torch, depth), W, H, gpyr)
    opyr, _ = oracle.depth_reduce(depth, W, H)
    rng = np.random.default_rng(5)
    evis0 = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
    mvis0 = rng.integers(0, 2 ** 32, vis_words, dtype=np.uint32) | np.uint32(0x55555555)

    def device_cull(p, infos, meshlets):
        ci = sc.make_cull_info(cam.view, cam.planes, occlusion_pass=p, p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
        evis, mvis = (dev(torch, evis0), dev(torch, mvis0)) if p else (None, None)
        disp = torch.zeros(12 + 16 * cap_d, dtype=torch.uint8, device="cuda")
        draw = torch.zeros(4 + 28 * cap_c, dtype=torch.uint8, device="cuda")
        kw = dict(depth_pyramid=gpyr if p == 2 else None, depth_pyramid_size=ps if p == 2 else (0, 0))
        eng.entity_cull(ci, g["entity_draws"], infos, disp, g["entities"], n, cap_d, visibility_buffer=evis, **kw)
        eng.meshlet_cull(ci, disp, meshlets, draw, g["entities"], g["materials"], cap_d, cap_c,
                         meshlet_visibility_buffer=mvis, material_count=len(b["materials"]), **kw)
        torch.cuda.synchronize()
        eng.status()
        return host(disp), host(draw)

    def oracle_cull(p, infos, meshlets):
        ci = sc.make_cull_info(cam.view, cam.planes, occlusion_pass=p, p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
        odisp, _, dd = oracle.entity_cull(ci, b["entity_draws"], n, infos, b["entities"], cap_d, evis0 if p else None,
                                          opyr if p == 2 else None, ps)
        odraw, _, dc = oracle.meshlet_cull(ci, odisp, meshlets, cap_c, b["entities"], b["materials"], mvis0 if p else None,
                                           opyr if p == 2 else None, ps)
        assert dd == 0 and dc == 0
        return odisp, odraw

    def same(a, o):
        nd = int(o[1][:4].view(np.uint32)[0])
        return np.array_equal(a[0], o[0]) and np.array_equal(a[1][:4 + 28 * nd], o[1][:4 + 28 * nd])

    want = {p: oracle_cull(p, infos1, meshlets1) for p in (0, 2)}
    assert int(want[0][1][:4].view(np.uint32)[0]) > 300
    try:
        # without the refit the cull of the stale bounds is another cull: the refit is needed
        assert not same(device_cull(0, g_infos, g_meshlets), want[0])
        eng.meshlet_bounds(g_meshlets, g["meshlet_data"], g_pos, len(pos1))  # every meshlet of every LOD
        eng.mesh_bounds(dev(torch, ranges), g_pos, len(pos1), g_infos)
        torch.cuda.synchronize()
        eng.status()
        assert host(g_meshlets).tobytes() == meshlets1.tobytes()
        for p in (0, 2):
            assert same(device_cull(p, g_infos, g_meshlets), want[p]), f"pass {p} from the Meshlet buffer"
        ms = eng.meshlet_stream(g_meshlets, 0, len(meshlets0))
        ms.update(g_meshlets, 0, len(meshlets0))
        ms.update_meshes(g_infos, 0, len(infos0))
        eng.bind_meshlet_stream(ms)
        for p in (0, 2):
            assert same(device_cull(p, g_infos, g_meshlets), want[p]), f"pass {p} from the streams"
        assert eng.meshlet_stream_culls() >= 2
        eng.bind_meshlet_stream(None)
        ms.close()
    finally:
        eng.close()
