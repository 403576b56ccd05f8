"""CPU checks of orbit_raster_depth's surface (include/orbit_abi_ext.h): the host mirror that is the GPU
tests' reference equals an independent numpy restatement of R1-R9 (tests/raster_ref.py) byte for byte, the case set of
tests/raster_cases.py reaches what it claims, the layouts match the header, the entry points validate before they touch
a device, and the loop closes: the pass-0 draw list of a scene rasterises to the same depth as the scene unculled."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raster_cases as rc
import raster_scene as rs
import raster_vis_cases as vc
from orbit_amd import _lib, passes, raster
from orbit_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = rc.all_cases()


def assert_same(name, got, want):
    depth, stats, err = got
    wdepth, wstats, werr, _ = want
    for k in rc.ref.STAT_NAMES:
        assert int(stats[k]) == wstats[k], f"{name}: {k} = {int(stats[k])}, restated {wstats[k]}"
    assert list(err) == werr, name
    diff = np.argwhere(depth.view(np.uint32) != wdepth.view(np.uint32))
    assert len(diff) == 0, f"{name}: {len(diff)} pixels differ, first at (y, x) = {diff[0]}"


def test_the_case_set_reaches_what_it_claims(capsys):
    missed = {k: v for k, v in rc.census(CASES).items() if v}
    assert not missed, missed
    assert len(capsys.readouterr().out.splitlines()) == len(CASES)
    restated = [rc.Packed(c).restated() for c in CASES if c.width == 64]
    assert sum(r[3]["lane_triangles"] for r in restated) > 100 and sum(r[3]["wave_triangles"] for r in restated) > 50


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_mirror_equals_the_restatement_on_the_census(case):
    pk = rc.Packed(case)
    assert_same(case.name, pk.host(), pk.restated())
    assert not rc.check_claims(case, *pk.host(), pk.restated()[3])  # the claims hold on the mirror's own output too


def test_host_mirror_draws_a_command_of_more_than_256_triangles():
    """The depth call has no triangle limit: the case whose middle command the visibility call skips (V3) is drawn whole,
    by the mirror and by the restatement alike.  tests/test_raster_depth_gpu.py runs the device against this mirror."""
    pk = rc.Packed(next(c for c in vc.new_cases() if c.name == "nt_257_between_neighbours"))
    assert (pk.case.width, pk.case.height) == (64, 48) and [len(m.corners) for m in pk.case.meshlets] == [1, 257, 1]
    got = pk.host()
    assert_same(pk.case.name, got, pk.restated())
    assert not got[2].any()
    assert (int(got[1]["range_errors"]), int(got[1]["commands"]), int(got[1]["triangles"])) == (0, 3, 259)
    assert (got[0] > 0).sum() > 90  # more than the two neighbours' 45 pixels each: the strip is in the buffer


@pytest.mark.parametrize("stride,offset", [(32, 0), (32, 20)])
def test_host_mirror_reads_strided_vertices(stride, offset):
    for case in CASES[:8]:
        want = rc.Packed(case).host()
        got = rc.Packed(case, stride, offset, vertex_base=1, data_base=0).host()
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], case.name


def test_host_mirror_loads_and_merges():
    """LoadOp::Load: B over A equals A and B together; the restatement agrees on the loaded buffer."""
    a, b = rc.Packed(CASES[0]), rc.Packed(CASES[2])
    da, _, _ = a.host()
    assert_same("load", b.host(depth=da, clear=False), b.restated(depth=da, clear=False))
    dab = b.host(depth=da, clear=False)[0]
    assert dab.tobytes() == np.maximum(da, b.host()[0]).tobytes() and (dab > 0).sum() > (da > 0).sum()


def test_host_mirror_equals_the_restatement_on_a_scene(oracle):
    scene = rs.glb_scene(8)
    w, h = 96, 54
    cam = rs.camera(w, h)
    _, _, draw, _, _ = scene.cull(oracle, cam, 0)
    n = int(draw[:4].view(np.uint32)[0])
    assert n > 200
    got = scene.host_raster(draw, cam, w, h)
    want = rc.ref.raster(draw, n, scene.meshlet_data, scene.vertices, len(scene.vertices), scene.entities,
                         rs.view_proj(cam), w, h)
    assert_same("glb scene", got, want)
    assert int(got[1]["fragments"]) > 0 and int(got[1]["back_facing"]) > 0 and int(got[1]["no_coverage"]) > 0
    assert want[3]["lane_triangles"] > 0


def test_pass0_draw_list_rasterises_to_the_unculled_depth(oracle):
    """The closed loop: what the early cull removes (frustum, cone) covers no sample that the kept meshlets do not
    cover nearer.  No tolerance: the two depth buffers are the same bytes."""
    scene = rs.glb_scene(100)
    w, h = 256, 144
    cam = rs.camera(w, h)
    _, _, pass0, _, _ = scene.cull(oracle, cam, 0)
    everything = scene.all_commands(oracle, cam)
    n0, n_all = int(pass0[:4].view(np.uint32)[0]), int(everything[0])
    print(f"pass 0: {n0} commands, unculled: {n_all}")
    assert n0 < n_all and n_all - n0 >= 0.05 * n_all
    d0, s0, e0 = scene.host_raster(pass0, cam, w, h)
    d1, s1, e1 = scene.host_raster(everything, cam, w, h)
    assert not e0.any() and not e1.any()
    print(f"covered pixels: {int((d0 > 0).sum())} of {w * h}; stats pass 0 {s0}, unculled {s1}")
    assert d0.tobytes() == d1.tobytes()
    assert int(s0["fragments"]) > 0 and int(s1["triangles"]) > int(s0["triangles"]) and (d0 > 0).any()


def test_layouts_match_the_header(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "orbit_abi_ext.h"\nint main(void){return sizeof(OrbitRasterDepth)==160'
                   " && offsetof(OrbitRasterDepth,entity_data)==24 && offsetof(OrbitRasterDepth,stats)==40"
                   " && offsetof(OrbitRasterDepth,vertex_count)==56 && offsetof(OrbitRasterDepth,entity_count)==68"
                   " && offsetof(OrbitRasterDepth,width)==80 && offsetof(OrbitRasterDepth,flags)==88"
                   " && offsetof(OrbitRasterDepth,view_proj)==96 && sizeof(OrbitRasterStats)==32"
                   " && offsetof(OrbitRasterStats,fragments)==24 && ORBIT_RASTER_CLEAR==1 && ORBIT_RASTER_CULL_NONE==2"
                   " && ORBIT_RASTER_MAX_DIM==32768?0:1;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
    j = _lib.RasterDepth
    assert C.sizeof(j) == 160 and j.entity_data.offset == 24 and j.stats.offset == 40 and j.vertex_count.offset == 56
    assert j.entity_count.offset == 68 and j.width.offset == 80 and j.flags.offset == 88 and j.view_proj.offset == 96
    assert L.RASTER_STATS.itemsize == 32 and L.RASTER_STATS.names == rc.ref.STAT_NAMES
    assert (_lib.RASTER_CLEAR, _lib.RASTER_CULL_NONE, _lib.RASTER_MAX_DIM) == (1, 2, 32768)


def test_entry_point_rejects_without_a_device():
    """Without a device only the NULL context and the NULL job can be reached: every other ORBIT_E_INVALID path (flags,
    stride, size, NULL buffers, alignment) lies behind a live context and is exercised by
    tests/test_raster_depth_gpu.py::test_argument_errors_and_the_empty_call; the host mirror's Panic paths below stand
    in for them on the CPU."""
    lib = _lib.load()
    assert lib.orbit_raster_depth(None, C.byref(_lib.RasterDepth()), None) == _lib.E_INVALID
    assert lib.orbit_raster_depth(None, None, None) == _lib.E_INVALID
    assert lib.orbit_abi_version() == 6  # additive


def test_host_mirror_rejects_what_the_device_call_rejects():
    pk = rc.Packed(CASES[0])
    kw, (words, mc, data, vb, vc, ent, vp, w, h) = pk.args()
    for over in (dict(vertex_stride=8), dict(vertex_stride=14), dict(vertex_stride=32, position_offset=24),
                 dict(vertex_stride=32, position_offset=6)):
        with pytest.raises(passes.Panic):
            raster.host_raster_depth(words, mc, data, np.zeros(4096, np.uint8), vc, ent, vp, w, h, **{**kw, **over})
    for size in ((0, 48), (64, 0), (32769, 1)):
        with pytest.raises(passes.Panic):
            raster.host_raster_depth(words, mc, data, vb, vc, ent, vp, *size, **kw)
    h_lib = passes.lib()
    depth = np.zeros((h, w), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    vpc = (C.c_float * 16)(*vp)
    args = [p(words), C.c_uint32(mc), p(data), C.c_uint64(len(data)), p(vb), C.c_uint64(vc), C.c_uint32(12), C.c_uint32(0),
            p(ent), C.c_uint32(1), vpc, p(depth), C.c_uint32(w), C.c_uint32(h), C.c_uint32(0), None, None]
    assert h_lib.orbit_host_raster_depth(*args) == 0
    for k in (0, 2, 4, 8, 10, 11):  # each NULL pointer
        bad = list(args)
        bad[k] = None
        assert h_lib.orbit_host_raster_depth(*bad) == passes.HOST_PANIC, k
    bad = list(args)
    bad[14] = C.c_uint32(4)  # an unknown flag
    assert h_lib.orbit_host_raster_depth(*bad) == passes.HOST_PANIC
