"""The PRODUCT against outputs of the reference's own compiled shaders (tests/golden/spirv_cull.npz; see
tests/test_spirv_vectors_cpu.py): entity_cull + meshlet_cull through the C ABI, from the Meshlet buffer and from the
derived meshlet streams, must reproduce the binaries' dispatch records, draw commands and visibility words."""
import numpy as np
import pytest

from orbit_amd import layouts as L
from test_gpu_parity import dev, host, torch_mod  # noqa: F401
from test_spirv_vectors_cpu import CASES, load_case, vectors  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("source", ["meshlet_buffer", "meshlet_stream"])
@pytest.mark.parametrize("name", CASES)
def test_product_equals_the_reference_binaries(torch_mod, vectors, name, source):
    from orbit_amd.engine import Engine

    torch = torch_mod
    c = load_case(vectors, name)
    p = int(c["ci"]["occlusion_pass"])
    n_draws = int(np.frombuffer(c["draws"][:4].tobytes(), np.uint32)[0])
    cap_d, cap_c = c["caps"]
    eng = Engine(0, max_entities=4096, max_dispatches=cap_d + 64, max_draws=cap_c + 64)
    g = {k: dev(torch, c[k]) for k in ("draws", "mesh_infos", "entities", "meshlets", "materials")}
    if source == "meshlet_stream":
        eng.bind_meshlet_stream(eng.meshlet_stream(g["meshlets"], 0, len(c["meshlets"])))
    evis = dev(torch, c["evis"]) if p else None
    mvis = dev(torch, c["mvis"]) if p else None
    pyr = dev(torch, c["pyr"]) if p == 2 else None
    ps = c["ps"] if p == 2 else (0, 0)
    disp = torch.zeros(L.DISPATCH_HEADER + 16 * cap_d, dtype=torch.uint8, device="cuda")
    draw = torch.zeros(L.DRAW_HEADER + 28 * cap_c, dtype=torch.uint8, device="cuda")
    eng.entity_cull(c["ci"], g["draws"], g["mesh_infos"], disp, g["entities"], n_draws, cap_d, visibility_buffer=evis,
                    depth_pyramid=pyr, depth_pyramid_size=ps)
    eng.meshlet_cull(c["ci"], disp, g["meshlets"], draw, g["entities"], g["materials"], cap_d, cap_c,
                     meshlet_visibility_buffer=mvis, depth_pyramid=pyr, depth_pyramid_size=ps,
                     material_count=len(c["materials"]))
    torch.cuda.synchronize()
    eng.status()
    nrec, ndraw = int(c["spv_dispatch"][:4].view(np.uint32)[0]), int(c["spv_draw"][:4].view(np.uint32)[0])
    assert np.array_equal(host(disp)[:L.DISPATCH_HEADER + 16 * nrec], c["spv_dispatch"]), "dispatch records differ"
    assert np.array_equal(host(draw)[:L.DRAW_HEADER + 28 * ndraw], c["spv_draw"]), "draw commands differ"
    if p:
        assert np.array_equal(host(evis, np.uint32), c["spv_evis"]) and np.array_equal(host(mvis, np.uint32), c["spv_mvis"])
    assert (eng.meshlet_stream_culls() > 0) == (source == "meshlet_stream" and p != 1)
    eng.close()


@pytest.mark.parametrize("name", ["s1", "s2", "s4", "s5", "s6"])
def test_product_equals_the_cluster_binaries(torch_mod, name):
    """cluster_mark / cluster_compact / cluster_assign through the C ABI against mark_active.comp.spv and
    light_culling.comp.spv outputs (tests/golden/spirv_cluster.npz)."""
    from orbit_amd.engine import Engine
    from test_spirv_vectors_cpu import CLUSTER_GOLD, load_cluster_case

    torch = torch_mod
    c = load_cluster_case(np.load(CLUSTER_GOLD), name)
    cc = [int(v) for v in c["push"]["cluster_count"]]
    total = cc[0] * cc[1] * cc[2]
    eng = Engine(0, max_lights=256, max_clusters=total)
    gm = torch.zeros(cc[0] * cc[1], dtype=torch.int32, device="cuda")
    gb = torch.zeros((total, 2), dtype=torch.int32, device="cuda")
    eng.cluster_mark(c["push"], dev(torch, c["depth"]), gm, gb)
    gu = torch.zeros(L.COMPACT_HEADER + 4 * total, dtype=torch.uint8, device="cuda")
    eng.cluster_compact(cc, gm, gu, total)
    na = int(c["unique"][12:16].view(np.uint32)[0])
    lcap = 256 * na + 16
    gl = torch.zeros(L.LIGHT_INDEX_HEADER + 4 * lcap, dtype=torch.uint8, device="cuda")
    gimg = torch.zeros((total, 2), dtype=torch.int32, device="cuda")
    eng.cluster_assign(c["info"], gu, gb, dev(torch, c["lights"]), gl, lcap, gimg)
    torch.cuda.synchronize()
    eng.status()
    assert np.array_equal(host(gm, np.uint32), c["spv_masks"]) and np.array_equal(host(gb, np.uint32).reshape(-1, 2), c["spv_bounds"])
    assert np.array_equal(host(gu)[:16 + 4 * na], c["unique"])
    nl = int(c["spv_light_list"][:4].view(np.uint32)[0])
    assert np.array_equal(host(gl)[:4 + 4 * nl], c["spv_light_list"])
    active = c["unique"][16:16 + 4 * na].view(np.uint32)
    assert np.array_equal(host(gimg, np.uint32).reshape(-1, 2)[active], c["spv_offset_image"][active])
    eng.close()


@pytest.mark.parametrize("source", ["meshlet_buffer", "meshlet_stream"])
@pytest.mark.parametrize("name", CASES)
def test_product_task_path_equals_the_task_shader_binary(torch_mod, vectors, name, source):
    """orbit_meshlet_task_cull against forward/forward_depth_prepass.task.spv's outputs."""
    from orbit_amd.engine import Engine

    torch = torch_mod
    c = load_case(vectors, name)
    p = int(c["ci"]["occlusion_pass"])
    cap_d = c["caps"][0]
    eng = Engine(0, max_entities=4096, max_dispatches=cap_d + 64, max_draws=1024)
    g = {k: dev(torch, c[k]) for k in ("entities", "meshlets", "materials")}
    if source == "meshlet_stream":
        eng.bind_meshlet_stream(eng.meshlet_stream(g["meshlets"], 0, len(c["meshlets"])))
    disp = torch.zeros(L.DISPATCH_HEADER + 16 * cap_d, dtype=torch.uint8, device="cuda")
    disp[:len(c["spv_dispatch"])] = dev(torch, c["spv_dispatch"])
    mvis = dev(torch, c["mvis"]) if p else None
    pyr = dev(torch, c["pyr"]) if p == 2 else None
    n = len(c["spv_task_records"])
    task = torch.full((44 * cap_d + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    eng.meshlet_task_cull(c["ci"], disp, g["meshlets"], task, g["entities"], g["materials"], cap_d,
                          meshlet_visibility_buffer=mvis, depth_pyramid=pyr,
                          depth_pyramid_size=c["ps"] if p == 2 else (0, 0))
    torch.cuda.synchronize()
    eng.status()
    assert np.array_equal(host(task)[:44 * n], c["spv_task_records"].view(np.uint8).reshape(-1)), "task records differ"
    if p == 2:
        assert np.array_equal(host(mvis, np.uint32), c["spv_task_mvis"])
    eng.close()


# ----------------------------------------------------------------------------- depth_reduce / compaction binaries
from test_spirv_vectors_cpu import COMPACT, PYR, PYR_SMALL, pyramid_1080p_input  # noqa: E402


@pytest.mark.parametrize("name", PYR_SMALL)
def test_product_pyramid_equals_the_depth_reduce_binary(torch_mod, name):
    """orbit_depth_reduce against depth_reduce.comp.spv's own pyramids (tests/golden/spirv_pyramid.npz)."""
    from orbit_amd.engine import Engine, depth_pyramid_desc

    torch = torch_mod
    v = np.load(PYR)
    seed, sw, sh, w0, h0, mips = (int(x) for x in v[f"{name}/geometry"])
    d = depth_pyramid_desc(sw, sh)
    assert (d.width, d.height, d.mip_levels) == (w0, h0, mips)
    eng = Engine(0)
    pyr = torch.full((d.total_texels + 64,), -1.0, dtype=torch.float32, device="cuda")
    eng.depth_reduce(dev(torch, v[f"{name}/depth"]), sw, sh, pyr)
    torch.cuda.synchronize()
    eng.status()
    got = host(pyr, np.uint32)
    assert np.array_equal(got[:d.total_texels], v[f"{name}/spv_pyramid"].view(np.uint32))
    assert (got[d.total_texels:] == np.float32(-1.0).view(np.uint32)).all(), "written past the pyramid"
    eng.close()


def test_product_pyramid_1080p_equals_the_depth_reduce_binary(torch_mod):
    """The 1920x1080 -> 1024x1024 level 0 (fractional footprint) and the ten levels above it."""
    import hashlib

    from orbit_amd.engine import Engine, depth_pyramid_desc

    torch = torch_mod
    depth, (sw, sh, w0, h0, mips), want = pyramid_1080p_input()
    d = depth_pyramid_desc(sw, sh)
    assert (d.width, d.height, d.mip_levels) == (w0, h0, mips)
    eng = Engine(0)
    pyr = torch.zeros(d.total_texels, dtype=torch.float32, device="cuda")
    eng.depth_reduce(dev(torch, depth), sw, sh, pyr)
    torch.cuda.synchronize()
    eng.status()
    assert hashlib.sha256(pyr.cpu().numpy().tobytes()).digest() == want
    eng.close()


@pytest.mark.parametrize("name", ["s1", "s2", "s4", "s5", "s6"])
def test_product_compaction_equals_the_binary_as_a_multiset(torch_mod, name):
    """orbit_cluster_compact against active_cluster_compaction.comp.spv: same header, same clusters (the binary's list
    is in the order of its atomic appends; the product's is ascending)."""
    from orbit_amd.engine import Engine

    torch = torch_mod
    v = np.load(COMPACT)
    cc = [int(x) for x in v[f"{name}/cluster_count"]]
    spv = v[f"{name}/spv_unique"]
    total = cc[0] * cc[1] * cc[2]
    eng = Engine(0, max_clusters=total)
    out = torch.zeros(16 + 4 * total, dtype=torch.uint8, device="cuda")
    eng.cluster_compact(cc, dev(torch, v[f"{name}/masks"]), out, total)
    torch.cuda.synchronize()
    eng.status()
    got = host(out)
    n = int(spv[12:16].view(np.uint32)[0])
    assert np.array_equal(got[:16], spv[:16])
    ids = got[16:16 + 4 * n].view(np.uint32)
    assert np.array_equal(ids, np.sort(spv[16:16 + 4 * n].view(np.uint32))) and (np.diff(ids.astype(np.int64)) > 0).all()
    eng.close()


# ----------------------------------------------------------------------------- light clusters at the other shapes
from test_spirv_vectors_cpu import CLUSTER_SHAPE_CASES, CLUSTER_SHAPES_GOLD, load_cluster_case  # noqa: E402


@pytest.mark.parametrize("max_lights", ["exact", 4096])
@pytest.mark.parametrize("name", CLUSTER_SHAPE_CASES)
def test_product_equals_the_cluster_binaries_at_other_shapes(torch_mod, name, max_lights):
    """cluster_mark / cluster_compact / cluster_assign, and compute_clusters, against the binaries' outputs at the shapes
    of tests/golden/spirv_cluster_shapes.npz.  The Engine's max_lights sets the coarse segment size (abi_ctx.hip:
    round64(ceil(max_lights / 16))): "exact" makes the light count equal to max_lights, 4096 puts every light of these
    cases into the first few segments."""
    from orbit_amd.engine import Engine

    torch = torch_mod
    c = load_cluster_case(np.load(CLUSTER_SHAPES_GOLD), name)
    cc = [int(v) for v in c["push"]["cluster_count"]]
    total = cc[0] * cc[1] * cc[2]
    n_lights = len(c["lights"])
    assert int(c["info"]["global_light_count"]) == n_lights
    eng = Engine(0, max_lights=max(n_lights, 1) if max_lights == "exact" else max_lights, max_clusters=total)
    lights = dev(torch, c["lights"]) if n_lights else None
    depth = dev(torch, c["depth"])
    na = int(c["unique"][12:16].view(np.uint32)[0])
    active = c["unique"][16:16 + 4 * na].view(np.uint32)
    nl = int(c["spv_light_list"][:4].view(np.uint32)[0])
    lcap = 256 * na + 16

    def check(gm, gb, gu, gl, gimg):
        assert np.array_equal(host(gm, np.uint32), c["spv_masks"]), "tile slice masks differ"
        assert np.array_equal(host(gb, np.uint32).reshape(-1, 2), c["spv_bounds"]), "depth bounds differ"
        assert np.array_equal(host(gu)[:16 + 4 * na], c["unique"]), "compacted list differs"
        assert np.array_equal(host(gl)[:4 + 4 * nl], c["spv_light_list"]), "light index lists differ"
        assert bool((host(gl)[4 + 4 * nl:] == 0xEE).all()), "written past the light list"
        img = host(gimg, np.uint32).reshape(-1, 2)
        assert np.array_equal(img[active], c["spv_offset_image"][active]), "(offset, count) image differs"

    gm = torch.full((cc[0] * cc[1],), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    gb = torch.full((total, 2), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    eng.cluster_mark(c["push"], depth, gm, gb)
    gu = torch.full((L.COMPACT_HEADER + 4 * total,), 0xEE, dtype=torch.uint8, device="cuda")
    eng.cluster_compact(cc, gm, gu, total)
    gl = torch.full((L.LIGHT_INDEX_HEADER + 4 * lcap,), 0xEE, dtype=torch.uint8, device="cuda")
    gimg = torch.zeros((total, 2), dtype=torch.int32, device="cuda")
    eng.cluster_assign(c["info"], gu, gb, lights, gl, lcap, gimg)
    torch.cuda.synchronize()
    eng.status()
    check(gm, gb, gu, gl, gimg)
    # the three stages behind one call
    gm2, gb2 = torch.full_like(gm, 0x55), torch.full_like(gb, 0x55)
    gu2, gl2, gimg2 = torch.full_like(gu, 0xEE), torch.full_like(gl, 0xEE), torch.zeros_like(gimg)
    eng.compute_clusters(c["push"], c["info"], depth, lights, gm2, gb2, gu2, total, gl2, lcap, gimg2)
    torch.cuda.synchronize()
    eng.status()
    check(gm2, gb2, gu2, gl2, gimg2)
    eng.close()
