"""The SPIR-V interpreter (oracle/spirv_vm.py) itself: its fused multiply-add is exactly rounded, and — where the
reference's shader binaries are present (copied into oracle/_ref/shaders by build()) — re-running them reproduces the
committed vectors byte for byte, i.e. tests/golden/spirv_*.npz are the interpreter's output on the reference's binaries,
not hand-made data."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
REF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "shaders", "meshlet_cull.comp.spv")  # oracle/Makefile `ref`


def _round_f32(q):
    from test_oracle_cpu import _round_f32 as r
    return r(q)


def test_vm_fma32_is_correctly_rounded():
    from oracle.spirv_vm import fma32

    rng = np.random.default_rng(5)
    a = (rng.integers(1, 2 ** 12, 3000) * 2 + 1).astype(np.float32)
    b = (rng.integers(1, 2 ** 12, 3000) * 2 + 1).astype(np.float32)
    c = rng.integers(-4, 5, 3000).astype(np.float32) * np.float32(2.0) ** rng.integers(-30, -20, 3000).astype(np.float32)
    a[2000:], b[2000:], c[2000:] = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    got = fma32(a, b, c)
    for k in range(len(a)):
        want = _round_f32(Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k])))
        assert float(got[k]) == want, (k, a[k], b[k], c[k])


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference's shader binaries are not in oracle/_ref")
@pytest.mark.parametrize("occlusion_pass,ortho,knife", [(0, False, True), (1, True, False), (2, True, True), (2, False, False)])
def test_rerunning_the_binaries_reproduces_the_committed_cull_vectors(occlusion_pass, ortho, knife):
    import make_spirv_vectors as gen

    seed = 3 + 7 * occlusion_pass + (2 if ortho else 0) + (1 if knife else 0)
    name = f"p{occlusion_pass}_{'ortho' if ortho else 'persp'}_{'knife' if knife else 'plain'}"
    stored = np.load(os.path.join(HERE, "golden", "spirv_cull.npz"))
    fresh = gen.case(seed, occlusion_pass, ortho, knife)
    for k, v in fresh.items():
        assert np.array_equal(np.ascontiguousarray(v).view(np.uint8).reshape(-1),
                              np.ascontiguousarray(stored[f"{name}/{k}"]).view(np.uint8).reshape(-1)), (name, k)


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference's shader binaries are not in oracle/_ref")
@pytest.mark.parametrize("S,ortho,knife", [(64, False, True), (128, True, False)])
def test_rerunning_the_binaries_at_another_dispatch_size_reproduces_the_committed_vectors(S, ortho, knife):
    """tests/golden/spirv_cull_dispatch_sizes.npz: the two cull binaries with spec constant 0 = 64 / 128, pass 0."""
    import make_spirv_vectors as gen

    seed = 3 + (2 if ortho else 0) + (1 if knife else 0)
    name = f"s{S}_p0_{'ortho' if ortho else 'persp'}_{'knife' if knife else 'plain'}"
    stored = np.load(os.path.join(HERE, "golden", "spirv_cull_dispatch_sizes.npz"))
    fresh = gen.case(seed, 0, ortho, knife, S=S)
    for k in ("dispatch_size", "spv_dispatch", "spv_draw"):
        assert np.array_equal(np.ascontiguousarray(fresh[k]).view(np.uint8).reshape(-1),
                              np.ascontiguousarray(stored[f"{name}/{k}"]).view(np.uint8).reshape(-1)), (name, k)


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference's shader binaries are not in oracle/_ref")
@pytest.mark.parametrize("occlusion_pass,ortho,knife", [(0, False, True), (2, False, True), (1, True, False)])
def test_rerunning_the_binaries_contracted_reproduces_the_committed_vectors(occlusion_pass, ortho, knife):
    """tests/golden/spirv_cull_contracted.npz: the same binaries with Dot / matrix products / Length as fma chains."""
    import make_spirv_vectors as gen

    seed = 3 + 7 * occlusion_pass + (2 if ortho else 0) + (1 if knife else 0)
    name = f"p{occlusion_pass}_{'ortho' if ortho else 'persp'}_{'knife' if knife else 'plain'}"
    stored = np.load(os.path.join(HERE, "golden", "spirv_cull_contracted.npz"))
    fresh = gen.case(seed, occlusion_pass, ortho, knife, fused_dot=True)
    for k in ("spv_dispatch", "spv_draw", "spv_evis", "spv_mvis", "spv_task_records", "spv_task_mvis"):
        assert np.array_equal(np.ascontiguousarray(fresh[k]).view(np.uint8).reshape(-1),
                              np.ascontiguousarray(stored[f"{name}/{k}"]).view(np.uint8).reshape(-1)), (name, k)


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference's shader binaries are not in oracle/_ref")
@pytest.mark.parametrize("name,fused_dot", [("v_ortho_1x1", False), ("v_persp_16x256", True)])
def test_rerunning_the_binaries_reproduces_the_committed_hiz_edge_vectors(name, fused_dot):
    """tests/golden/spirv_cull_hiz_edges.npz: pass 2 on the hostile cases of tests/hiz_edges.py, canonical and contracted."""
    import make_spirv_vectors as gen

    stored = np.load(os.path.join(HERE, "golden", "spirv_cull_hiz_edges.npz"))
    fresh = gen.hiz_edges_case(name, fused_dot=fused_dot)
    for k in gen.HIZ_EDGE_INPUTS + gen.HIZ_EDGE_OUTPUTS:
        key = f"{name}/contracted/{k}" if fused_dot and k in gen.HIZ_EDGE_OUTPUTS else f"{name}/{k}"
        assert np.array_equal(np.ascontiguousarray(fresh[k]).view(np.uint8).reshape(-1),
                              np.ascontiguousarray(stored[key]).view(np.uint8).reshape(-1)), key


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference's shader binaries are not in oracle/_ref")
def test_rerunning_the_binaries_reproduces_a_committed_cluster_vector():
    import make_spirv_vectors as gen

    stored = np.load(os.path.join(HERE, "golden", "spirv_cluster.npz"))
    fresh = gen.cluster_case(2, 96, 64, 120, True)
    for k, v in fresh.items():
        assert np.array_equal(np.ascontiguousarray(v).view(np.uint8).reshape(-1),
                              np.ascontiguousarray(stored[f"s2/{k}"]).view(np.uint8).reshape(-1)), k


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference's shader binaries are not in oracle/_ref")
def test_the_compaction_binary_marks_the_same_clusters_with_the_same_header(oracle):
    """active_cluster_compaction.comp.spv (integer-only; a 4x4x4-workgroup dispatch; the last workgroup writes the
    indirect-dispatch header): the header {ceil(n / 256), 1, 1, n} and the SET of cluster indices equal the oracle's.
    The order of the list is the order of the binary's atomic appends — nondeterministic on hardware, workgroup-major in
    the interpreter — where the oracle's canonical order is ascending linear cluster index."""
    import make_spirv_vectors as gen
    from oracle import spirv_vm as vm
    from orbit_amd import layouts as L

    st = np.load(os.path.join(HERE, "golden", "spirv_cluster.npz"))
    for name in ("s1", "s2", "s4", "s5", "s6"):
        masks = st[f"{name}/spv_masks"]
        cc = [int(v) for v in st[f"{name}/push"].view(L.MARK_ACTIVE_PUSH)[0]["cluster_count"]]
        total = cc[0] * cc[1] * cc[2]
        B = {1: masks.view(np.uint8).copy(), 2: np.zeros(16 + 4 * total, np.uint8)}
        m = vm.Machine(vm.Module(gen.CREF + "active_cluster_compaction.comp.spv"), B,
                       np.array(cc + [1, 2], np.uint32).tobytes(), gen.log2, subgroup=32)
        m.run(((cc[0] + 3) // 4, (cc[1] + 3) // 4, (cc[2] + 3) // 4), batch=64)
        ou, dropped = oracle.cluster_compact(cc, masks, total)
        n = int(ou[12:16].view(np.uint32)[0])
        assert dropped == 0 and n > 100 and np.array_equal(B[2][:16], ou[:16])
        assert sorted(B[2][16:16 + 4 * n].view(np.uint32).tolist()) == ou[16:16 + 4 * n].view(np.uint32).tolist()


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference's shader binaries are not in oracle/_ref")
@pytest.mark.parametrize("shader", ["forward/forward.task.spv", "shadow/shadow.task.spv"])
def test_the_other_task_shaders_compute_the_same_task_records(shader):
    """forward.task and shadow.task cull with the same functions as forward_depth_prepass.task (the one the committed
    vectors come from): executed on a knife-edge case they must emit the same counts and payloads."""
    import make_spirv_vectors as gen
    from oracle import oracle, spirv_vm as vm
    from orbit_amd import layouts as L

    stored = np.load(os.path.join(HERE, "golden", "spirv_cull.npz"))
    name = "p0_persp_knife"
    g = lambda k: stored[f"{name}/{k}"]
    B = {3: g("spv_dispatch").copy(), 4: g("entities").view(np.uint8).reshape(-1).copy(),
         5: g("cull_info").view(np.uint8).reshape(-1).copy(), 7: g("mvis_in").view(np.uint8).reshape(-1).copy(),
         8: g("meshlets").view(np.uint8).reshape(-1).copy(), 10: g("materials").view(np.uint8).reshape(-1).copy(),
         12: np.zeros(64, np.uint8), 13: np.zeros(64, np.uint8)}
    mod = vm.Module(gen.REF + shader, spec={0: 32})
    # the registry indices go where the binary's own push-constant block has the members of those names
    index = {"draw_command_buffer": 3, "cull_info_buffer": 5, "vertex_buffer": 12, "meshlet_buffer": 8,
             "meshlet_data_buffer": 13, "entity_buffer": 4, "materials_buffer": 10}
    layout = mod.push_constant_layout()
    assert {"draw_command_buffer", "cull_info_buffer", "meshlet_buffer", "entity_buffer", "materials_buffer"} <= set(layout)
    push = np.zeros(max(o + n for o, n in layout.values()), np.uint8)
    for member, (off, size) in layout.items():
        if size == 4:
            push[off:off + 4].view(np.uint32)[0] = index.get(member, 12)  # anything else: an empty 64-byte buffer
    nrec = int(B[3][:4].view(np.uint32)[0])
    m = vm.Machine(mod, B, push.tobytes(), gen.log2, subgroup=32)
    m.run(nrec)
    want = g("spv_task_records").view(L.MESH_TASK_RECORD)
    assert len(m.emitted) == nrec
    for k, (counts, pay) in enumerate(m.emitted):
        assert counts == (int(want[k]["task_mesh_count"]), 1, 1)
        assert (int(pay[0]), int(pay[1])) == (int(want[k]["entity_index"]), int(want[k]["meshlet_offset"]))
        assert [int(x) & 0xFF for x in pay[2]] == want[k]["meshlet_indices"].tolist()


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference's shader binaries are not in oracle/_ref")
@pytest.mark.parametrize("placement", ["model", "mesh"])
def test_config1_bitset_is_what_the_entity_cull_binary_keeps(placement):
    """BASELINE config 1 (8 192 spheres, frustum only): the fixture's visibility bitset — generated by the oracle — is
    exactly the set of entities entity_cull.comp.spv emits dispatch records for."""
    import make_spirv_vectors as gen
    import scenes as sc
    from oracle import spirv_vm as vm
    from orbit_amd import layouts as L

    g = np.load(os.path.join(HERE, "golden", "config1_spheres.npz"))
    spheres = sc.config1_spheres()
    edb, mesh, ent, _, _ = sc.config1_scene(spheres, placement)
    n = len(spheres)
    ci = sc.make_cull_info(sc.default_camera().view, g["planes"])
    B = {1: np.ascontiguousarray(edb).view(np.uint8).reshape(-1).copy(), 2: mesh.view(np.uint8).reshape(-1).copy(),
         4: ent.view(np.uint8).reshape(-1).copy(), 5: np.array(ci).reshape(1).view(np.uint8).reshape(-1).copy(),
         3: np.zeros(L.DISPATCH_HEADER + 16 * (n + 8), np.uint8)}
    B[3][4:12] = np.array([1, 1], np.uint32).view(np.uint8)
    vm.Machine(gen.module("entity_cull.comp.spv"), B, np.array([1, 2, 3, 4, 5], np.uint32).tobytes(), gen.log2,
               subgroup=32).run((n + 255) // 256, batch=8)
    hdr, recs = L.dispatch_buffer_records(B[3])
    want = np.flatnonzero(np.unpackbits(g["bitset"].view(np.uint8), bitorder="little")[:n])
    assert len(recs) == int(g["count"]) and np.array_equal(recs["entity_index"], want)
    assert bool((recs["meshlet_count"] == 1).all()) and np.array_equal(recs["meshlet_offset"], want)


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference's shader binaries are not in oracle/_ref")
def test_rerunning_the_depth_reduce_binary_reproduces_the_committed_pyramids():
    import make_spirv_vectors as gen

    st = np.load(os.path.join(HERE, "golden", "spirv_pyramid.npz"))
    for name in ("200x120", "33x257", "16x9"):
        seed, sw, sh, w0, h0, mips = (int(x) for x in st[f"{name}/geometry"])
        depth, geo, pyr = gen.pyramid_case(seed, sw, sh)
        assert geo == (w0, h0, mips) and np.array_equal(depth, st[f"{name}/depth"])
        assert np.array_equal(pyr.view(np.uint32), st[f"{name}/spv_pyramid"].view(np.uint32))
