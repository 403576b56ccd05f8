"""numpy classifier of orbit_cull_stats: every entity-draw and every meshlet of a cull, by the first test that rejected it.

Built from tests/np_restatement.py's primitives (transform_sphere, plane_test, occlusion_test, hiz_sample, log2c, dot3),
which are pinned to the oracle and through it to the reference's binaries; the order of the tests is the shaders'
(shaders/entity_cull.comp:106-230, meshlet_cull.comp:108-214).  Canonical arithmetic (arith_profile 0).
`classify` returns the counters under OrbitCullStats' names, and the entity stage's records and the meshlet stage's
drawn mask for the consistency checks against np_restatement.entity_cull / meshlet_cull and the oracle.
"""
import numpy as np

import np_restatement as R
from orbit_amd import layouts as L

F = np.float32


def _lod(ci, x, y, z, r, mi):
    """The LOD whose MeshLod is read (:203-209): after min_/max_mesh_lod, lod_count - 1 and the 8 slots."""
    t = ci["lod_target_pos_view_space"]
    ex, ey, ez = (t[0] - x).astype(F), (t[1] - y).astype(F), (t[2] - z).astype(F)
    with np.errstate(all="ignore"):
        dist = (np.sqrt(R.dot3(ex, ey, ez, ex, ey, ez), dtype=F) - r).astype(F)
        lf = (R.log2c((R.gmax(dist, F(0.0)) / F(ci["lod_base"])).astype(F)) / R.log2c(np.array([ci["lod_step"]], F))).astype(F)
        lod = R.f2u_sat(R.gmax((lf + F(1.0)).astype(F), F(0.0)))
    lod = np.minimum(np.maximum(lod, int(ci["min_mesh_lod"])), int(ci["max_mesh_lod"]))
    lod = np.minimum(lod, (mi["lod_count"].astype(np.uint64) - 1) & 0xFFFFFFFF)
    return np.minimum(lod, 7).astype(np.int64)


def classify_entities(ci, draws, count, entity_draw_count, mesh_infos, entities, vis_words=None, pyr=None, pyr_size=(0, 0)):
    """-> (counters, records [MESHLET_DISPATCH, S = 32], drawn [bool per evaluated entity-draw])."""
    end = min(count, (entity_draw_count + 255) // 256 * 256)
    draws = draws[:end]
    g = np.arange(end)
    mi = mesh_infos[draws["mesh_index"]]
    op = int(ci["occlusion_pass"])
    meshlet_occ = int(ci["meshlet_visibility_buffer"]) != L.NONE
    vib = np.ones(end, dtype=bool)
    if op in (1, 2):
        vib = ((vis_words[g // 32] >> (g % 32).astype(np.uint32)) & 1).astype(bool)
    gated = vib if op == 1 else np.ones(end, dtype=bool)
    mv = R.mat_mul(ci["view_matrix"], entities[draws["entity_index"]]["model_matrix"])
    x, y, z, r, scale = R.transform_sphere(mv, mi["bounding_sphere"])
    inside = gated & R.plane_test(ci, x, y, z, r)
    visible = inside.copy()
    if op == 2:
        ov, zf = R.occlusion_test(ci, x, y, z, r, pyr, *pyr_size, mi["bounding_sphere"][:, 3].astype(F), scale)
        if int(ci["projection_type"]) == 0:
            z = np.where(inside, zf, z).astype(F)  # the flip persists into the LOD distance
        visible = inside & ov
    drawn = visible & (~vib | meshlet_occ) if op == 2 else visible
    lod = _lod(ci, x, y, z, r, mi)
    c = dict(entities=end, entity_skipped_prev_invisible=int((~gated).sum()),
             entity_frustum_culled=int((gated & ~inside).sum()), entity_occlusion_culled=int((inside & ~visible).sum()),
             entity_drawn_in_early_pass=int((visible & ~drawn).sum()), entity_drawn=int(drawn.sum()),
             lod_drawn=[int((drawn & (lod == k)).sum()) for k in range(8)])
    records = []
    for i in np.nonzero(drawn)[0]:
        off, cnt = (int(v) for v in mi["mesh_lods"][i, lod[i]])
        vo = int(draws["visibility_offset"][i])
        for j in range((cnt + R.S - 1) // R.S):
            records.append((int(draws["entity_index"][i]), off + R.S * j, min(cnt - R.S * j, R.S), vo + j))
    records = np.array(records, dtype=np.uint32).reshape(-1, 4).view(L.MESHLET_DISPATCH).reshape(-1)
    c["records"] = len(records)
    return c, records, drawn


def classify_meshlets(ci, records, meshlets, entities, materials, mvis=None, pyr=None, pyr_size=(0, 0)):
    """-> (counters, drawn [bool per active (record, lane) in record order])."""
    op = int(ci["occlusion_pass"])
    meshlet_occ = int(ci["meshlet_visibility_buffer"]) != L.NONE
    lane = np.tile(np.arange(R.S), len(records))
    rid = np.repeat(np.arange(len(records)), R.S)
    active = lane < records["meshlet_count"][rid]
    rid, lane = rid[active], lane[active]
    rec = records[rid]
    m = meshlets[rec["meshlet_offset"].astype(np.int64) + lane]
    mv = R.mat_mul(ci["view_matrix"], entities["model_matrix"][rec["entity_index"]])
    x, y, z, r, scale = R.transform_sphere(mv, m["bounding_sphere"])
    n = len(x)
    vib = np.ones(n, dtype=bool)
    if op in (1, 2) and meshlet_occ:
        vib = ((mvis[rec["visibility_offset"] + lane // 32] >> (lane % 32).astype(np.uint32)) & 1).astype(bool)
    gated = vib if op == 1 else np.ones(n, dtype=bool)
    inside = gated & R.plane_test(ci, x, y, z, r)
    ax = (m["cone_axis"].astype(np.int32).astype(F) * R.RCP127).astype(F)
    axis = R.mat_vec(mv, ax[:, 0], ax[:, 1], ax[:, 2], np.zeros(n, F))
    cutoff = (m["cone_cutoff"].astype(np.int32).astype(F) * R.RCP127).astype(F)
    with np.errstate(all="ignore"):
        if int(ci["projection_type"]) == 1:  # camera_position = centre - (0, 0, -1)
            camx, camy, camz = (x - F(0)).astype(F), (y - F(0)).astype(F), (z - F(-1.0)).astype(F)
        else:
            camx = camy = camz = np.zeros(n, F)
        dx, dy, dz = (x - camx).astype(F), (y - camy).astype(F), (z - camz).astype(F)
        cone = R.dot3(dx, dy, dz, axis[0], axis[1], axis[2]) >= R.fma32(
            cutoff, np.sqrt(R.dot3(dx, dy, dz, dx, dy, dz), dtype=F), r)
    geo = inside & ~cone
    occ2 = op == 2 and meshlet_occ
    visible = geo.copy()
    if occ2:
        ov, _ = R.occlusion_test(ci, x, y, z, r, pyr, *pyr_size, m["bounding_sphere"][:, 3].astype(F), scale)
        visible = geo & ov
    bit = lambda a, flag: (np.where(a < 32, np.uint64(1) << np.minimum(a, 31).astype(np.uint64), np.uint64(0))  # noqa: E731
                           & np.uint64(int(flag))) != 0
    alpha = materials["alpha_mode"][m["material_index"]]
    allow, noskip = bit(alpha, ci["alpha_mode_flag"]), bit(alpha, ci["noskip_alphamode"])
    drawn = visible & allow
    early = np.zeros(n, dtype=bool)
    if occ2:  # :210-213: outside noskip_alphamode the alpha flag is not consulted
        drawn = np.where(noskip, drawn, visible & ~vib)
        early = visible & ~noskip & vib
    c = dict(meshlets=n, meshlet_skipped_prev_invisible=int((~gated).sum()),
             meshlet_frustum_culled=int((gated & ~inside).sum()), meshlet_cone_culled=int((inside & cone).sum()),
             meshlet_occlusion_culled=int((geo & ~visible).sum()),
             meshlet_alpha_filtered=int((visible & ~drawn & ~early).sum()),
             meshlet_drawn_in_early_pass=int(early.sum()), meshlet_drawn=int(drawn.sum()))
    return c, drawn


def classify(ci, draws, count, entity_draw_count, mesh_infos, entities, meshlets, materials, vis_words=None, mvis=None,
             pyr=None, pyr_size=(0, 0)):
    """Every counter of OrbitCullStats (engine.cull_stats_dict's keys), plus ("_records", "_meshlet_drawn")."""
    ce, records, _ = classify_entities(ci, draws, count, entity_draw_count, mesh_infos, entities, vis_words, pyr, pyr_size)
    cm, mdrawn = classify_meshlets(ci, records, meshlets, entities, materials, mvis, pyr, pyr_size)
    out = dict(ce, **cm)
    out["_records"], out["_meshlet_drawn"] = records, mdrawn
    return out


ENTITY_CLASSES = L.CULL_STATS_ENTITY[1:]
MESHLET_CLASSES = L.CULL_STATS_MESHLET[1:]


def check_invariants(c):
    """The sums include/orbit_abi_ext.h documents."""
    assert c["entities"] == sum(c[k] for k in ENTITY_CLASSES), c
    assert c["meshlets"] == sum(c[k] for k in MESHLET_CLASSES), c
    assert sum(c["lod_drawn"]) == c["entity_drawn"], c


def public(c):
    return {k: v for k, v in c.items() if not k.startswith("_")}


# ------------------------------------------------------------------------------------------------------- the scene set
# Shared by tests/test_cull_stats_cpu.py (classifier against np_restatement and the oracle, coverage of every counter)
# and tests/test_cull_stats_gpu.py (the product's counters against the classifier).
CASES = ["p0_persp_lods", "p0_ortho_cascade", "p1_persp", "p1_no_meshlet_occ", "p2_persp", "p2_persp_noskip",
         "p2_ortho", "p2_no_meshlet_occ", "p0_ragged_counts", "p0_all_alpha_no_planes"]


def make_case(name, oracle):
    """-> dict(scene, ci, count (in-buffer), edc (entity_draw_count), evis, mvis, pyr, psize)."""
    import scenes as sc

    rng = np.random.default_rng(sum(map(ord, name)))
    cam = sc.default_camera(rot=(0.8, 0.6))
    kw, evis, mvis, pyr, psize = {}, None, None, None, (0, 0)
    scene = sc.make_scene(31, 700, n_meshes=150, lods=3, meshlets_per_mesh=(1, 90), extent=(40.0, 10.0, 40.0))
    count = edc = scene.entity_draw_count
    if name == "p0_persp_lods":  # eight LODs spread over the scene: every lod_drawn slot
        scene = sc.make_scene(32, 900, n_meshes=200, lods=8, meshlets_per_mesh=(8, 120), extent=(60.0, 10.0, 60.0))
        count = edc = scene.entity_draw_count
        ci = sc.make_cull_info(cam.view, cam.planes, lod_base=8.0, lod_step=1.3)
    elif name == "p0_ortho_cascade":
        proj = sc.orthographic_rh(-25, 25, -25, 25, 0.1, 80.0)
        planes = np.concatenate([sc.frustum_planes(proj, 6), cam.planes[:3]])
        ci = sc.make_cull_info(sc.translation(0.0, 0.0, -40.0), planes, projection_type=1, lod_target=(1.0, 2.0, 3.0))
    elif name == "p0_ragged_counts":  # in-buffer count below entity_draw_count, and a count that is not a multiple of 256
        count, edc = 517, 600
        ci = sc.make_cull_info(cam.view, cam.planes, lod_base=4.0)
    elif name == "p0_all_alpha_no_planes":
        ci = sc.make_cull_info(cam.view, np.zeros((0, 4), np.float32), alpha_mode_flag=L.ALPHA_ALL)
    else:
        op = int(name[1])
        ortho = "ortho" in name
        evis = rng.integers(0, 2 ** 32, (count + 31) // 32, dtype=np.uint32)
        mvis = rng.integers(0, 2 ** 32, scene.vis_words, dtype=np.uint32)
        if ortho:
            proj = sc.orthographic_rh(-30, 30, -30, 30, 0.1, 90.0)
            view, planes = sc.translation(0.0, 0.0, -45.0), sc.frustum_planes(proj, 6)
            kw = dict(projection_type=1)
            if op == 2:
                kw.update(p00=2.0 / 60.0, p11=2.0 / 60.0, z_near=0.1, z_far=90.0)
        else:
            view, planes = cam.view, cam.planes
            if op == 2:
                kw = dict(p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
        if "noskip" in name:
            kw["noskip_alphamode"] = L.ALPHA_MASKED | L.ALPHA_TRANSPARENT  # transparent: not in alpha_mode_flag
        if op == 2:
            W, H = 320, 180
            if ortho:
                depth = np.full((H, W), 0.5, dtype=np.float32)
                depth[:, : W // 2] = 0.9
            else:
                depth = sc.make_depth(9, W, H, cam)
            pyr, d = oracle.depth_reduce(depth, W, H)
            psize = (d.width, d.height)
        ci = sc.make_cull_info(view, planes, occlusion_pass=op, meshlet_visibility="no_meshlet_occ" not in name,
                               lod_base=6.0, **kw)
        if "no_meshlet_occ" in name:
            mvis = None
    return dict(scene=scene, ci=ci, count=count, edc=edc, evis=evis, mvis=mvis, pyr=pyr, psize=psize)


def classify_case(c):
    s = c["scene"]
    return classify(c["ci"], s.entity_draws, c["count"], c["edc"], s.mesh_infos, s.entities, s.meshlets, s.materials,
                    c["evis"], c["mvis"], c["pyr"], c["psize"])
