"""The per-block pre-test of the pass-0 evaluation (orbit_amd/csrc/block_pretest.h, exported by liborbit_host) against the
oracle, on the host: a "certain" verdict must never contradict what oracle_meshlet_cull decides for that meshlet, and a
derived bound must contain every meshlet of its block in float64.

A case is one dispatch record of 32 meshlets with its own entity; the view matrix is the identity, so the (view x model)
product the evaluation's slab holds is the model matrix bit for bit, and `scale` is the slab's: sqrtf of the largest of
the three column sums ((x x + y y) + z z), in binary32."""
import ctypes as C

import numpy as np
import pytest

import scenes as sc
from orbit_amd import layouts as L
from orbit_amd.passes import lib as host_lib

F = np.float32
PER = 32


def _host():
    h = host_lib()
    h.orbit_host_block_pretest.restype = C.c_uint32
    h.orbit_host_block_pretest.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float,
                                           C.c_void_p, C.c_uint64, C.c_void_p]
    h.orbit_host_block_bounds.restype = None
    h.orbit_host_block_bounds.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return h


BOUND = np.dtype([("c", "<f4", (3,)), ("packed", "<u4"), ("rc", "<f4"), ("r_max", "<f4"), ("valid", "<u4"), ("pad", "<u4")])


def bounds_of(spheres):
    spheres = np.ascontiguousarray(spheres, dtype=F).reshape(-1, 4)
    out = np.zeros((len(spheres) + PER - 1) // PER, dtype=BOUND)
    _host().orbit_host_block_bounds(spheres.ctypes.data, len(spheres), out.ctypes.data)
    return out


def slab_scale(m):
    """setup_write's largest_scale_from_matrix of column-major matrices m[n, 16], in binary32."""
    m = m.astype(F)
    d = [(m[:, 4 * c] * m[:, 4 * c] + m[:, 4 * c + 1] * m[:, 4 * c + 1]).astype(F) + m[:, 4 * c + 2] * m[:, 4 * c + 2] for c in range(3)]
    return np.sqrt(np.maximum(np.maximum(d[0], d[1]), d[2]).astype(F)).astype(F)


def pretest(models, spheres, cones, planes, ratio):
    """-> verdicts[n_records, 32], flags[n_records] of records i = meshlets [32 i, 32 i + 32) under models[i]."""
    h = _host()
    n = len(models)
    bnd = bounds_of(spheres)
    scale = slab_scale(models)
    planes = np.ascontiguousarray(planes, dtype=F).reshape(-1, 4)
    cones = np.ascontiguousarray(cones, dtype=np.uint32).reshape(n, PER)
    out = np.zeros((n, PER), dtype=np.uint8)
    flags = np.zeros(n, dtype=np.uint32)
    models = np.ascontiguousarray(models, dtype=F)
    for i in range(n):
        flags[i] = h.orbit_host_block_pretest(models[i].ctypes.data, 1, float(scale[i]), bnd[i:i + 1].ctypes.data,
                                              planes.ctypes.data, len(planes), ratio, cones[i].ctypes.data, PER,
                                              out[i].ctypes.data)
    return out, flags, bnd


def oracle_visible(oracle, models, spheres, cones, planes):
    """The set of meshlets oracle_meshlet_cull draws, as a boolean per meshlet."""
    n = len(models)
    ent = np.zeros(n, dtype=L.ENTITY_DATA)
    ent["model_matrix"] = models
    ent["normal_matrix"] = np.eye(4, dtype=F).reshape(-1)
    ml = np.zeros(n * PER, dtype=L.MESHLET)
    ml["bounding_sphere"] = np.asarray(spheres, dtype=F).reshape(-1, 4)
    cw = np.ascontiguousarray(cones, dtype=np.uint32).reshape(-1)
    ml["cone_axis"] = np.stack([(cw >> (8 * k)) & 0xFF for k in range(3)], axis=1).astype(np.uint8).view(np.int8)
    ml["cone_cutoff"] = (cw >> 24).astype(np.uint8).view(np.int8)
    ml["vertex_count"], ml["triangle_count"] = 3, 1
    mat = np.zeros(1, dtype=L.MATERIAL)
    disp = np.zeros(L.DISPATCH_HEADER + 16 * n, dtype=np.uint8)
    disp[:12].view("<u4")[:] = (n, 1, 1)
    rec = disp[L.DISPATCH_HEADER:].view(L.MESHLET_DISPATCH)
    rec["entity_index"] = np.arange(n)
    rec["meshlet_offset"] = np.arange(n) * PER
    rec["meshlet_count"] = PER
    ci = sc.make_cull_info(np.eye(4, dtype=F), planes, occlusion_pass=0, alpha_mode_flag=L.ALPHA_ALL)
    out, _, dropped = oracle.meshlet_cull(ci, disp, ml, n * PER, ent, mat)
    assert dropped == 0
    count = int(out[:4].view("<u4")[0])
    cmds = out[L.DRAW_HEADER:L.DRAW_HEADER + 28 * count].view(L.MESHLET_DRAW_COMMAND)
    vis = np.zeros(n * PER, dtype=bool)
    vis[cmds["meshlet_index"]] = True
    return vis.reshape(n, PER)


def check(oracle, models, spheres, cones, planes, ratio):
    """No certain verdict contradicts the oracle, without planes (the cone verdicts alone) and with them."""
    v, flags, _ = pretest(models, spheres, cones, planes, ratio)
    cone_only = oracle_visible(oracle, models, spheres, cones, np.zeros((0, 4), dtype=F))
    with_planes = oracle_visible(oracle, models, spheres, cones, planes)
    culled, kept, inside = (v & 3) == 1, (v & 3) == 2, (v & 4) != 0
    assert not (culled & cone_only).any(), "certainly culled, but the oracle's cone test keeps it"
    assert not (kept & ~cone_only).any(), "certainly kept, but the oracle's cone test culls it"
    assert not (kept & inside & ~with_planes).any(), "certainly kept and inside, but the oracle does not draw it"
    assert not (culled & with_planes).any()
    return v, flags


def random_models(rng, n):
    """Affine matrices: rotations with uniform scale, non-uniform scale, shear, mirrored; the translation comes later."""
    q = rng.normal(size=(n, 3, 3))
    rot = np.linalg.qr(q)[0]
    kind = rng.integers(0, 4, size=n)
    s = np.exp(rng.uniform(np.log(0.05), np.log(20.0), size=(n, 3)))
    s[kind == 0] = s[kind == 0][:, :1]                       # uniform
    lin = rot * s[:, None, :]                                # columns scaled
    shear = np.eye(3)[None].repeat(n, 0)
    shear[:, 0, 1] = np.where(kind == 2, rng.uniform(-2, 2, size=n), 0.0)
    shear[:, 1, 2] = np.where(kind == 2, rng.uniform(-2, 2, size=n), 0.0)
    lin = lin @ shear
    lin[kind == 3, :, 0] *= -1.0                             # mirrored
    m = np.zeros((n, 4, 4))
    m[:, :3, :3] = lin
    m[:, 3, 3] = 1.0
    return m


def place(rng, m, centre, dist):
    """Sets the translation so that the block's centre lands `dist` from the camera in a random direction."""
    n = len(m)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m[:, :3, 3] = d * dist[:, None] - np.einsum("nij,nj->ni", m[:, :3, :3], centre)
    return np.ascontiguousarray(m.transpose(0, 2, 1).reshape(n, 16)).astype(F)  # column-major


def random_cones(rng, n):
    c = rng.integers(-128, 128, size=(n, PER, 4))
    edge = rng.random(size=(n, PER)) < 0.05
    c[edge, :3] = rng.choice([-127, 127], size=(int(edge.sum()), 3))
    c[..., 3][rng.random(size=(n, PER)) < 0.05] = rng.choice([-128, -127, 0, 127])
    b = (c & 0xFF).astype(np.uint32)
    return b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16 | b[..., 3] << 24


def frustum():
    cam = sc.default_camera(position=(0.0, 0.0, 0.0))
    return cam.planes


@pytest.mark.parametrize("ratio", [-1.0, 1.0])
def test_random_records_never_contradict_the_oracle(oracle, ratio):
    rng = np.random.default_rng(20260 + int(ratio))
    n = 32768  # x 32 meshlets: 1 048 576 cases
    m = random_models(rng, n)
    centre = rng.uniform(-50, 50, size=(n, 3))
    spread = np.exp(rng.uniform(np.log(1e-3), np.log(20.0), size=n))
    c = centre[:, None, :] + rng.uniform(-1, 1, size=(n, PER, 3)) * spread[:, None, None]
    r = rng.uniform(0, 3, size=(n, PER)) * (rng.random(size=(n, 1)) < 0.8)  # a fifth of the blocks: radius 0
    spheres = np.concatenate([c, r[..., None]], axis=2).astype(F)
    sigma = np.linalg.norm(m[:, :3, :3], ord=2, axis=(1, 2))
    # from barely above the block's view-space radius to far away
    dist = sigma * spread * np.sqrt(3.0) * np.exp(rng.uniform(np.log(1.02), np.log(2000.0), size=n))
    models = place(rng, m, centre, dist)
    v, flags = check(oracle, models, spheres, random_cones(rng, n), frustum(), ratio)
    sparse = (flags & 1) != 0
    assert sparse.mean() > 0.3 and ((v & 3) != 0).mean() > 0.2, "the generator must exercise the certain verdicts"
    print(f"ratio {ratio}: {sparse.mean():.3f} of the records sparse, verdicts culled / kept / open of their lanes: "
          f"{((v[sparse] & 3) == 1).mean():.3f} / {((v[sparse] & 3) == 2).mean():.3f} / {((v[sparse] & 3) == 0).mean():.3f}")


def test_knife_edge_records_never_contradict_the_oracle(oracle):
    """Blocks of 32 copies of one meshlet whose cone quantity S = p . L a - cutoff |p| - r is zero to within rounding, one
    coordinate of the centre scanned ulp by ulp: the block's radius is a few ulps, so the band around zero is almost only
    the rounding margin — which is what these cases hold to account."""
    rng = np.random.default_rng(77)
    n = 4096
    m = random_models(rng, n)
    centre = rng.uniform(-50, 50, size=(n, 3))
    dist = np.exp(rng.uniform(np.log(0.5), np.log(3000.0), size=n))
    models = place(rng, m, centre, dist)
    cones_i = rng.integers(-127, 128, size=(n, 4))
    cones_i[: n // 8, :3] = rng.choice([-127, 127], size=(n // 8, 3))
    cones_i[n // 8: n // 4, 3] = rng.choice([-128, 127], size=n // 8)
    radius = np.where(rng.random(size=n) < 0.5, 0.0, rng.uniform(0, 2, size=n)).astype(F)
    kf = np.float64(np.frombuffer(np.uint32(0x3C010204).tobytes(), dtype=F)[0])
    M = models.astype(np.float64).reshape(n, 4, 4).transpose(0, 2, 1)
    scale = slab_scale(models).astype(np.float64)
    a = (cones_i[:, :3].astype(F) * F(kf)).astype(np.float64)
    cutoff = np.float64((cones_i[:, 3].astype(F) * F(kf)))

    def S(c):
        p = np.einsum("nij,nj->ni", M[:, :3, :3], c) + M[:, :3, 3]
        ax = np.einsum("nij,nj->ni", M[:, :3, :3], a)
        return (p * ax).sum(1) - cutoff * np.linalg.norm(p, axis=1) - radius * scale

    # bisect along x through the centre for a zero of S (where there is a sign change within +-100)
    lo, hi = centre.copy(), centre.copy()
    lo[:, 0] -= 100.0
    hi[:, 0] += 100.0
    ok = np.sign(S(lo)) != np.sign(S(hi))
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        left = np.sign(S(mid)) != np.sign(S(hi))
        lo = np.where(left[:, None], mid, lo)
        hi = np.where(left[:, None], hi, mid)
    assert ok.mean() > 0.3
    root = (0.5 * (lo + hi)).astype(F)
    # block j sits 0, +-1, +-2, +-4 ... +-2^15 ulps from the root and scans 32 ulps there: near the root the lanes straddle
    # the oracle's flip (and must stay open), further out the block's radius (16 ulps) is small against its offset and
    # the verdicts become certain — on both sides, at offsets that are a small multiple of the margin
    j = np.arange(n)
    offset = np.where(j % 17 == 0, 0, (1 << ((j % 17) - 1).clip(0)) * np.where((j // 17) % 2 == 0, 1, -1))
    steps = offset[:, None] + np.arange(PER)[None, :] - PER // 2
    x = (root[:, 0].view(np.int32)[:, None] + np.where(root[:, :1] >= 0, steps, -steps)).astype(np.int32).view(F)
    assert np.isfinite(x).all() and (np.sign(x) == np.sign(root[:, :1])).all()
    c = np.repeat(root[:, None, :], PER, axis=1)
    c[:, :, 0] = x
    spheres = np.concatenate([c, np.repeat(radius[:, None, None], PER, axis=1)], axis=2).astype(F)
    b = (cones_i & 0xFF).astype(np.uint32)
    cw = np.repeat((b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16 | b[:, 3] << 24)[:, None], PER, axis=1)
    sel = np.flatnonzero(ok)
    v, flags = check(oracle, models[sel], spheres[sel], cw[sel], frustum(), 1.0)
    vis = oracle_visible(oracle, models[sel], spheres[sel], cw[sel], np.zeros((0, 4), dtype=F))
    straddle = vis.any(axis=1) & ~vis.all(axis=1)
    assert straddle.sum() > 100, "the scans must cross the oracle's own decision"
    assert ((flags & 1) != 0).mean() > 0.5
    # ... and the assertion above is not empty: whole blocks certainly culled and certainly kept, within 2^15 ulps of a root
    off = np.abs(offset[sel])
    culled, kept = ((v & 3) == 1).all(axis=1), ((v & 3) == 2).all(axis=1)
    assert (culled & (off <= 1 << 15)).sum() > 50 and (kept & (off <= 1 << 15)).sum() > 50
    assert not ((v[straddle] & 3) != 0).any(), "a block that straddles the oracle's flip has no certain lane"
    first = {k: int(off[m].min()) for k, m in (("culled", culled), ("kept", kept))}
    print(f"knife edge: nearest certain blocks at {first} ulps from the root; {straddle.sum()} blocks straddle the flip")


def test_non_finite_and_negative_blocks_are_not_valid():
    s = np.zeros((6 * PER, 4), dtype=F)
    s[:, :3] = np.random.default_rng(3).uniform(-5, 5, size=(6 * PER, 3))
    s[:, 3] = 1.0
    s[1 * PER + 7, 1] = np.inf
    s[2 * PER + 31, 0] = np.nan
    s[3 * PER + 0, 3] = -0.5
    s[4 * PER + 3, 3] = np.nan
    b = bounds_of(s)
    assert list(b["valid"]) == [1, 0, 0, 0, 0, 1] and all(b["packed"][1:5] == 0) and b["packed"][0] != 0
    # a projective matrix, or one the slab does not flag as affine, keeps the record dense
    v = np.zeros(PER, dtype=np.uint8)
    cones = np.zeros(PER, dtype=np.uint32)
    m = np.eye(4, dtype=F).reshape(-1).copy()
    m[14] = -500.0
    h = _host()
    pl = np.zeros((1, 4), dtype=F)
    assert h.orbit_host_block_pretest(m.ctypes.data, 1, 1.0, b[0:1].ctypes.data, pl.ctypes.data, 0, -1.0, cones.ctypes.data, PER, v.ctypes.data) & 1
    assert h.orbit_host_block_pretest(m.ctypes.data, 0, 1.0, b[0:1].ctypes.data, pl.ctypes.data, 0, -1.0, cones.ctypes.data, PER, v.ctypes.data) == 0
    assert h.orbit_host_block_pretest(m.ctypes.data, 1, 1.0, b[1:2].ctypes.data, pl.ctypes.data, 0, -1.0, cones.ctypes.data, PER, v.ctypes.data) == 0
    m[12] = np.inf
    assert h.orbit_host_block_pretest(m.ctypes.data, 1, 1.0, b[0:1].ctypes.data, pl.ctypes.data, 0, -1.0, cones.ctypes.data, PER, v.ctypes.data) == 0


def test_bounds_contain_their_meshlets_in_float64():
    rng = np.random.default_rng(11)
    n = 20000
    scale = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), size=(n, 1, 1)))
    c = (rng.uniform(-1, 1, size=(n, 1, 3)) * 10 + rng.uniform(-1, 1, size=(n, PER, 3))) * scale
    r = rng.uniform(0, 1, size=(n, PER, 1)) * scale
    s = np.concatenate([c, r], axis=2).astype(F)
    b = bounds_of(s.reshape(-1, 4))
    assert b["valid"].all()
    d = np.linalg.norm(s[:, :, :3].astype(np.float64) - b["c"].astype(np.float64)[:, None, :], axis=2)
    assert (d <= b["rc"].astype(np.float64)[:, None]).all()
    assert (s[:, :, 3] <= b["r_max"][:, None]).all()
    # ... and so do the rounded-up halves the evaluation reads, which are at most 2^-7 above
    rc16 = (b["packed"] & 0xFFFF0000).view(F)
    rm16 = (b["packed"] << 16).view(F)
    assert (rc16 >= b["rc"]).all() and (rc16 <= b["rc"] * F(1 + 2.0 ** -7)).all()
    assert (rm16 >= b["r_max"]).all() and (rm16 <= b["r_max"] * F(1 + 2.0 ** -7) + F(1e-38)).all()


def test_candidate_share_of_the_config5_generator(oracle):
    """Prints the share of lanes the pre-test leaves open on bench.py's scene generator at 2 000 entities (its camera and
    planes), and holds the verdicts against the oracle there too."""
    torch = pytest.importorskip("torch")
    from orbit_amd import camera, synth

    dev = torch.device("cpu")
    spec = synth.C5Spec(entities=2000, meshlets_per_entity=256)
    _, _, ent, half = synth.gen_entity_tables(spec, dev)
    mlt = synth.gen_meshlets(spec, 0, spec.entities, dev, half)
    ml = mlt.numpy().view(np.uint8).reshape(-1).view(L.MESHLET)
    ci = np.frombuffer(bytes(camera.frame_cull_info((0.0, 0.0, 1300.0))), dtype=L.GPU_CULL_INFO)[0]
    e = ent.numpy().view(np.uint8).reshape(-1).view(L.ENTITY_DATA)
    view = ci["view_matrix"].reshape(4, 4).T.astype(F)
    per_entity = spec.meshlets_per_entity // PER
    n = spec.entities * per_entity
    # the slab's (view x model) in binary32, term by term as mat4_mul_col sums it
    model = e["model_matrix"].reshape(-1, 4, 4).transpose(0, 2, 1).astype(F)
    vm = np.zeros_like(model)
    for k in range(4):
        vm = (vm + view[None, :, k, None] * model[:, None, k, :]).astype(F)
    models = np.repeat(np.ascontiguousarray(vm.transpose(0, 2, 1)).reshape(-1, 16), per_entity, axis=0)
    cones = (ml["cone_axis"].view(np.uint8).astype(np.uint32) * np.array([1, 1 << 8, 1 << 16], dtype=np.uint32)).sum(1).astype(np.uint32) | ml["cone_cutoff"].view(np.uint8).astype(np.uint32) << 24
    planes = ci["cull_planes"][:int(ci["cull_plane_count"])]
    v, flags, _ = pretest(models, ml["bounding_sphere"], cones, planes, -1.0)
    sparse = (flags & 1) != 0
    open_lanes = ((v & 3) == 0) | (((v & 3) == 2) & ((v & 4) == 0))
    print(f"config 5 at 2000 entities: {sparse.mean():.4f} of the records sparse, {(flags & 2).astype(bool).mean():.4f} inside "
          f"every plane; candidates {open_lanes[sparse].mean():.4f} of the sparse records' lanes "
          f"(cone verdict open: {((v[sparse] & 3) == 0).mean():.4f})")
    assert n == len(models)
