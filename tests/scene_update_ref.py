"""Inputs and an independent restatement for orbit_scene_update_entities (include/orbit_abi_ext.h).

`entity_rows` restates EntityData::entity_gpu_data (src/scene.rs:75-82; the host mirror's orbit_scene.cpp) in numpy
float32, product by product in the host's association: mat4_from_quat, the scale of columns 0..2, the cofactor
inverse with the affine matrix's zero terms kept, det, rdet = 1 / det, inv * rdet, transpose, identity outside the
upper 3x3.  numpy float32 arithmetic is IEEE binary32 with no contraction and keeps denormals.
"""
import numpy as np

from orbit_amd import layouts as L
from orbit_amd import scene as S

F = np.float32


def edge_transforms(seed, n):
    """n transforms: random ones mixed with non-uniform, negative, tiny (1e-20), huge (1e20) and zero scales,
    unnormalised quaternions, -0.0 and denormal components."""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=L.ENTITY_TRANSFORM)
    t["position"] = rng.uniform(-100, 100, (n, 3))
    q = rng.normal(size=(n, 4))
    t["orientation"] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.choice([1.0, 1.0, 0.5, 3.0], (n, 1))
    t["scale"] = rng.uniform(0.1, 4.0, (n, 3)) * rng.choice([1.0, -1.0], (n, 3))
    special = np.array([0.0, -0.0, 1e-20, -1e-20, 1e20, -1e20, 1e-40, -1e-40, 1.0, -1.0, 2.5], dtype=F)
    pick = rng.random(n) < 0.5  # half of the entities get special values in some components
    for field, width in (("position", 3), ("orientation", 4), ("scale", 3)):
        m = pick[:, None] & (rng.random((n, width)) < 0.35)
        vals = rng.choice(special, (n, width))
        col = t[field]
        col[m] = vals[m]
        t[field] = col
    if n > 4:  # a few whole rows of the corner cases
        t[0] = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), (1.0, 1.0, 1.0))
        t[1] = ((-0.0, -0.0, -0.0), (-0.0, -0.0, -0.0, -1.0), (0.0, 0.0, 0.0))
        t[2] = ((1e-40, -1e-40, 1e-41), (1e-40, 0.0, 0.0, 1.0), (1e-20, 1e-20, 1e-20))
        t[3] = ((1e20, -1e20, 0.0), (0.0, 0.0, 0.0, 0.0), (1e20, 1e-20, -1e20))
    return t


def entity_rows(t):
    """ENTITY_DATA rows of ENTITY_TRANSFORM rows."""
    t = np.ascontiguousarray(t, dtype=L.ENTITY_TRANSFORM)
    px, py, pz = (t["position"][:, k] for k in range(3))
    qx, qy, qz, qw = (t["orientation"][:, k] for k in range(4))
    sx, sy, sz = (t["scale"][:, k] for k in range(3))
    n = len(t)
    one, zero = np.ones(n, F), np.zeros(n, F)
    with np.errstate(all="ignore"):
        x2, y2, z2 = qx + qx, qy + qy, qz + qz
        xx, xy, xz, yy, yz, zz = qx * x2, qx * y2, qx * z2, qy * y2, qy * z2, qz * z2
        wx, wy, wz = qw * x2, qw * y2, qw * z2
        m = [(one - (yy + zz)) * sx, (xy + wz) * sx, (xz - wy) * sx, zero,
             (xy - wz) * sy, (one - (xx + zz)) * sy, (yz + wx) * sy, zero,
             (xz + wy) * sz, (yz - wx) * sz, (one - (xx + yy)) * sz, zero,
             px, py, pz, one]
        inv = {}
        inv[0] = (m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] +
                  m[13] * m[6] * m[11] - m[13] * m[7] * m[10])
        inv[4] = (-m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] -
                  m[12] * m[6] * m[11] + m[12] * m[7] * m[10])
        inv[8] = (m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] +
                  m[12] * m[5] * m[11] - m[12] * m[7] * m[9])
        inv[12] = (-m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] -
                   m[12] * m[5] * m[10] + m[12] * m[6] * m[9])
        inv[1] = (-m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] -
                  m[13] * m[2] * m[11] + m[13] * m[3] * m[10])
        inv[5] = (m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] +
                  m[12] * m[2] * m[11] - m[12] * m[3] * m[10])
        inv[9] = (-m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] -
                  m[12] * m[1] * m[11] + m[12] * m[3] * m[9])
        inv[2] = (m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] +
                  m[13] * m[2] * m[7] - m[13] * m[3] * m[6])
        inv[6] = (-m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] -
                  m[12] * m[2] * m[7] + m[12] * m[3] * m[6])
        inv[10] = (m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] +
                   m[12] * m[1] * m[7] - m[12] * m[3] * m[5])
        det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12]
        rdet = one / det
        normal = [inv[0] * rdet, inv[4] * rdet, inv[8] * rdet, zero,
                  inv[1] * rdet, inv[5] * rdet, inv[9] * rdet, zero,
                  inv[2] * rdet, inv[6] * rdet, inv[10] * rdet, zero,
                  zero, zero, zero, one]
    out = np.zeros(n, dtype=L.ENTITY_DATA)
    out["model_matrix"] = np.stack(m, axis=1).astype(F)
    out["normal_matrix"] = np.stack(normal, axis=1).astype(F)
    return out


ONE_MESH = np.zeros(1, dtype=L.MESH_INFO)
ONE_MESH["lod_count"] = 1
ONE_MESH["mesh_lods"][0, 0] = (0, 1)  # one meshlet: one visibility word per entity


def host_rows(t):
    """The host mirror's update_scene entity_data for one drawn entity per transform (instance i = transform i)."""
    sd = S.SceneData()
    for r in np.ascontiguousarray(t, dtype=L.ENTITY_TRANSFORM):
        sd.add_entity(position=r["position"], orientation=r["orientation"], scale=r["scale"], mesh=0)
    sd.update_scene(ONE_MESH)
    return sd.entity_data_cache()


def assert_rows_equal(got, want):
    """Every non-NaN lane bit-exact; NaN lanes only NaN in both (x86's default NaN has its sign bit set, the GPU's
    does not)."""
    g = np.ascontiguousarray(got).view(np.float32).reshape(-1)
    w = np.ascontiguousarray(want).view(np.float32).reshape(-1)
    assert g.shape == w.shape
    gn, wn = np.isnan(g), np.isnan(w)
    if not np.array_equal(gn, wn):
        k = np.flatnonzero(gn != wn)[0]
        raise AssertionError(f"NaN lanes differ at floats {np.flatnonzero(gn != wn)[:8]}; row {k // 32}: "
                             f"{g[k // 32 * 32:k // 32 * 32 + 32].tolist()} vs {w[k // 32 * 32:k // 32 * 32 + 32].tolist()}")
    diff = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)) & ~wn)
    assert diff.size == 0, (f"{diff.size} lanes differ, first at float {diff[0]} (row {diff[0] // 32}): "
                            f"{g[diff[0]]!r} vs {w[diff[0]]!r}")
