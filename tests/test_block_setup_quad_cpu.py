"""The per-block evaluation derives a record's BlockRecord on four lanes (orbit_amd/csrc/block_pretest.h
block_record_setup_quad, the host's form of meshlet_eval_blocks.hip blk_setup) from plane norms computed once
(block_plane_norm): both must give block_record_setup's 32 bytes, bit for bit, for every input — every value is computed
by the same expression tree, only by another lane.  liborbit_host exports both forms (orbit_host_block_record).

Records come from the generators of tests/test_block_pretest_cpu.py (random_models, place: rotations, non-uniform scale,
shear, mirrors, from barely outside the block to far away).  Its knife-edge scan lives inside its test, so the knife
edges of THIS code are built here the same way (blocks a few ulps wide around one centre): a centre within ulps of a cull
plane, where `inside` flips, and a ratio at D / Rc', where `sparse` flips."""
import ctypes as C

import numpy as np
import pytest

from orbit_amd.passes import lib as host_lib
from test_block_pretest_cpu import BOUND, F, PER, bounds_of, frustum, place, random_models, slab_scale

RECORD = np.dtype([("g", "<f4", (3,)), ("dk", "<f4"), ("sigma", "<f4"), ("bk", "<f4"), ("rr", "<f4"), ("flags", "<u4")])
PLANE_COUNTS = (0, 1, 3, 4, 5, 6, 8, 12)


def _host():
    h = host_lib()
    h.orbit_host_block_record.restype = None
    h.orbit_host_block_record.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float,
                                          C.c_int32, C.c_void_p]
    h.orbit_host_block_plane_norm.restype = C.c_float
    h.orbit_host_block_plane_norm.argtypes = [C.c_float, C.c_float, C.c_float]
    return h


def records(models, affine, scale, bnd, planes, ratio, quad):
    """-> RECORD[n]: record i from models[i] (column-major), affine[i], scale[i], bnd[i] and the same planes."""
    h = _host()
    models = np.ascontiguousarray(models, dtype=F)
    planes = np.ascontiguousarray(planes, dtype=F).reshape(-1, 4)
    out = np.zeros(len(models), dtype=RECORD)
    for i in range(len(models)):
        h.orbit_host_block_record(models[i].ctypes.data, int(affine[i]), float(scale[i]), bnd[i:i + 1].ctypes.data,
                                  planes.ctypes.data, len(planes), ratio, quad, out[i:i + 1].ctypes.data)
    return out


def both_forms(models, affine, scale, bnd, planes, ratio, payloads=True):
    """Asserts the two forms equal in all 32 bytes; -> the records.  payloads=False (records whose inputs hold two
    DIFFERENT NaNs, nothing else): a NaN equals a NaN in the same place — which operand's payload an operation on two NaNs
    returns is the instruction's operand order, which a compiler may swap within one source expression."""
    a = records(models, affine, scale, bnd, planes, ratio, 0)
    b = records(models, affine, scale, bnd, planes, ratio, 1)
    ne = a.view(np.uint32).reshape(-1, 8) != b.view(np.uint32).reshape(-1, 8)
    if not payloads:
        ne[:, :7] &= ~(np.isnan(a.view(F).reshape(-1, 8)[:, :7]) & np.isnan(b.view(F).reshape(-1, 8)[:, :7]))
    diff = np.flatnonzero(ne.any(1))
    assert len(diff) == 0, f"{len(diff)} records differ, the first: {a[diff[0]]} against {b[diff[0]]} (record {diff[0]})"
    return a


def planes_through(rng, n, reach=60.0, first=None):
    """The five frustum planes (or `first`), then planes that cut through the records' positions: unit and far-from-unit
    normals, offsets of either sign, one plane with a zero normal."""
    extra = rng.normal(size=(12, 4))
    extra[:, :3] *= np.exp(rng.uniform(np.log(1e-3), np.log(1e3), size=(12, 1)))
    extra[:, 3] = rng.uniform(-reach, reach, size=12) * np.linalg.norm(extra[:, :3], axis=1)
    extra[4, :3] = 0.0
    return np.concatenate([frustum() if first is None else first, extra.astype(F)])[:n].astype(F)


def random_case(rng, n):
    m = random_models(rng, n)
    centre = rng.uniform(-50, 50, size=(n, 3))
    spread = np.exp(rng.uniform(np.log(1e-3), np.log(20.0), size=n))
    c = centre[:, None, :] + rng.uniform(-1, 1, size=(n, PER, 3)) * spread[:, None, None]
    r = rng.uniform(0, 3, size=(n, PER)) * (rng.random(size=(n, 1)) < 0.8)
    spheres = np.concatenate([c, r[..., None]], axis=2).astype(F)
    sigma = np.linalg.norm(m[:, :3, :3], ord=2, axis=(1, 2))
    dist = sigma * spread * np.sqrt(3.0) * np.exp(rng.uniform(np.log(1.02), np.log(2000.0), size=n))
    models = place(rng, m, centre, dist)
    return models, bounds_of(spheres)


@pytest.mark.parametrize("n_planes", PLANE_COUNTS)
def test_random_records(n_planes):
    rng = np.random.default_rng(500 + n_planes)
    n = 4096
    models, bnd = random_case(rng, n)
    planes = planes_through(rng, n_planes)
    seen = np.zeros(4, dtype=int)
    for ratio in (-1.0, 0.0, 1.0, 100.0):
        r = both_forms(models, np.ones(n, dtype=bool), slab_scale(models), bnd, planes, ratio)
        seen += np.bincount(r["flags"], minlength=4)
    assert seen[0] > 100 and seen[1] + seen[3] > 100, "dense and sparse records"
    assert seen[2] == 0, "inside without sparse"
    if n_planes == 0:
        assert seen[1] == 0, "without planes every sparse record is inside"
    elif n_planes <= 5:
        assert seen[1] > 20 and seen[3] > 20, "sparse records on both sides of the planes"


def icosahedron_planes(n, distance, rng=None):
    """n <= 12 planes tangent to the sphere of radius `distance` around the origin, inside towards it, their normals the
    vertices of an icosahedron (63 degrees apart or more: a point just outside one of them is well inside all the
    others), each scaled by its own factor if `rng` is given."""
    phi = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([(0, s1, s2 * phi) for s1 in (1, -1) for s2 in (1, -1)], dtype=np.float64)
    v = np.concatenate([v, np.roll(v, 1, axis=1), np.roll(v, 2, axis=1)])
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    k = np.ones(12) if rng is None else np.exp(rng.uniform(np.log(0.01), np.log(100.0), size=12))
    return np.concatenate([-v * k[:, None], (distance * k)[:, None]], axis=1)[:n].astype(F)


@pytest.mark.parametrize("n_planes", (1, 4, 5, 6, 12))
def test_every_plane_index_decides_alone(n_planes):
    """For every plane i < n some record is sparse and fails `inside` because of plane i alone — in both forms, so the
    plane-to-lane map and the AND over the quad's four lanes are held to account plane by plane.  (No frustum here: what
    is behind its near plane is outside its side planes too.)  Record r is a small block 5 to 30 % beyond plane r % n."""
    rng = np.random.default_rng(600 + n_planes)
    n = 64 * n_planes
    planes = icosahedron_planes(n_planes, 100.0, rng)
    m = random_models(rng, n)
    centre = rng.uniform(-50, 50, size=(n, 3))
    spread = np.exp(rng.uniform(np.log(1e-3), np.log(0.05), size=n))
    c = centre[:, None, :] + rng.uniform(-1, 1, size=(n, PER, 3)) * spread[:, None, None]
    spheres = np.concatenate([c, rng.uniform(0, 1, size=(n, PER, 1))], axis=2).astype(F)
    unit = planes[:, :3].astype(np.float64) / np.linalg.norm(planes[:, :3].astype(np.float64), axis=1, keepdims=True)
    target = -unit[np.arange(n) % n_planes] * rng.uniform(105.0, 130.0, size=(n, 1))
    m[:, :3, 3] = target - np.einsum("nij,nj->ni", m[:, :3, :3], centre)
    models = np.ascontiguousarray(m.transpose(0, 2, 1).reshape(n, 16)).astype(F)
    bnd = bounds_of(spheres)
    aff, scale = np.ones(n, dtype=bool), slab_scale(models)
    full = both_forms(models, aff, scale, bnd, planes, -1.0)
    alone = np.stack([(both_forms(models, aff, scale, bnd, planes[i:i + 1], -1.0)["flags"] & 2) != 0 for i in range(n_planes)])
    sparse = (full["flags"] & 1) != 0
    assert sparse.all()
    assert np.array_equal((full["flags"] & 2) != 0, sparse & alone.all(0))
    for i in range(n_planes):
        others = np.delete(alone, i, axis=0).all(0)
        assert (sparse & ~alone[i] & others).sum() >= 32, f"too few sparse records outside plane {i} alone"


def test_knife_edges_of_the_planes_and_of_the_ratio():
    """Blocks a few ulps wide whose centre's view-space x is scanned ulp by ulp across the plane x = x0 (dist against
    margin), and ratios scanned ulp by ulp across D / Rc' of each record (the sparse predicate)."""
    rng = np.random.default_rng(71)
    n = 2048
    m = random_models(rng, n)
    centre = rng.uniform(-50, 50, size=(n, 3))
    models = place(rng, m, centre, np.exp(rng.uniform(np.log(5.0), np.log(3000.0), size=n)))
    c32 = centre.astype(F)
    ulps = (np.arange(PER) - PER // 2)[None, :]
    x = (c32[:, 0].view(np.int32)[:, None] + np.where(c32[:, :1] >= 0, ulps, -ulps)).astype(np.int32).view(F)
    c = np.repeat(c32[:, None, :], PER, axis=1)
    c[:, :, 0] = x
    radius = np.where(rng.random(size=n) < 0.5, 0.0, rng.uniform(0, 2, size=n)).astype(F)
    spheres = np.concatenate([c, np.repeat(radius[:, None, None], PER, axis=1)], axis=2).astype(F)
    bnd = bounds_of(spheres)
    aff, scale = np.ones(n, dtype=bool), slab_scale(models)
    base = both_forms(models, aff, scale, bnd, np.zeros((0, 4), dtype=F), 1.0)
    sparse = (base["flags"] & 1) != 0
    assert sparse.mean() > 0.5
    # the plane x = d_x of record j, moved by -8 .. 8 times the margin's order of magnitude: `inside` flips in between
    M = models.astype(np.float64).reshape(n, 4, 4).transpose(0, 2, 1)
    d = np.einsum("nij,nj->ni", M[:, :3, :3], bnd["c"].astype(np.float64)) + M[:, :3, 3]
    flips = 0
    for j in np.flatnonzero(sparse)[:256]:
        step = (np.abs(d[j]).max() + 1.0) * 2.0 ** -18
        pl = np.array([[1.0, 0.0, 0.0, -d[j, 0] + k * step] for k in range(-8, 9)], dtype=F)
        ins = [(both_forms(models[j:j + 1], aff[:1], scale[j:j + 1], bnd[j:j + 1], pl[k:k + 1], 1.0)["flags"][0] & 2) != 0
               for k in range(len(pl))]
        flips += ins[0] != ins[-1]
    assert flips > 100, "the planes must cross the records' own decision"
    # the ratio at which record j turns dense: D / Rc' from a record of its own (dk = k_f D; bk holds Rc' only in sum),
    # so bisect on the flag and scan the ulps around the flip
    for j in np.flatnonzero(sparse)[:64]:
        one = lambda ratio: both_forms(models[j:j + 1], aff[:1], scale[j:j + 1], bnd[j:j + 1], np.zeros((0, 4), dtype=F), ratio)["flags"][0] & 1  # noqa: E731
        lo, hi = F(1.0), F(1e12)
        assert one(float(lo)) == 1 and one(float(hi)) == 0
        while hi.view(np.int32) - lo.view(np.int32) > 1:
            mid = ((lo.view(np.int32).astype(np.int64) + hi.view(np.int32)) // 2).astype(np.int32).view(F)
            lo, hi = (mid, hi) if one(float(mid)) else (lo, mid)
        for k in range(-3, 4):
            one(float((lo.view(np.int32) + np.int32(k)).view(F)))


def test_damaged_records():
    """Non-affine matrices (flagged and projective), bounds that are invalid or were never derived, non-finite matrix
    entries and centres, negative and NaN scale, huge magnitudes: the two forms agree in every byte, NaNs included."""
    rng = np.random.default_rng(81)
    n = 4096
    models, bnd = random_case(rng, n)
    models, bnd = models.copy(), bnd.copy()
    planes = planes_through(rng, 6)
    aff, scale = np.ones(n, dtype=bool), slab_scale(models).copy()
    k = np.arange(n)
    aff[k % 16 == 1] = False
    models[k % 16 == 2, 3] = 1e-3                      # projective
    models[k % 16 == 3, 15] = 0.5
    aff[(k % 16 == 2) | (k % 16 == 3)] = False         # (the slab's flag says so: the setup reads no last row)
    bnd["packed"][k % 16 == 4] = 0                     # invalid
    bnd[k % 16 == 5] = np.zeros((), dtype=BOUND)       # never derived: the zero page
    special = np.array([np.inf, -np.inf, np.nan, -np.nan, 3e38, -3e38, 1e-45, 0.0, -0.0], dtype=F)
    nan2 = np.array([0x7FC00001, 0xFFC12345, 0x7F800001], dtype=np.uint32).view(F)  # NaNs with payloads, one signalling
    pool = np.concatenate([special, nan2])
    for j in np.flatnonzero(k % 16 == 6):
        models[j, rng.integers(0, 16, size=rng.integers(1, 4))] = rng.choice(pool, size=1)
    mixed = k % 16 == 7                                # several different NaNs in one matrix: compared apart, below
    for j in np.flatnonzero(mixed):
        models[j, rng.choice([0, 1, 2, 4, 5, 6, 8, 9, 10], size=3, replace=False)] = nan2
    for j in np.flatnonzero(k % 16 == 8):
        bnd["c"][j, rng.integers(0, 3)] = rng.choice(pool)
    scale[k % 16 == 9] *= F(-1.0)
    scale[k % 16 == 10] = rng.choice(pool, size=int((k % 16 == 10).sum()))
    models[k % 16 == 11] *= F(1e30)
    models[k % 16 == 12] *= F(1e-30)
    models[k % 16 == 13, :12] = 0.0                    # zero scale
    for ratio in (-1.0, 1.0):
        r = both_forms(models[~mixed], aff[~mixed], scale[~mixed], bnd[~mixed], planes, ratio)
        rm = both_forms(models[mixed], aff[mixed], scale[mixed], bnd[mixed], planes, ratio, payloads=False)
        assert not rm["flags"].any() and np.isnan(rm["sigma"]).all()
        kind = k[~mixed] % 16
        sparse = (r["flags"] & 1) != 0
        for g in (1, 2, 3, 4, 5, 9):
            assert not sparse[kind == g].any(), f"damage of kind {g} keeps a record dense"
        assert sparse[kind == 0].any()
    assert np.isnan(r["sigma"]).any(), "NaNs must reach the records for their bits to be compared"


def _fma32(a, b, c):
    """fmaf in binary32, exactly: the product is exact in binary64, the sum rounded to odd there (TwoSum's error says
    which way), and binary64 has more than two bits beyond binary32."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where((e > 0) == (s > 0), s.view(np.int64) + 1, s.view(np.int64) - 1).view(np.float64)
    return np.where((e != 0) & even, toward, s).astype(F)


def test_plane_norm_is_the_expression_it_replaced():
    """nn = sqrtf(fmaf(nz, nz, fmaf(ny, ny, nx * nx))) * kBlkUp + kBlkTiny, every step rounded to binary32."""
    rng = np.random.default_rng(91)
    nrm = (rng.normal(size=(20000, 3)) * np.exp(rng.uniform(np.log(1e-12), np.log(1e12), size=(20000, 1)))).astype(F)
    nrm[:5] = frustum()[:, :3]
    nrm[5] = 0.0
    nrm[6] = (1e-30, 0.0, 0.0)
    h = _host()
    got = np.array([h.orbit_host_block_plane_norm(float(x), float(y), float(z)) for x, y, z in nrm], dtype=F)
    sq = _fma32(nrm[:, 2], nrm[:, 2], _fma32(nrm[:, 1], nrm[:, 1], (nrm[:, 0] * nrm[:, 0]).astype(F)))
    want = (np.sqrt(sq).astype(F) * F(1.0 + 2.0 ** -20)).astype(F) + F(2.0 ** -80)
    assert np.array_equal(got.view(np.uint32), want.astype(F).view(np.uint32))
    assert h.orbit_host_block_plane_norm(float("inf"), 0.0, 0.0) == float("inf")
    assert np.isnan(h.orbit_host_block_plane_norm(float("nan"), 0.0, 1.0))
