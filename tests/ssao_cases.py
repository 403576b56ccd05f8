"""Inputs for orbit_ssao (include/orbit_abi_ext.h A1-A9): hand-built depth planes on SSAO sizes that sit one texel either
side of the shader's 8 x 8 group and of the kernel's 16 x 16 tile, each with the screen at the SSAO size, at twice it and at
twice it plus one (the odd sizes `/ 2` floors); the two tables seeded, degenerate and of other sizes.  As in its neighbours,
the expected bytes are never stored: they come from the host mirror or from tests/ssao_ref.py."""
import numpy as np

from orbit_amd import passes, post

F = np.float32
Z_NEAR = 0.01

SSAO_SIZES = ((1, 1), (2, 1), (1, 9), (5, 3), (7, 7), (8, 8), (9, 9), (15, 17), (16, 16), (17, 15), (33, 31), (70, 33))
SMALL_SIZES = ((1, 1), (5, 3), (9, 9), (17, 15), (33, 31))
IMAGES = ("uncovered", "plane", "floor_box", "spike", "steps", "nonfinite", "noise")
SAMPLE_COUNTS = (1, 2, 31, 32, 33, 64)
RADII = ((0.0, 0.0), (0.1, 0.5), (1.0, 1.0))
OUTPUT_SUBSETS = (("raw",), ("raw", "blurred"), ("raw", "blurred", "ao_pixel"))


def screens(ssao_w, ssao_h):
    """The screen sizes an SSAO size runs with: its own, 2 x and 2 x + 1"""
    return ((ssao_w, ssao_h), (2 * ssao_w, 2 * ssao_h), (2 * ssao_w + 1, 2 * ssao_h + 1))


def camera(screen_w, screen_h, fov_deg=90.0):
    """(projection[16], inverse_projection[16]) of the reference's camera at this aspect: reverse-z, infinite far plane"""
    proj = passes.projection_compute_matrix(passes.Projection.Perspective(float(np.deg2rad(F(fov_deg))), Z_NEAR), screen_w / screen_h)
    return proj, passes.mat4_inverse(proj)


def depth_image(kind, width, height, seed=11):
    """(height, width) float32 reverse-z depth: Z_NEAR / distance, 0 = uncovered"""
    rng = np.random.default_rng(seed + 1000 * width + height)
    yy, xx = np.mgrid[0:height, 0:width]
    if kind == "uncovered":
        return np.zeros((height, width), F)
    dist = np.full((height, width), 5.0)
    if kind == "plane":  # constant depth: every |dz| of A2 ties, so every pixel takes left / up
        pass
    elif kind == "floor_box":  # a floor receding toward the top, a box standing on it and a strip of sky: real occlusion
        dist = 2.0 + 6.0 * (1.0 - (yy + 0.5) / height) + 0.3 * (xx + 0.5) / width
        box = (xx >= width // 3) & (xx < max(width // 3 + 1, 2 * width // 3)) & (yy >= height // 3) & (yy < max(height // 3 + 1, 3 * height // 4))
        dist = np.where(box, 3.0 + 0.2 * (xx + 0.5) / width, dist)
        d = (Z_NEAR / dist).astype(F)
        d[0, :] = 0.0 if height > 2 else d[0, :]
        return d
    elif kind == "spike":  # one pixel much nearer than the plane around it
        dist[height // 2, width // 2] = 0.5
    elif kind == "steps":  # depth steps on columns and rows 0, 1 and the last, where A1's wrap decides the normal
        dist = np.where((xx == 0) | (xx == width - 1), 4.0, dist)
        dist = np.where(xx == 1, 6.0, dist)
        dist = np.where((yy == 0) | (yy == height - 1), dist - 0.5, dist)
        dist = np.where(yy == 1, dist + 0.75, dist)
    elif kind == "nonfinite":
        d = (Z_NEAR / (4.0 + rng.uniform(0.0, 2.0, (height, width)))).astype(F)
        d[0, 0] = np.nan
        d[height - 1, width - 1] = np.inf
        d[height // 2, width // 2] = -0.002
        d[height // 3, (2 * width) // 3] = -np.inf
        return d
    elif kind == "noise":
        return (rng.uniform(0.0, 1.0, (height, width)) ** 3 * 0.01).astype(F)
    else:
        raise KeyError(kind)
    return (Z_NEAR / dist).astype(F)


def tables(kind="seeded", seed=5):
    """(noise (n, n, 2) int8, samples (m, 4) uint8)"""
    if kind == "seeded":
        return post.ssao_tables(seed)
    if kind == "zero_noise":  # (0, 0) texels: the basis is NaN, every sample fails the range test, every byte 255
        return np.zeros((4, 4, 2), np.int8), post.ssao_tables(seed)[1]
    if kind == "snorm_clamp":  # -128 reads as -1, as -127 does
        return np.full((4, 4, 2), -128, np.int8), post.ssao_tables(seed)[1]
    if kind == "mixed_noise":  # some (0, 0) texels among the rest, and the clamp
        n = post.ssao_tables(seed, noise_size=4)[0].copy()
        n[1, 2] = 0
        n[3, 0] = -128
        return n, post.ssao_tables(seed)[1]
    sizes = dict(noise1=(1, 64), noise3=(3, 64), noise64=(64, 64), samples1=(4, 1), samples100=(4, 100), samples256=(4, 256))
    return post.ssao_tables(seed, *sizes[kind])


TABLES = ("seeded", "zero_noise", "snorm_clamp", "mixed_noise", "noise1", "noise3", "noise64", "samples1", "samples100", "samples256")


def case(kind, ssao_size, screen_size, table_kind="seeded", **settings):
    """-> (name, dict of host_ssao's / ssao_ref.ssao's arguments)"""
    (w, h), (sw, sh) = ssao_size, screen_size
    proj, inv = camera(sw, sh)
    noise, samples = tables(table_kind)
    kw = dict(depth=depth_image(kind, sw, sh), projection=proj, inverse_projection=inv, noise=noise, samples=samples, ssao_w=w, ssao_h=h, **settings)
    tail = "".join(f" {k}={v}" for k, v in settings.items())
    return f"{kind} {w}x{h} of {sw}x{sh} {table_kind}{tail}", kw


def census(kw):
    """What a case exercises, counted by the mirror over every pixel and sample -> {name: count} over post.SSAO_CENSUS: A2's
    four branches, samples in / out of range, occluded / not, range_check strictly inside (0, 1), exactly 0, exactly 1 and
    NaN, samples with sample_depth == proj.z, pixels whose horizontal / vertical |dz| tie"""
    return post.host_ssao(want_census=True, **kw)["census"]


# A5's knife edges, found by searching with the mirror's own functions: (image, SSAO size = screen, sample_count, the radius
# bracket).  Between the bracket's ends some sample leaves [0, 1]; the search bisects the float32 radii (min = max) down to
# two NEIGHBOURING floats, the last radius with the sample in range and the first with it rejected.  A radius step moves
# proj.xy by far less than an ulp of it, so on the last radius the component is EXACTLY on the edge (1, or 0) and on the
# first it is one step outside (1 + 2^-23, or -2^-24: the first value x * 0.5 + 0.5 takes below 0); census() says which.
EDGE_SEARCHES = (("plane", (9, 9), 4, 0.0, 6.0), ("plane", (5, 3), 3, 0.0, 6.0), ("plane", (17, 15), 6, 0.0, 6.0), ("floor_box", (9, 9), 7, 0.0, 6.0))
_EDGES = []


def _radius_boundary(make, lo, hi):
    """Neighbouring float32 radii (a, b), lo <= a < b <= hi: out_of_range of make(a) equals that of make(lo), of make(b) not"""
    bits = lambda x: int(F(x).view(np.uint32))  # noqa: E731
    flt = lambda b: float(np.uint32(b).view(F))  # noqa: E731
    c0 = census(make(lo))["out_of_range"]
    assert census(make(hi))["out_of_range"] != c0, "the bracket holds no edge"
    a, b = bits(lo), bits(hi)
    while b - a > 1:
        m = (a + b) // 2
        if census(make(flt(m)))["out_of_range"] == c0:
            a = m
        else:
            b = m
    return flt(a), flt(b)


def edge_cases():
    """[(name, arguments)]: per search the case at the last radius in range and the case at the first one rejected"""
    if not _EDGES:
        for kind, size, count, lo, hi in EDGE_SEARCHES:
            make = lambda r: case(kind, size, size, sample_count=count, min_radius=r, max_radius=r)  # noqa: E731
            a, b = _radius_boundary(lambda r: make(r)[1], lo, hi)
            _EDGES.extend([make(a), make(b)])
    return list(_EDGES)


def all_cases(sizes=SSAO_SIZES):
    """Every image on every SSAO size and each of its three screens, the reference's default settings"""
    return [case(kind, size, screen) for size in sizes for screen in screens(*size) for kind in IMAGES]


def settings_cases():
    """Sample counts x radii and the other tables, on a few sizes and the images that have samples in range"""
    out = []
    for size in ((5, 3), (17, 15)):
        screen = screens(*size)[2]
        for n in SAMPLE_COUNTS:
            for lo, hi in RADII:
                for kind in ("floor_box", "noise"):
                    out.append(case(kind, size, screen, sample_count=n, min_radius=lo, max_radius=hi))
        for t in TABLES[1:]:
            for kind in ("floor_box", "steps"):
                out.append(case(kind, size, screen, t))
                out.append(case(kind, size, screen, t, sample_count=64))
    return out
