"""ctypes binding of the host mirror of ``orbit_bloom`` and ``orbit_post_process`` (``orbit_amd/host/orbit_post.hpp``):
the reference's bloom chain of a colour plane and its tone mapping and sRGB encoding on host arrays — the references of
``Engine.bloom`` and ``Engine.post_process`` —, ``orbit_bloom_layout``, the pieces of ``csrc/post_common.h`` the tests pin
one by one (downsample and upsample on floats, the B10G11R11 pack, ``powc``), and ``write_ppm``; and of the mirror of
``orbit_ssao`` (``orbit_amd/host/orbit_ssao.hpp``) with the pieces of ``csrc/ssao_common.h``, ``ssao_tables``,
``ssao_resolution`` and ``write_pgm``.  Python adds nothing to the arithmetic."""
import ctypes as C

import numpy as np

from . import _lib
from . import layouts as L
from .passes import _check, lib

FORCE_PER_LEVEL, FORCE_DIRECT, BGRA = _lib.BLOOM_FORCE_PER_LEVEL, _lib.BLOOM_FORCE_DIRECT, _lib.POST_BGRA
MAX_LEVELS = _lib.BLOOM_MAX_LEVELS
DEFAULTS = dict(threshold=0.0, soft_threshold=0.0, filter_radius=0.003, bloom_intensity=0.025)  # BloomSettings::default


def bloom_layout(width, height, max_levels=MAX_LEVELS):
    """orbit_bloom_layout -> dict(levels, total_texels, sizes: [(w, h)] per level, offsets: [first texel] per level)."""
    out = _lib.BloomLayout()
    out.max_levels = int(max_levels)
    _lib.check(_lib.load().orbit_bloom_layout(int(width), int(height), C.byref(out)))
    n = out.levels
    return dict(levels=n, total_texels=out.total_texels, sizes=[(out.level_width[k], out.level_height[k]) for k in range(n)],
                offsets=[out.level_offset[k] for k in range(n)])


def _p(a):
    return None if a is None else a.ctypes.data


def host_bloom(color, threshold=0.0, soft_threshold=0.0, filter_radius=0.003, max_levels=MAX_LEVELS, form=None, want_stats=True,
               fill=0, guard=0):
    """orbit_host_bloom of color (height, width, 4) float32 -> dict(mips: np.uint32 (total_texels + guard,), the words
    behind the chain still `fill`; stats: np[layouts.BLOOM_STATS] scalar row or None; layout: bloom_layout's dict)."""
    col = np.ascontiguousarray(color, dtype=np.float32)
    height, width = col.shape[:2]
    lay = bloom_layout(width, height, max_levels)
    mips = np.full(lay["total_texels"] + guard, fill, np.uint32)
    stats = np.zeros(1, L.BLOOM_STATS) if want_stats else None
    j = _lib.Bloom()
    j.color, j.mips, j.stats = _p(col), _p(mips), _p(stats)
    _lib.fill_bloom(j, width, height, threshold, soft_threshold, filter_radius, max_levels, form)
    _check(lib().orbit_host_bloom(C.byref(j)))
    return dict(mips=mips, stats=None if stats is None else stats[0], layout=lay)


def host_post_process(color, bloom=None, exposure=1.0, bloom_intensity=0.025, render_mode=0, bgra=False, want_ldr=True,
                      want_rgba8=True, want_stats=True, fill=0):
    """orbit_host_post_process of color (height, width, 4) float32 and bloom (None, or at least height * width np.uint32:
    level 0 of host_bloom's mips) -> dict(ldr (height, width, 4) float32, rgba8 (height, width, 4) uint8, stats:
    np[layouts.POST_STATS] scalar row), each None if not wanted."""
    col = np.ascontiguousarray(color, dtype=np.float32)
    height, width = col.shape[:2]
    blm = None if bloom is None else np.ascontiguousarray(bloom, dtype=np.uint32).reshape(-1)
    if blm is not None and blm.size < width * height:
        raise ValueError("bloom holds fewer texels than the target")
    ldr = np.full((height, width, 4), fill, np.uint32).view(np.float32) if want_ldr else None
    rgba8 = np.full((height, width), fill, np.uint32).view(np.uint8).reshape(height, width, 4) if want_rgba8 else None
    stats = np.zeros(1, L.POST_STATS) if want_stats else None
    j = _lib.PostProcess()
    j.color, j.bloom, j.ldr, j.rgba8, j.stats = _p(col), _p(blm), _p(ldr), _p(rgba8), _p(stats)
    _lib.fill_post_process(j, width, height, exposure, bloom_intensity, render_mode, bgra)
    _check(lib().orbit_host_post_process(C.byref(j)))
    return dict(ldr=ldr, rgba8=rgba8, stats=None if stats is None else stats[0])


def threshold_filter(threshold, soft_threshold):
    """B2's four floats, in float32 as the reference's host code computes them."""
    f = np.float32
    knee = f(threshold) * f(soft_threshold)
    return np.array([f(threshold), f(threshold) - knee, f(2.0) * knee, f(0.25) / (knee + f(0.00001))], np.float32)


def host_downsample_floats(src, dst_w, dst_h, level0=False, tf=None):
    """One downsample (B3-B5) of src (h, w, 3) float32 -> (dst_h, dst_w, 3) float32, nothing packed."""
    s = np.ascontiguousarray(src, dtype=np.float32)
    out = np.zeros((dst_h, dst_w, 3), np.float32)
    t = np.zeros(4, np.float32) if tf is None else np.ascontiguousarray(tf, dtype=np.float32)
    fn = lib().orbit_host_bloom_downsample_floats
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    fn(_p(s), s.shape[1], s.shape[0], dst_w, dst_h, 1 if level0 else 0, _p(t), _p(out))
    return out


def host_upsample_floats(src, dst_w, dst_h, filter_radius):
    """B6's added term of one upsample of src (h, w, 3) float32 -> (dst_h, dst_w, 3) float32."""
    s = np.ascontiguousarray(src, dtype=np.float32)
    out = np.zeros((dst_h, dst_w, 3), np.float32)
    fn = lib().orbit_host_bloom_upsample_floats
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
    fn(_p(s), s.shape[1], s.shape[0], dst_w, dst_h, float(filter_radius), _p(out))
    return out


def host_pack(rgb):
    """B7 of rgb (..., 3) float32 -> (words np.uint32 (...), clamped np.bool_ (...))."""
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    n = a.size // 3
    words, clamped = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    fn = lib().orbit_host_bloom_pack
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    fn(_p(a), n, _p(words), _p(clamped))
    return words.reshape(a.shape[:-1]), clamped.astype(bool).reshape(a.shape[:-1])


def host_unpack(words):
    """B7's decode of np.uint32 (...) -> (..., 3) float32."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.zeros(w.shape + (3,), np.float32)
    fn = lib().orbit_host_bloom_unpack
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_uint64, C.c_void_p]
    fn(_p(w), w.size, _p(out))
    return out


def host_powc(x, y):
    """powc(x, y) of B5 and T4, elementwise over float32 x."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros_like(a)
    fn = lib().orbit_host_powc
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_uint64, C.c_float, C.c_void_p]
    fn(_p(a), a.size, float(y), _p(out))
    return out


SSAO_DEFAULTS = dict(sample_count=32, min_radius=0.1, max_radius=0.5, full_res=False)  # SsaoSettings::default
SSAO_NOISE_SIZE, SSAO_SAMPLES_SIZE = 4, 64                                              # ssao.rs:174-175
SSAO_CENSUS = ("right_up", "right_down", "left_up", "left_down", "in_range", "out_of_range", "occluded", "unoccluded", "range_inside",
               "range_zero", "range_one", "range_nan", "depth_equal", "tie_horizontal", "tie_vertical", "proj_at_zero", "proj_at_one",
               "proj_below_zero", "proj_above_one")


def ssao_resolution(width, height, full_res=False):
    """The SSAO images' size of a width x height screen (ssao.rs:93-97): the screen's, or each dimension // 2."""
    return (int(width), int(height)) if full_res else (int(width) // 2, int(height) // 2)


def ssao_tables(seed, noise_size=SSAO_NOISE_SIZE, samples_size=SSAO_SAMPLES_SIZE):
    """The reference's two tables as ssao.rs:177-237 fills them, every byte random, from a seeded generator -> (noise
    (noise_size, noise_size, 2) int8: R8G8_SNORM, samples (samples_size, 4) uint8: R8G8B8A8_UNORM)."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(-128, 128, (noise_size, noise_size, 2), dtype=np.int8)
    samples = rng.integers(0, 256, (samples_size, 4), dtype=np.uint8)
    return noise, samples


def host_ssao(depth, projection, inverse_projection, noise, samples, ssao_w=None, ssao_h=None, sample_count=32, min_radius=0.1,
              max_radius=0.5, want=("raw", "blurred", "ao_pixel"), want_stats=True, want_census=False, fill=0, flags=0):
    """orbit_host_ssao of depth (screen_h, screen_w) float32, noise (n, n, 2) int8 and samples (m, 4) uint8 -> dict(raw,
    blurred: (ssao_h, ssao_w) uint8; ao_pixel: (screen_h, screen_w) float32; stats: np[layouts.SSAO_STATS] scalar row;
    census: {name: count} over SSAO_CENSUS), each None if not wanted.  ssao_w, ssao_h default to the screen's."""
    dep = np.ascontiguousarray(depth, dtype=np.float32)
    screen_h, screen_w = dep.shape
    ssao_w, ssao_h = screen_w if ssao_w is None else int(ssao_w), screen_h if ssao_h is None else int(ssao_h)
    noi, sam = np.ascontiguousarray(noise, dtype=np.int8), np.ascontiguousarray(samples, dtype=np.uint8)
    shape = (max(ssao_h, 0), max(ssao_w, 0))
    raw = np.full(shape, fill, np.uint8) if "raw" in want else None
    blurred = np.full(shape, fill, np.uint8) if "blurred" in want else None
    ao_pixel = np.full((screen_h, screen_w), fill, np.uint32).view(np.float32) if "ao_pixel" in want else None
    stats = np.zeros(1, L.SSAO_STATS) if want_stats else None
    census = np.zeros(len(SSAO_CENSUS), np.uint64) if want_census else None
    j = _lib.Ssao()
    j.depth, j.noise, j.samples, j.raw, j.blurred, j.ao_pixel, j.stats = _p(dep), _p(noi), _p(sam), _p(raw), _p(blurred), _p(ao_pixel), _p(stats)
    _lib.fill_ssao(j, projection, inverse_projection, screen_w, screen_h, ssao_w, ssao_h, noi.shape[0], sam.shape[0], sample_count, min_radius,
                   max_radius, flags)
    fn = lib().orbit_host_ssao
    fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.c_void_p]
    _check(fn(C.byref(j), _p(census)))
    return dict(raw=raw, blurred=blurred, ao_pixel=ao_pixel, stats=None if stats is None else stats[0],
                census=None if census is None else {n: int(v) for n, v in zip(SSAO_CENSUS, census)})


def host_ssao_table(samples, sample_count, min_radius=0.1, max_radius=0.5):
    """A4's table of samples (m, 4) uint8 -> (sample_count, 4) float32: the hemisphere direction and the radius per sample."""
    sam = np.ascontiguousarray(samples, dtype=np.uint8)
    out = np.zeros((int(sample_count), 4), np.float32)
    fn = lib().orbit_host_ssao_table
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_void_p]
    fn(_p(sam), sam.shape[0], int(sample_count), float(min_radius), float(max_radius), _p(out))
    return out


def host_ssao_in_range(proj):
    """A5's range test of proj (..., 3) float32 -> np.bool_ (...)."""
    a = np.ascontiguousarray(proj, dtype=np.float32)
    out = np.zeros(a.size // 3, np.uint8)
    fn = lib().orbit_host_ssao_in_range
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_uint64, C.c_void_p]
    fn(_p(a), out.size, _p(out))
    return out.astype(bool).reshape(a.shape[:-1])


def host_ssao_range_check(min_radius, sample_depth, proj_w):
    """A5's range_check, elementwise over float32 arrays of one shape."""
    args = np.ascontiguousarray(np.stack(np.broadcast_arrays(np.float32(min_radius), np.float32(sample_depth), np.float32(proj_w)), -1), dtype=np.float32)
    out = np.zeros(args.shape[:-1], np.float32)
    fn = lib().orbit_host_ssao_range_check
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_uint64, C.c_void_p]
    fn(_p(args), out.size, _p(out))
    return out


def write_pgm(path, gray):
    """A binary PGM (P5) of gray (height, width) uint8."""
    img = np.ascontiguousarray(gray, dtype=np.uint8)
    height, width = img.shape
    with open(path, "wb") as fh:
        fh.write(b"P5\n%d %d\n255\n" % (width, height))
        fh.write(img.tobytes())


def write_ppm(path, rgba8):
    """A binary PPM (P6) of rgba8 (height, width, 4) uint8 in R, G, B, A order; alpha is dropped."""
    img = np.ascontiguousarray(rgba8, dtype=np.uint8)
    height, width = img.shape[:2]
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (width, height))
        fh.write(np.ascontiguousarray(img[:, :, :3]).tobytes())
