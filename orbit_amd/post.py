"""ctypes binding of the host mirror of ``orbit_bloom`` and ``orbit_post_process`` (``orbit_amd/host/orbit_post.hpp``):
the reference's bloom chain of a colour plane and its tone mapping and sRGB encoding on host arrays — the references of
``Engine.bloom`` and ``Engine.post_process`` —, ``orbit_bloom_layout``, the pieces of ``csrc/post_common.h`` the tests pin
one by one (downsample and upsample on floats, the B10G11R11 pack, ``powc``), and ``write_ppm``.  Python adds nothing."""
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


def write_ppm(path, rgba8):
    """A binary PPM (P6) of rgba8 (height, width, 4) uint8 in R, G, B, A order; alpha is dropped."""
    img = np.ascontiguousarray(rgba8, dtype=np.uint8)
    height, width = img.shape[:2]
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (width, height))
        fh.write(np.ascontiguousarray(img[:, :, :3]).tobytes())
