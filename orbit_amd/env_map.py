"""ctypes binding of ``orbit_env_map`` and ``orbit_env_sample`` (include/orbit_abi_ext.h E0-E12): the layout call, the job
builders, a device call (on torch tensors, through an ``Engine``'s context) and a mirror call (on numpy arrays, through
``liborbit_host.so``: ``orbit_amd/host/orbit_env_map.hpp``) for each entry point, and the pieces of ``csrc/env_common.h``
the tests pin one by one.  Python adds nothing to the arithmetic."""
import ctypes as C

import numpy as np

from . import _lib
from . import layouts as L
from .passes import _check, lib

MAX_SIZE, MAX_LEVELS, MAX_SAMPLES = _lib.ENV_MAX_SIZE, _lib.ENV_MAX_LEVELS, _lib.ENV_MAX_SAMPLES
# env_map_loader.rs:9-11, cubemap_convolution.frag:20, environmental_map_prefilter.frag:14, forward.rs:135, brdf_integration.frag:75
REFERENCE = dict(sky_size=1024, irradiance_size=32, prefiltered_size=512, prefiltered_levels=5, brdf_size=512, sample_count=4096,
                 sample_delta=0.025, brdf_sample_count=1024)
CENSUS_SIZE = 64  # ORBIT_HOST_ENV_CENSUS
CENSUS_MAJOR, CENSUS_EDGE, CENSUS_CORNER = slice(0, 6), slice(6, 30), slice(30, 54)
CENSUS = dict(z_up=54, x_up=55, ndl_not_positive=56, roughness_zero_texels=57, weight_zero_texels=58, nan_frame_texels=59, two_level_taps=60)


def layout(sky_size=0, irradiance_size=0, prefiltered_size=0, prefiltered_levels=0, brdf_size=0):
    """orbit_env_map_layout -> dict(sky_levels, sky_sizes, sky_offsets, prefiltered_sizes, prefiltered_offsets: per level, in
    texels; sky_texels, irradiance_texels, prefiltered_texels: 8-B texels; brdf_texels: 4-B texels)."""
    out = _lib.EnvMapLayout()
    _lib.check(_lib.load().orbit_env_map_layout(int(sky_size), int(irradiance_size), int(prefiltered_size), int(prefiltered_levels),
                                                int(brdf_size), C.byref(out)))
    ns, npre = out.sky_levels, out.prefiltered_levels
    return dict(sky_levels=ns, sky_sizes=[out.sky_level_size[k] for k in range(ns)], sky_offsets=[out.sky_level_offset[k] for k in range(ns)],
                prefiltered_levels=npre, prefiltered_sizes=[out.prefiltered_level_size[k] for k in range(npre)],
                prefiltered_offsets=[out.prefiltered_level_offset[k] for k in range(npre)], sky_texels=out.sky_texels,
                irradiance_texels=out.irradiance_texels, prefiltered_texels=out.prefiltered_texels, brdf_texels=out.brdf_texels)


def _p(a):
    return None if a is None else a.ctypes.data


def env_map_job(equirect, sky, irradiance, prefiltered, brdf, stats, equirect_w=0, equirect_h=0, sky_size=0, irradiance_size=0,
                prefiltered_size=0, prefiltered_levels=0, brdf_size=0, sample_count=REFERENCE["sample_count"],
                sample_delta=REFERENCE["sample_delta"], brdf_sample_count=REFERENCE["brdf_sample_count"], flags=0):
    """An OrbitEnvMap of six addresses (ints or None) and the by-value fields."""
    j = _lib.EnvMap()
    j.equirect, j.sky, j.irradiance, j.prefiltered, j.brdf, j.stats = equirect, sky, irradiance, prefiltered, brdf, stats
    _lib.fill_env_map(j, equirect_w, equirect_h, sky_size, irradiance_size, prefiltered_size, prefiltered_levels, brdf_size, sample_count,
                      sample_delta, brdf_sample_count, flags)
    return j


def env_sample_job(cube, directions, lods, rgb, bad_directions, size, levels, n, flags=0):
    """An OrbitEnvSample of five addresses (ints or None) and the by-value fields."""
    j = _lib.EnvSample()
    j.cube, j.directions, j.lods, j.rgb, j.bad_directions = cube, directions, lods, rgb, bad_directions
    j.size, j.levels, j.n, j.flags = int(size), int(levels), int(n), int(flags)
    return j


def host_env_map(equirect=None, sky=None, sky_size=0, irradiance_size=0, prefiltered_size=0, prefiltered_levels=0, brdf_size=0,
                 sample_count=REFERENCE["sample_count"], sample_delta=REFERENCE["sample_delta"],
                 brdf_sample_count=REFERENCE["brdf_sample_count"], want_stats=True, want_census=False, fill=0):
    """orbit_host_env_map.  equirect: None or (h, w, 4) float32; sky: None (made from equirect where sky_size > 0) or the
    caller's cube, np.uint16 (sky_texels * 4,).  A product of size 0 is not made.  -> dict(sky, irradiance, prefiltered:
    np.uint16 (texels * 4,); brdf: np.uint16 (texels * 2,); stats: np[layouts.ENV_MAP_STATS] row; census: np.uint64
    (CENSUS_SIZE,); layout), each None if not made or wanted."""
    lay = layout(sky_size, irradiance_size, prefiltered_size, prefiltered_levels, brdf_size)
    eq = None if equirect is None or not sky_size else np.ascontiguousarray(equirect, dtype=np.float32)  # no sky cube: no panorama
    make = lambda texels, halves: np.full(int(texels) * halves, fill, np.uint16) if texels else None  # noqa: E731
    if sky is None:
        sky_buf = make(lay["sky_texels"], 4) if eq is not None else None
    else:
        sky_buf = np.ascontiguousarray(sky, dtype=np.uint16).reshape(-1).copy()
        if sky_buf.size != lay["sky_texels"] * 4:
            raise ValueError("sky holds another number of texels than the layout's")
    irr, pre, brdf = make(lay["irradiance_texels"], 4), make(lay["prefiltered_texels"], 4), make(lay["brdf_texels"], 2)
    stats = np.zeros(1, L.ENV_MAP_STATS) if want_stats else None
    census = np.zeros(CENSUS_SIZE, np.uint64) if want_census else None
    eh, ew = (0, 0) if eq is None else eq.shape[:2]
    j = env_map_job(_p(eq), _p(sky_buf), _p(irr), _p(pre), _p(brdf), _p(stats), ew, eh, sky_size, irradiance_size, prefiltered_size,
                    prefiltered_levels, brdf_size, sample_count, sample_delta, brdf_sample_count)
    fn = lib().orbit_host_env_map
    fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.c_void_p]
    _check(fn(C.byref(j), _p(census)))
    return dict(sky=sky_buf, irradiance=irr, prefiltered=pre, brdf=brdf, stats=None if stats is None else stats[0], census=census, layout=lay)


def host_prefilter_texels(sky, sky_size, prefiltered_size, prefiltered_levels, sample_count, level, texels):
    """orbit_host_env_prefilter_texels: the stated texels (face * n * n + py * n + px) of one level of the prefiltered cube
    from a sky cube np.uint16 -> np.uint16 (len(texels), 4).  For runs too large for the whole mirror."""
    sky_buf = np.ascontiguousarray(sky, dtype=np.uint16).reshape(-1)
    tex = np.ascontiguousarray(texels, dtype=np.uint32).reshape(-1)
    out = np.zeros((max(len(tex), 1), 4), np.uint16)
    j = env_map_job(None, _p(sky_buf), None, _p(out), None, None, sky_size=sky_size, prefiltered_size=prefiltered_size,
                    prefiltered_levels=prefiltered_levels, sample_count=sample_count)
    fn = lib().orbit_host_env_prefilter_texels
    fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    _check(fn(C.byref(j), int(level), _p(tex), len(tex), _p(out)))
    return out[:len(tex)]


def host_env_map_raw(job, census=None):
    """orbit_host_env_map of a job block as it is -> the status (for the tests of E9)."""
    fn = lib().orbit_host_env_map
    fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.c_void_p]
    return fn(C.byref(job), _p(census))


def host_env_sample(cube, size, levels, directions, lods, want_census=False):
    """orbit_host_env_sample of cube np.uint16 (E0's layout), directions (n, 3) and lods (n,) float32 -> dict(rgb (n, 3)
    float32, bad_directions: int, census)."""
    cub = np.ascontiguousarray(cube, dtype=np.uint16).reshape(-1)
    d, l = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(lods, dtype=np.float32).reshape(-1)
    if len(d) != len(l):
        raise ValueError("directions and lods differ in number")
    if cub.size != layout(prefiltered_size=size, prefiltered_levels=levels)["prefiltered_texels"] * 4:
        raise ValueError("cube holds another number of texels than its size and levels give")
    rgb, bad = np.zeros((max(len(d), 1), 3), np.float32), np.zeros(1, np.uint64)
    census = np.zeros(CENSUS_SIZE, np.uint64) if want_census else None
    j = env_sample_job(_p(cub), _p(d), _p(l), _p(rgb), _p(bad), size, levels, len(d))
    fn = lib().orbit_host_env_sample
    fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.c_void_p]
    _check(fn(C.byref(j), _p(census)))
    return dict(rgb=rgb[:len(d)], bad_directions=int(bad[0]), census=census)


def host_env_sample_raw(job):
    """orbit_host_env_sample of a job block as it is -> the status (for the tests of E9)."""
    fn = lib().orbit_host_env_sample
    fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.c_void_p]
    return fn(C.byref(job), None)


def host_direction(face, px, py, n):
    """E1 of one texel -> (3,) float32."""
    out = np.zeros(3, np.float32)
    fn = lib().orbit_host_env_direction
    fn.restype, fn.argtypes = None, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    fn(int(face), int(px), int(py), int(n), _p(out))
    return out


def _routine(which, a, b=None):
    x = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    y = x if b is None else np.ascontiguousarray(np.broadcast_to(np.asarray(b, np.float32), np.shape(a)), dtype=np.float32).reshape(-1)
    out = np.zeros(x.size, np.float32)
    fn = lib().orbit_host_env_routines
    fn.restype, fn.argtypes = None, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    fn(which, _p(x), _p(y), x.size, _p(out))
    return out.reshape(np.shape(a))


def host_atan2c(y, x):
    """E2's atan(y, x), elementwise over float32 arrays of one shape."""
    return _routine(0, y, x)


def host_asinc(x):
    """E2's asin."""
    return _routine(1, x)


def host_sincos(theta):
    """The sine and cosine E5-E7 use (H6's routine) -> (sin, cos)."""
    return _routine(2, theta), _routine(3, theta)


def host_half(x):
    """E0's store of float32 values, read back -> float32 (NaN where the value is not finite and +0 is stored)."""
    return _routine(4, x)


def _ptr(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def _stream(stream):
    import torch

    s = torch.cuda.current_stream() if stream is None else stream
    return C.c_void_p(s.cuda_stream)


def device_env_map(engine, equirect=None, sky=None, irradiance=None, prefiltered=None, brdf=None, stats=None, equirect_w=0, equirect_h=0,
                   sky_size=0, irradiance_size=0, prefiltered_size=0, prefiltered_levels=0, brdf_size=0,
                   sample_count=REFERENCE["sample_count"], sample_delta=REFERENCE["sample_delta"],
                   brdf_sample_count=REFERENCE["brdf_sample_count"], flags=0, stream=None):
    """orbit_env_map on device tensors (or raw addresses): equirect (equirect_w * equirect_h * 4 floats) or None, sky /
    irradiance / prefiltered (uint16 or any tensor of layout()'s sizes, 8 B per texel), brdf (4 B per texel), stats (48
    bytes, layouts.ENV_MAP_STATS, cleared by the call); a product that is None is not made.  Byte-equal to host_env_map.
    Enqueued on `stream`."""
    j = env_map_job(_ptr(equirect), _ptr(sky), _ptr(irradiance), _ptr(prefiltered), _ptr(brdf), _ptr(stats), equirect_w, equirect_h,
                    sky_size, irradiance_size, prefiltered_size, prefiltered_levels, brdf_size, sample_count, sample_delta,
                    brdf_sample_count, flags)
    _lib.check(engine._lib.orbit_env_map(engine._ctx, C.byref(j), _stream(stream)), engine._ctx)


def device_env_sample(engine, cube, size, levels, directions, lods, rgb, n, bad_directions=None, flags=0, stream=None):
    """orbit_env_sample on device tensors: cube (E0's layout), directions (n * 3 floats), lods (n floats) -> rgb (n * 3
    floats) and bad_directions (8 bytes, cleared by the call, or None).  Byte-equal to host_env_sample."""
    j = env_sample_job(_ptr(cube), _ptr(directions), _ptr(lods), _ptr(rgb), _ptr(bad_directions), size, levels, n, flags)
    _lib.check(engine._lib.orbit_env_sample(engine._ctx, C.byref(j), _stream(stream)), engine._ctx)
