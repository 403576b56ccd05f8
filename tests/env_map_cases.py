"""The case matrix of orbit_env_map and orbit_env_sample (include/orbit_abi_ext.h E0-E12), shared by tests/test_env_map_cpu.py
(mirror against the numpy restatement), tests/test_env_map_gpu.py (device against mirror) and tools/count_env_map.py.

Sky sizes 1, 2, 4, 8, 16; irradiance sizes 1, 2, 3 (an odd size: the NaN frame at the centre of the +-Y layers), 5, 8;
prefiltered sizes 1, 2, 5, 16, 17 (17 crosses the kernel's 16 x 16 tile) each with 1, 2 and 5 levels (5 levels on sizes 1,
2 and 5 reach extent 1 more than once); sample counts 1, 2, 63, 64, 65 (either side of a wave of the threads that fill a
chunk), 255, 256, 257 (either side of the 256-sample LDS chunk) and 513 (a third chunk); sample_delta 0.5, 0.25 and
DISAGREEING_DELTA, found by search, at which the loop's fp32 accumulation and i * delta disagree on the trip count; BRDF
sizes 1, 2, 16, 17.  The large counts go with the small sizes: the restatement is a Python loop over the samples."""
import itertools

import numpy as np

F = np.float32


def _trips(delta, limit, accumulate):
    n, x = 0, F(0.0)
    while x < limit:
        n += 1
        x = F(x + delta) if accumulate else F(F(n) * delta)
    return n


def find_disagreeing_delta():
    """the first delta of a fixed sweep at which `for (x = 0; x < 2 PI; x += delta)` in fp32 runs another number of times than
    counting the i with i * delta < 2 PI.  The two can only part where k * delta comes within the accumulated rounding of 2
    PI, so the sweep is 2 PI / k for k = 11 .. 40, a few steps of fp32 either side"""
    limit = F(2.0) * F(3.14159265359)
    for k in range(11, 41):
        centre = F(limit / F(k))
        for steps in range(-4, 5):
            delta = centre
            for _ in range(abs(steps)):
                delta = np.nextafter(delta, F(np.inf) if steps > 0 else F(0.0))
            if _trips(delta, limit, True) != _trips(delta, limit, False):
                return float(delta)
    raise AssertionError("no such delta in the sweep")


DISAGREEING_DELTA = find_disagreeing_delta()


def panorama(name):
    """(h, w, 4) float32"""
    rng = np.random.default_rng(20261021)
    if name == "constant":
        p = np.full((1, 1, 4), 0.75, F)
    elif name == "one_lit":
        p = np.zeros((3, 7, 4), F)
        p[1, 4] = (3.0, 2.0, 1.0, 1.0)
    elif name == "gradient_u":  # shows E1's rotation
        p = np.zeros((32, 64, 4), F)
        p[..., 0] = np.linspace(0, 1, 64, dtype=F)[None, :]
        p[..., 1] = 0.25
    elif name == "gradient_v":  # shows E2's flip
        p = np.zeros((3, 7, 4), F)
        p[..., 2] = np.linspace(0, 2, 3, dtype=F)[:, None]
    elif name == "above_max":
        p = np.array([[[20000.0, 9999.0, 10001.0, 1.0], [1e-6, 3e-8, 6e-5, 1.0]]], F)  # and values below fp16's normal range
    elif name == "hostile":
        p = rng.random((3, 7, 4)).astype(F)
        p[0, 0, 0], p[0, 3, 1], p[1, 5, 2], p[2, 2, 0], p[2, 6, 1] = -1.0, np.nan, np.inf, -np.inf, -0.0
    elif name == "noise":
        p = (rng.random((32, 64, 4)) * 4.0).astype(F)
    elif name == "noise_2x1":
        p = rng.random((1, 2, 4)).astype(F)
    else:
        raise KeyError(name)
    return p


def _case(name, pano, sky, irr=0, delta=0.5, pre=(0, 0), count=1, brdf=0, brdf_count=1):
    return name, dict(equirect=None if pano is None else panorama(pano), sky_size=sky, irradiance_size=irr, sample_delta=delta,
                      prefiltered_size=pre[0], prefiltered_levels=pre[1], sample_count=count, brdf_size=brdf, brdf_sample_count=brdf_count)


def chain_cases():
    """[(name, host_env_map's keywords)]: whole calls, every product from the call's own sky cube"""
    return [
        _case("sky1_constant", "constant", 1, irr=1, pre=(1, 1), count=1, brdf=1, brdf_count=1),
        _case("sky2_one_lit", "one_lit", 2, irr=2, delta=0.25, pre=(2, 2), count=2, brdf=2, brdf_count=2),
        _case("sky4_gradient_u", "gradient_u", 4, irr=3, pre=(5, 5), count=63, brdf=16, brdf_count=64),
        _case("sky8_gradient_v", "gradient_v", 8, irr=5, delta=DISAGREEING_DELTA, pre=(16, 1), count=64, brdf=17, brdf_count=65),
        _case("sky16_hostile", "hostile", 16, irr=8, pre=(17, 2), count=65),
        _case("sky4_above_max", "above_max", 4, irr=2, pre=(1, 5), count=256),
        _case("sky8_noise", "noise", 8, irr=3, delta=0.25, pre=(5, 2), count=257),
        _case("sky2_noise_2x1", "noise_2x1", 2, irr=5, pre=(2, 1), count=255),
        _case("sky16_noise", "noise", 16, pre=(16, 5), count=7),
        _case("sky8_pre17x5", "noise", 8, pre=(17, 5), count=3),
        _case("sky4_pre1x2", "one_lit", 4, pre=(1, 2), count=513),
        _case("sky4_pre2x5", "gradient_u", 4, pre=(2, 5), count=64),
        _case("sky8_pre5x1", "hostile", 8, pre=(5, 1), count=65),
        _case("sky16_pre16x2", "gradient_v", 16, pre=(16, 2), count=5),
        _case("sky1_pre17x1", "constant", 1, pre=(17, 1), count=2),
    ]


# the one chained run of the GPU test and tools/bench_env_map.py's reduced size
CHAINED = _case("chained", "noise", 16, irr=8, delta=0.25, pre=(16, 5), count=64, brdf=16, brdf_count=64)


def noise_cube(size, levels, seed=7):
    """a cube in E0's layout of finite seeded halves (some negative, some subnormal), alpha 1 -> np.uint16"""
    rng = np.random.default_rng(seed)
    texels = sum(6 * max(1, size >> m) ** 2 for m in range(levels))
    v = (rng.random((texels, 4)) * 8.0 - 1.0).astype(np.float16)
    v[::7, 1] = np.float16(3e-6)
    v[:, 3] = np.float16(1.0)
    return v.view(np.uint16).reshape(-1)


SAMPLE_CUBES = [(8, 4), (5, 3), (1, 1), (2, 2)]  # (size, levels): a full chain, a size that is no power of two, one texel


def sample_directions(levels):
    """-> directions (n, 3) float32, lods (n,) float32: the six axes, twelve edge and eight corner directions exactly and with
    each non-zero component one ulp either side; directions scaled by 1e30 and 1e-30; taps that leave the face in one axis and
    in both, on every layer; zero and non-finite directions; each at lods 0, two fractions, the last level, beyond it,
    negative and NaN"""
    exact = [np.array(d, F) for d in itertools.product((-1.0, 0.0, 1.0), repeat=3) if any(d)]
    dirs = list(exact)
    for d in exact:
        for k in range(3):
            if d[k] != 0:
                for toward in (0.0, np.inf):
                    e = d.copy()
                    e[k] = np.nextafter(e[k], F(np.sign(e[k]) * np.inf) if toward else F(0.0))
                    dirs.append(e)
    dirs += [d * F(1e30) for d in exact[::3]] + [d * F(1e-30) for d in exact[1::3]]
    for axis in range(3):
        for sign in (-1.0, 1.0):
            for a, b in ((0.2, 0.999), (0.999, -0.3), (-0.999, 0.999), (0.999, 0.999), (-0.999, -0.999), (0.999, -0.999), (0.0, 0.0), (0.93, 0.4)):
                d = np.zeros(3, F)
                d[axis], d[(axis + 1) % 3], d[(axis + 2) % 3] = sign, a, b
                dirs.append(d)
    dirs += [np.array(d, F) for d in ((0, 0, 0), (-0.0, 0, -0.0), (np.nan, 1, 0), (np.inf, 0, 0), (1, -np.inf, 2), (0, 0, np.nan))]
    lods = [0.0, 0.5, 1.25, float(levels - 1), float(levels + 3), -1.0, np.nan, levels - 1.5]
    d = np.repeat(np.stack(dirs), len(lods), axis=0)
    return np.ascontiguousarray(d, F), np.tile(np.array(lods, F), len(dirs))
