"""orbit_bloom's and orbit_post_process' host mirrors (orbit_amd.post.host_bloom / host_post_process, the device calls' pin;
include/orbit_abi_ext.h B1-B9 and T1-T5) against the numpy restatement of the rules
(tests/post_chain_ref.py), byte for byte, on the hand-built cases of tests/post_chain_cases.py; the downsample against what
the reference's own binary passed to imageStore (tests/golden/spirv_bloom.npz, bit for bit: coordinates, taps, weights, sum
order, which invocations write); the B10G11R11 pack and unpack over every code and its neighbours; the layout; the argument
errors; non-finite inputs; and, MEASURED against the GLSL in float64 with a true pow, the error of powc and the share of
packed texels and of rgba8 bytes that differ (held at the measured value plus one unit of its last printed digit;
profiles/post_chain_cpu.json keeps the figures).  No GPU.

Of B7's "all codes round-trip": the 32 x 64 (32 x 32) codes with exponent 31 are infinities and NaNs, which B8 stores as 0,
so they decode to non-finite values and encode to 0; every other code round-trips."""
import math
import os

import numpy as np
import pytest

import post_chain_cases as pc
import post_chain_ref as ref
from orbit_amd import _lib, passes, post
from orbit_amd import layouts as L

F = np.float32
FILL = 0xA5A5A5A5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spirv_bloom.npz")
RADII = (0.0, 0.003, 0.025)
# measured (tools/render_frame.py writes them to profiles/post_chain_cpu.json), plus one unit of the last printed digit
POWC_22_MAX_REL, POWC_24_MAX_REL = 6.65e-7 + 0.01e-7, 2.71e-7 + 0.01e-7
TEXEL_SHARE, BYTE_SHARE = 0.0395 + 0.0001, 3.9e-6 + 0.1e-6


def stats_equal(got, want):
    return all(int(got[k]) == int(v) for k, v in want.items())


# -- 1. mirror = restatement, byte for byte, between guards
@pytest.mark.parametrize("radius", RADII)
def test_the_bloom_mirror_equals_the_restatement(radius):
    clamped = nonfinite = 0
    for name, color, settings in pc.all_cases():
        for max_levels in (1, 2, 6):
            got = post.host_bloom(color, filter_radius=radius, max_levels=max_levels, fill=FILL, guard=4, **settings)
            want = ref.bloom(color, filter_radius=radius, max_levels=max_levels, **settings)
            n = want["layout"]["total_texels"]
            diff = np.flatnonzero(got["mips"][:n] != want["mips"])
            assert len(diff) == 0, f"{name} r={radius} levels<={max_levels}: {len(diff)} texels differ, first {diff[0]}: {got['mips'][diff[0]]:#x} != {want['mips'][diff[0]]:#x}"
            assert (got["mips"][n:] == FILL).all(), f"{name}: the words behind the chain were written"
            assert stats_equal(got["stats"], want["stats"]), f"{name}: {got['stats']} != {want['stats']}"
            assert np.isfinite(post.host_unpack(got["mips"][:n])).all()  # B8: no non-finite bytes
            clamped += int(got["stats"]["clamped_texels"])
            nonfinite += int(got["stats"]["nonfinite_inputs"])
    assert clamped > 0 and nonfinite > 0  # the census reaches what it is there for


@pytest.mark.parametrize("render_mode,with_bloom,bgra", [(0, False, False), (0, True, False), (8, True, False), (0, True, True), (8, False, True)])
def test_the_post_process_mirror_equals_the_restatement(render_mode, with_bloom, bgra):
    bloomed = 0
    for name, color, settings in pc.all_cases():
        mips = post.host_bloom(color, **settings)["mips"] if with_bloom else None
        for exposure, intensity in ((1.0, 0.025), (2.5, 1.0)):
            got = post.host_post_process(color, mips, exposure, intensity, render_mode, bgra, fill=FILL)
            want = ref.post_process(color, mips, exposure, intensity, render_mode, bgra)
            assert np.array_equal(got["ldr"].view(np.uint32), want["ldr"].view(np.uint32)), name
            assert np.array_equal(got["rgba8"], want["rgba8"]), name
            assert stats_equal(got["stats"], want["stats"]), f"{name}: {got['stats']} != {want['stats']}"
            assert (got["ldr"][..., 3] == 1.0).all() and (got["rgba8"][..., 3] == 255).all() and np.isfinite(got["ldr"]).all()
            bloomed += int(got["stats"]["bloom_pixels"])
    assert (bloomed > 0) == (with_bloom and render_mode == 0)  # T2: mode 8 takes the same path without bloom


def test_each_output_alone_and_the_byte_order():
    color = pc.image("random", 17, 9)
    mips = post.host_bloom(color)["mips"]
    both = post.host_post_process(color, mips, fill=FILL)
    only_ldr = post.host_post_process(color, mips, want_rgba8=False, want_stats=False)
    only_bytes = post.host_post_process(color, mips, want_ldr=False)
    assert only_ldr["rgba8"] is None and only_ldr["ldr"].tobytes() == both["ldr"].tobytes()
    assert only_bytes["ldr"] is None and only_bytes["rgba8"].tobytes() == both["rgba8"].tobytes()
    bgra = post.host_post_process(color, mips, bgra=True)
    assert np.array_equal(bgra["rgba8"][..., [2, 1, 0, 3]], both["rgba8"]) and len(np.unique(both["rgba8"][..., :3])) > 50


# -- 2. the downsample against the reference's binary
def test_the_downsample_equals_the_reference_binary():
    data = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in data.files})
    assert names == sorted(["10x6->5x3", "7x5->3x2", "1x9->1x4", "33x17->16x8", "2x2->1x1"])
    for name in names:
        src, want = data[name + "/src"], data[name + "/spv_dst"]
        dh, dw = want.shape[:2]
        got = post.host_downsample_floats(src, dw, dh)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), f"{name}: the mirror's floats differ from the binary's"
        again = ref.downsample(src, dw, dh)
        assert again.view(np.uint32).tolist() == want.view(np.uint32).tolist(), f"{name}: the restatement differs from the binary's"
        assert len(np.unique(want)) > want.size // 4  # a real image, not a constant


# -- 3. B7, exhaustively
@pytest.mark.parametrize("mant,channel", [(6, 0), (6, 1), (5, 2)])
def test_pack_and_unpack_over_every_code(mant, channel):
    shift = (0, 11, 22)[channel]
    codes = np.arange(1 << (5 + mant), dtype=np.uint32)
    rgb = post.host_unpack(codes << np.uint32(shift))
    value = rgb[:, channel]
    finite = (codes >> mant) != 31
    restated = ref.decode(codes, mant)
    assert np.array_equal(value[finite].view(np.uint32), restated[finite].view(np.uint32))
    assert np.array_equal(np.isnan(value), np.isnan(restated)) and np.array_equal(np.isinf(value), np.isinf(restated))
    others = np.delete(rgb, channel, axis=1)
    assert (others == 0).all()
    assert np.isfinite(value[finite]).all() and not np.isfinite(value[~finite]).any()
    assert (np.diff(value[finite]) > 0).all()  # decode is strictly increasing over the finite codes
    step = 2.0 ** -(14 + mant)
    assert value[1] == step and value[finite][-1] == (65024.0 if mant == 6 else 64512.0)

    def encode(v):
        full = np.zeros((len(v), 3), F)
        full[:, channel] = v
        words, clamped = post.host_pack(full)
        want_words, want_clamped = ref.pack(full)
        assert np.array_equal(words, want_words) and np.array_equal(clamped, want_clamped)
        assert (words & ~np.uint32(((1 << (5 + mant)) - 1) << shift) == 0).all()
        return words >> np.uint32(shift), clamped

    got, clamped = encode(value)  # every finite code round-trips; infinities and NaNs are stored as 0 (B8)
    assert np.array_equal(got[finite], codes[finite]) and (got[~finite] == 0).all()
    top = codes[finite][-1]
    assert clamped[top] and not clamped[:top].any()  # at the largest finite value: that value, counted
    v = value[finite]
    below, _ = encode(np.nextafter(v, F(-np.inf)))  # one ulp below a code's value: the code before (truncation)
    assert np.array_equal(below[1:], codes[finite][:-1]) and below[0] == 0
    above, c_above = encode(np.nextafter(v, F(np.inf)))  # one ulp above: still the code
    assert np.array_equal(above, codes[finite]) and c_above[top] and not c_above[:top].any()
    big = F(65024.0 if mant == 6 else 64512.0)
    edge = np.array([0.0, -0.0, -1.0, -1e-30, np.nextafter(F(step), F(0)), big, np.nextafter(big, F(0)), np.nextafter(big, F(np.inf)), 1e6, 3.4e38,
                     np.inf, -np.inf, np.nan, 1e-45], F)
    got, clamped = encode(edge)
    assert got.tolist() == [0, 0, 0, 0, 0, top, top - 1, top, top, top, 0, 0, 0, 0]
    assert clamped.tolist() == [False] * 5 + [True, False, True, True, True] + [False] * 4


# -- 4. the layout
@pytest.mark.parametrize("size,levels", [((1, 1), 1), ((2, 1), 2), ((1, 40), 6), ((5, 3), 3), ((64, 64), 6), ((70, 33), 6), ((1920, 1080), 6)])
def test_the_layout(size, levels):
    w, h = size
    got, want = post.bloom_layout(w, h), ref.layout(w, h)
    assert got == want and got["levels"] == levels and got["sizes"][0] == (w, h) and got["offsets"][0] == 0
    for k in range(1, levels):
        assert got["sizes"][k] == (max(w >> k, 1), max(h >> k, 1))
        assert got["offsets"][k] == got["offsets"][k - 1] + got["sizes"][k - 1][0] * got["sizes"][k - 1][1]
    for cap in (1, 2):
        short = post.bloom_layout(w, h, cap)
        assert short == ref.layout(w, h, cap) and short["levels"] == min(levels, cap)
    assert post.bloom_layout(w, h, 0) == got  # 0 = the default, 6
    for bad in ((0, 1, 6), (1, 0, 6), (_lib.RASTER_MAX_DIM + 1, 1, 6), (4, 4, 7)):
        with pytest.raises(_lib.OrbitError, match="bloom_layout"):
            post.bloom_layout(*bad)
    assert post.bloom_layout(_lib.RASTER_MAX_DIM, _lib.RASTER_MAX_DIM)["total_texels"] == sum((32768 >> k) ** 2 for k in range(6))


# -- 5. against the GLSL in float64 with a true pow: measured, then held
def bits_range(lo, hi, stride):
    a, b = np.array([lo, hi], F).view(np.uint32)
    return np.arange(int(a), int(b) + 1, stride, dtype=np.uint32).view(F)


def measure_powc():
    out = {}
    for key, lo, hi, y, stride in (("powc_1_2.2_max_rel_error", 2.0 ** -20, 65504.0, 1 / 2.2, 257), ("powc_1_2.4_max_rel_error", 0.0031308, 1.0, 1 / 2.4, 61)):
        x = bits_range(lo, hi, stride)
        got = post.host_powc(x, F(y))
        assert np.array_equal(got, ref.powc(x, F(y)))  # the restated log2c and exp2c are the mirror's, bit for bit
        want = np.power(x.astype(np.float64), np.float64(F(y)))
        out[key] = float((np.abs(got.astype(np.float64) - want) / want).max())
    return out


def measure_shares():
    texels, bytes_ = [0, 0], [0, 0]
    for name, color, settings in pc.all_cases():
        got = post.host_bloom(color, **settings)
        want = ref.bloom(color, T=np.float64, power=ref.pow64, **settings)
        texels[0] += int((got["mips"] != want["mips"]).sum())
        texels[1] += got["mips"].size
        img = post.host_post_process(color, got["mips"])["rgba8"]
        img64 = ref.post_process(color, got["mips"], T=np.float64, power=ref.pow64)["rgba8"]
        assert np.abs(img.astype(int) - img64.astype(int)).max() <= 1, name
        bytes_[0] += int((img != img64).sum())
        bytes_[1] += img.size
    return dict(texel_share_differing=texels[0] / texels[1], texels=texels[1], byte_share_differing=bytes_[0] / bytes_[1], bytes=bytes_[1])


def test_powc_against_float64():
    m = measure_powc()
    print(f"powc: largest relative error {m['powc_1_2.2_max_rel_error']:.3g} (y = 1 / 2.2 over [2^-20, 65504]), "
          f"{m['powc_1_2.4_max_rel_error']:.3g} (y = 1 / 2.4 over [0.0031308, 1])")
    assert m["powc_1_2.2_max_rel_error"] <= POWC_22_MAX_REL and m["powc_1_2.4_max_rel_error"] <= POWC_24_MAX_REL
    assert post.host_powc(np.array([0.0, -0.0, -1.0, np.nan, -np.inf], F), 0.5).tolist() == [0.0] * 5  # B5: x <= 0 is 0
    assert post.host_powc(np.array([1.0], F), 1 / 2.4)[0] == 1.0


def test_the_chain_against_float64():
    m = measure_shares()
    print(f"against the GLSL in float64: {m['texel_share_differing']:.3g} of {m['texels']} packed texels differ, "
          f"{m['byte_share_differing']:.2g} of {m['bytes']} rgba8 bytes (by 1 at most)")
    assert m["texel_share_differing"] <= TEXEL_SHARE and m["byte_share_differing"] <= BYTE_SHARE
    # the pieces, level 0 and the upsample on floats, nothing packed in between: relative to the level's largest value
    color = pc.image("random", 33, 31)
    tf = post.threshold_filter(0.25, 1.0)
    assert np.array_equal(tf, np.array(ref.threshold_filter(0.25, 1.0), F))
    rgb = color[..., :3]
    for got, want in ((post.host_downsample_floats(rgb, 33, 31, True, tf), ref.downsample(rgb, 33, 31, True, tf, np.float64, ref.pow64)),
                      (post.host_upsample_floats(rgb, 66, 62, 0.003), ref.upsample_term(rgb, 66, 62, 0.003, np.float64))):
        assert np.abs(got - want).max() <= 4e-6 * np.abs(want).max()  # a few fp32 roundings of sums of 13 (9) taps of four texels


# -- 6. what the device answers with ORBIT_E_INVALID
def test_the_argument_errors():
    color = pc.image("random", 8, 4)

    def bloom_job(**kw):
        j = _lib.Bloom()
        mips, stats = np.zeros(64, np.uint32), np.zeros(1, L.BLOOM_STATS)
        keep = (color, mips, stats)
        j.color, j.mips, j.stats = color.ctypes.data, mips.ctypes.data, stats.ctypes.data
        _lib.fill_bloom(j, 8, 4, 0.0, 0.0, 0.003, 6, None)
        for k, v in kw.items():
            setattr(j, k, v)
        return j, keep

    import ctypes as C
    j, keep = bloom_job()
    assert passes.lib().orbit_host_bloom(C.byref(j)) == 0
    bad = [dict(color=None), dict(mips=None), dict(color=color.ctypes.data + 4), dict(mips=keep[1].ctypes.data + 2), dict(stats=keep[2].ctypes.data + 1),
           dict(width=0), dict(height=0), dict(width=_lib.RASTER_MAX_DIM + 1), dict(height=_lib.RASTER_MAX_DIM + 1), dict(max_levels=0),
           dict(max_levels=7), dict(threshold=-1.0), dict(threshold=math.nan), dict(soft_threshold=math.inf), dict(soft_threshold=-0.5),
           dict(filter_radius=-0.001), dict(filter_radius=math.inf), dict(flags=2), dict(flags=8), dict(flags=1 << 31),
           dict(mips=color.ctypes.data)]
    for kw in bad:
        j, keep = bloom_job(**kw)
        assert passes.lib().orbit_host_bloom(C.byref(j)) == passes.HOST_PANIC, kw
        assert passes.lib().orbit_host_last_error().decode().startswith("bloom:"), kw
    assert passes.lib().orbit_host_bloom(None) == passes.HOST_PANIC
    for flags in (_lib.BLOOM_FORCE_PER_LEVEL, _lib.BLOOM_FORCE_DIRECT, _lib.BLOOM_FORCE_PER_LEVEL | _lib.BLOOM_FORCE_DIRECT):
        j, keep = bloom_job(flags=flags)
        assert passes.lib().orbit_host_bloom(C.byref(j)) == 0

    def post_job(**kw):
        j = _lib.PostProcess()
        bloom, ldr, rgba8, stats = np.zeros(32, np.uint32), np.zeros((4, 8, 4), F), np.zeros((4, 8, 4), np.uint8), np.zeros(1, L.POST_STATS)
        keep = (color, bloom, ldr, rgba8, stats)
        j.color, j.bloom, j.ldr, j.rgba8, j.stats = (a.ctypes.data for a in keep)
        _lib.fill_post_process(j, 8, 4, 1.0, 0.025, 0, False)
        for k, v in kw.items():
            setattr(j, k, v)
        return j, keep

    j, keep = post_job()
    assert passes.lib().orbit_host_post_process(C.byref(j)) == 0
    for ok in (dict(bloom=None), dict(ldr=None), dict(rgba8=None), dict(stats=None), dict(render_mode=8), dict(flags=_lib.POST_BGRA)):
        j, keep = post_job(**ok)
        assert passes.lib().orbit_host_post_process(C.byref(j)) == 0, ok
    _, k0 = post_job()
    bad = [dict(color=None), dict(ldr=None, rgba8=None), dict(color=color.ctypes.data + 8), dict(ldr=k0[2].ctypes.data + 4),
           dict(bloom=k0[1].ctypes.data + 2), dict(rgba8=k0[3].ctypes.data + 1), dict(stats=k0[4].ctypes.data + 2), dict(width=0), dict(height=0),
           dict(width=_lib.RASTER_MAX_DIM + 1), dict(render_mode=7), dict(render_mode=1), dict(exposure=math.nan), dict(exposure=math.inf),
           dict(bloom_intensity=-math.inf), dict(flags=2), dict(ldr=color.ctypes.data), dict(rgba8=k0[1].ctypes.data), dict(rgba8=k0[2].ctypes.data)]
    for kw in bad:
        j, keep = post_job(**kw)
        if "rgba8" in kw and kw["rgba8"] == k0[1].ctypes.data:
            j.bloom = k0[1].ctypes.data
        if "rgba8" in kw and kw["rgba8"] == k0[2].ctypes.data:
            j.ldr = k0[2].ctypes.data
        assert passes.lib().orbit_host_post_process(C.byref(j)) == passes.HOST_PANIC, kw
        assert passes.lib().orbit_host_last_error().decode().startswith("post_process:"), kw
    assert passes.lib().orbit_host_post_process(None) == passes.HOST_PANIC


# -- 7. non-finite inputs, and the default threshold on a black image
def test_non_finite_inputs_are_counted_once_and_never_stored():
    for w, h in ((1, 1), (5, 3), (17, 9), (70, 33)):
        color = pc.image("nonfinite", w, h)
        bad = int((~np.isfinite(color[..., :3])).any(axis=-1).sum())
        assert bad == (1 if (w, h) == (1, 1) else 3)
        got = post.host_bloom(color)
        assert int(got["stats"]["nonfinite_inputs"]) == bad and np.isfinite(post.host_unpack(got["mips"])).all()
        zeroed = color.copy()
        zeroed[..., :3] = np.where(np.isfinite(color[..., :3]), color[..., :3], 0.0)
        assert np.array_equal(post.host_bloom(zeroed)["mips"], got["mips"])  # reads as +0.0f in every tap
        out = post.host_post_process(color, got["mips"])
        assert int(out["stats"]["nonfinite_pixels"]) == bad and np.isfinite(out["ldr"]).all()
        assert np.array_equal(post.host_post_process(zeroed, got["mips"])["rgba8"], out["rgba8"])
    alpha = pc.image("random", 5, 3)
    alpha[..., 3] = np.nan  # alpha is not read
    assert int(post.host_bloom(alpha)["stats"]["nonfinite_inputs"]) == 0 and int(post.host_post_process(alpha)["stats"]["nonfinite_pixels"]) == 0
    huge = pc.image("black", 5, 3)
    huge[1, 2, :3] = 3e38  # finite in, infinite sums of taps on the way: stored as 0 or clamped, never non-finite
    got = post.host_bloom(huge, filter_radius=0.025)
    assert np.isfinite(post.host_unpack(got["mips"])).all() and int(got["stats"]["nonfinite_inputs"]) == 0
    assert np.isfinite(post.host_post_process(huge, got["mips"], bloom_intensity=3e38)["ldr"]).all()


def test_the_default_threshold_on_a_black_image():
    for w, h in ((1, 1), (17, 9), (64, 64)):
        got = post.host_bloom(pc.image("black", w, h))  # threshold = 0: prefilter divides 0 by max(0, 0.00001), not by 0
        assert (got["mips"] == 0).all() and int(got["stats"]["clamped_texels"]) == 0
        lay = got["layout"]
        assert int(got["stats"]["levels"]) == lay["levels"]
        assert int(got["stats"]["texels_written"]) == 2 * lay["total_texels"] - lay["sizes"][-1][0] * lay["sizes"][-1][1]
        out = post.host_post_process(pc.image("black", w, h), got["mips"])
        assert (out["rgba8"][..., :3] == 0).all() and int(out["stats"]["bloom_pixels"]) == 0
