"""Generates tests/golden/spirv_bloom.npz: inputs and OUTPUTS OF THE REFERENCE'S OWN COMPILED bloom/bloom_downsample.comp.spv
with mip_level >= 1, executed by oracle/spirv_vm.py.

Run after build() has copied the reference's binaries (oracle/Makefile `ref`; it reads
oracle/_ref/shaders/bloom/bloom_downsample.comp.spv, which does not travel): `python tests/golden/make_spirv_bloom.py`.

What the binary decides: which invocations write, the 13 coordinates in its own arithmetic, the five groups, their weights
and the order of every sum, one imageStore per texel.  What it is handed: the sampler — rule B3 of include/orbit_abi_ext.h
(LinearClamp in fp32 as written: the project's canonical choice, hardware filters in fixed point), restated in
tests/post_chain_ref.py — over source texels that are exactly representable in B10G11R11 (unpacked random words).  With
mip_level = 0 the interpreter stops at GLSL.std.450 Pow, and bloom_upsample.comp.spv needs OpImageRead, which it does not
list: level 0 and the upsample are not pinned by the binary.

Per case `WxH->wxh/`: src (H, W, 3) float32, spv_dst (h, w, 3) float32: the floats the binary passed to imageStore.
The test that consumes the file: tests/test_post_chain_cpu.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import post_chain_ref as ref  # noqa: E402
from oracle import spirv_vm as vm  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "shaders", "")
F = np.float32
SHAPES = (((10, 6), (5, 3)), ((7, 5), (3, 2)), ((1, 9), (1, 4)), ((33, 17), (16, 8)), ((2, 2), (1, 1)))  # source -> destination


def source(seed, w, h):
    """Random B10G11R11 texels, unpacked: small and large exponents, zeros, a few subnormals; nothing non-finite"""
    rng = np.random.default_rng(seed)
    e = rng.integers(8, 22, (h, w, 3)).astype(np.uint32)  # 2^-7 .. 2^6
    e[rng.random((h, w, 3)) < 0.05] = 0  # subnormal or zero
    r = (e[..., 0] << 6) | rng.integers(0, 64, (h, w)).astype(np.uint32)
    g = (e[..., 1] << 6) | rng.integers(0, 64, (h, w)).astype(np.uint32)
    b = (e[..., 2] << 5) | rng.integers(0, 32, (h, w)).astype(np.uint32)
    return ref.unpack((r | (g << 11) | (b << 22)).astype(np.uint32))


def run_case(mod, src, dst_w, dst_h, mip_level=1):
    h, w = src.shape[:2]
    dst = np.full((dst_h, dst_w, 3), np.nan, F)  # every texel must be written exactly once
    calls = [0]

    def sample(img, smp, u, v, lod):
        assert float(lod) == 0.0
        calls[0] += 1
        rgb = ref.sample(src, np.array([u], F), np.array([v], F), F)[0, 0]
        return np.array([rgb[0], rgb[1], rgb[2], 1.0], F)

    def write(x, y, texel):
        assert np.isnan(dst[y, x]).all(), "a texel written twice"
        dst[y, x] = texel[:3]

    push = np.zeros(36, np.uint8)  # uvec2 image_size; uint input_image, output_image; vec4 threshold_filter; uint mip_level
    push[:16].view(np.uint32)[:] = (dst_w, dst_h, 1, 2)
    push[16:32].view(F)[:] = (1.0, 0.5, 1.0, 0.5)  # not read with mip_level >= 1
    push[32:36].view(np.uint32)[:] = mip_level
    vm.Machine(mod, {}, push.tobytes(), None, images={1: {"size": lambda lod: (w, h)}, 2: {"write": write}},
               samplers={k: {"id": k} for k in range(8)}, sample=sample, subgroup=32).run(((dst_w + 7) // 8, (dst_h + 7) // 8))
    assert not np.isnan(dst).any(), "a texel of the level was not written"
    assert calls[0] == 13 * dst_w * dst_h, calls[0]
    return dst


def main():
    mod = vm.Module(REF + "bloom/bloom_downsample.comp.spv")
    out = {}
    for seed, ((w, h), (dw, dh)) in enumerate(SHAPES, 31):
        src = source(seed, w, h)
        dst = run_case(mod, src, dw, dh, mip_level=1 + seed % 3)
        out[f"{w}x{h}->{dw}x{dh}/src"], out[f"{w}x{h}->{dw}x{dh}/spv_dst"] = src, dst
        print("bloom downsample %2dx%-2d -> %2dx%-2d: %d texels, 13 samples each" % (w, h, dw, dh, dw * dh))
    np.savez_compressed(os.path.join(HERE, "spirv_bloom.npz"), **out)


if __name__ == "__main__":
    main()
