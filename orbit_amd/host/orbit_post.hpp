// orbit_post.hpp — host mirror of orbit_bloom and orbit_post_process (include/orbit_abi_ext.h B1-B9 and T1-T5, DESIGN.md
// §4.27) on HOST copies of the same buffers, sequential: the obvious loops over the levels and the texels, each texel
// through ../csrc/post_common.h, which the kernels share.  It is the reference of the GPU tests: the same bytes of mips,
// ldr and rgba8, the same counters.
#pragma once
#include <cstdint>

#include "../../include/orbit_abi_ext.h"

namespace orbit {
namespace raster {

// The job's pointers are HOST pointers; the form flags are checked and change nothing.  Throws Panic for what the device
// call answers with ORBIT_E_INVALID.
void bloom(const OrbitBloom &job);
void post_process(const OrbitPostProcess &job);

// tests: one downsample (B3-B5) of src_w x src_h x 3 floats into dst_w x dst_h x 3 floats, nothing packed; level0: with
// B5 under the threshold vector tf[4].  What the reference's binary computes between its samples and its imageStore.
void bloom_downsample_floats(const float *src, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h, bool level0,
                             const float *tf, float *dst);
// tests: B6's result (what is added to the destination) of one upsample, floats in and out as above
void bloom_upsample_floats(const float *src, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h, float filter_radius,
                           float *dst);
// tests: B7 of n texels; clamped (may be null): 1 where a component was at or above the largest finite value
void bloom_pack_texels(const float *rgb, uint64_t n, uint32_t *words, uint8_t *clamped);
void bloom_unpack_texels(const uint32_t *words, uint64_t n, float *rgb);
// tests: powc(x[i], y) of B5 and T4
void powc_array(const float *x, uint64_t n, float y, float *out);

} // namespace raster
} // namespace orbit
