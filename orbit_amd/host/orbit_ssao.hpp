// orbit_ssao.hpp — host mirror of orbit_ssao (include/orbit_abi_ext.h A1-A9) on HOST copies of the same
// buffers, sequential: the obvious loops over the pixels, each through ../csrc/ssao_common.h, which the kernels share.  It
// is the reference of the GPU tests: the same bytes of raw, blurred and ao_pixel, the same counters.
#pragma once
#include <cstdint>

#include "../../include/orbit_abi_ext.h"

namespace orbit {
namespace raster {

// The job's pointers are HOST pointers.  Throws Panic for what the device call answers with ORBIT_E_INVALID.  census (may
// be null): 19 counters over every pixel and sample — pixels by A2's branch (right + up, right + down, left + up, left +
// down), samples in range, out of range, occluded, not occluded, with range_check strictly inside (0, 1), exactly 0,
// exactly 1, NaN, and with sample_depth == proj.z, then pixels whose horizontal and whose vertical |dz| tie, then in-range
// samples with a component exactly 0 and exactly 1 and rejected samples with a component one step below 0 and above 1.
void ssao(const OrbitSsao &job, uint64_t *census = nullptr);

// tests: A4's table of sample_count entries of four floats (direction, radius)
void ssao_table(const uint8_t *samples, uint32_t samples_size, uint32_t sample_count, float min_radius, float max_radius, float *table);
// tests: A5's range test of n triples (1 = in range) and its range_check of n (min_radius, sample_depth, proj.w) triples
void ssao_in_range_array(const float *proj, uint64_t n, uint8_t *out);
void ssao_range_check_array(const float *args, uint64_t n, float *out);

} // namespace raster
} // namespace orbit
