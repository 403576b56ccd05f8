// orbit_env_map.hpp — host mirror of orbit_env_map and orbit_env_sample (include/orbit_abi_ext.h E0-E12)
// on HOST copies of the same buffers, sequential: the obvious loops over the texels, each through ../csrc/env_common.h,
// which the kernels share.  It is the reference of the GPU tests: the same bytes of every product, the same counters.
#pragma once
#include <cstdint>

#include "../../include/orbit_abi_ext.h"

namespace orbit {
namespace raster {

// The job's pointers are HOST pointers.  Throws Panic for what the device call answers with ORBIT_E_INVALID.  census (may
// be null): ORBIT_HOST_ENV_CENSUS counters, added to, not cleared (orbit_host_c.h names them).
void env_map(const OrbitEnvMap &job, uint64_t *census = nullptr);
void env_sample_job(const OrbitEnvSample &job, uint64_t *census = nullptr);

// tools: `count` texels of level m of the job's prefiltered cube (indices face * n * n + py * n + px) from the job's sky
// cube, which must hold the cube already; out: count texels.  The job's prefiltered pointer is not written.
void env_prefilter_texels(const OrbitEnvMap &job, uint32_t m, const uint32_t *texels, uint32_t count, uint16_t *out);

// tests: E1 of one texel, and the routines over n values (which = 0: atan2c(a, b), 1: asinc(a), 2 / 3: sine / cosine, 4: E0's stored
// half of a, back as a float, NaN where a is not finite)
void env_direction(uint32_t face, uint32_t px, uint32_t py, uint32_t n, float *out);
void env_routines(uint32_t which, const float *a, const float *b, uint64_t n, float *out);

} // namespace raster
} // namespace orbit
