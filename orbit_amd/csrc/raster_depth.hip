// raster_depth.hip — orbit_raster_depth (include/orbit_abi_ext.h): the reference's depth prepass
// (forward_depth_prepass.mesh / .vert + fixed-function raster, forward.rs:300-356) in compute, from the draw commands
// the meshlet cull wrote.  The host mirror is the pin: the depth bytes and the counters equal orbit_host_raster_depth's
// for every input.
//
// The raster kernel is the walker of raster_walk.h over a sink that writes depth by atomicMax on the u32 view (positive
// floats order as their bits), behind a relaxed atomic load that skips the atomic where the buffer already holds as
// much: the buffer only grows, so a stale smaller value costs an atomic, never a pixel.
#include "raster_walk.h"

#ifndef ORBIT_RASTER_VARIANT // raster_depth_clip.hip and raster_depth_wide.hip compile this file with theirs
#define ORBIT_RASTER_VARIANT Plain
#endif
// the variant's kernel, under the name the profiles know it by
#define ORBIT_RASTER_KERNEL_Plain raster_depth_kernel
#define ORBIT_RASTER_KERNEL_ClipNear raster_depth_clip_kernel
#define ORBIT_RASTER_KERNEL_Wide raster_depth_wide_kernel
#define ORBIT_RASTER_DEPTH_KERNEL ORBIT_RASTER_PASTE(ORBIT_RASTER_KERNEL_, ORBIT_RASTER_VARIANT)

namespace orbit {
namespace {

using namespace raster;

// R7, R8 of one inside sample -> it is a fragment (d > 0)
struct DepthSink {
    static constexpr uint32_t kMaxTriangles = ~0u; // no limit: the depth word carries no triangle index
    uint32_t *depth;
    template <class AnySetup> // Setup (R7) or SetupW (R7w)
    __device__ __forceinline__ bool write(const AnySetup &s, int32_t x, int32_t y, uint32_t width, uint32_t /*id*/) const {
        const float d = depth_at(s, 256 * x + 128, 256 * y + 128);
        if (!(d > 0.0f)) return false;
        const uint32_t bits = __float_as_uint(d);
        uint32_t *dst = depth + (size_t)y * width + (uint32_t)x;
        // (a relaxed load beside the other waves' atomics: a stale value is a smaller one and costs an atomic, never a pixel)
        if (bits > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dst, bits);
        return true;
    }
};

constexpr RasterVariant kVariant = RasterVariant::ORBIT_RASTER_VARIANT;

__global__ __launch_bounds__(kRasterThreads) void ORBIT_RASTER_DEPTH_KERNEL(const RasterParams p, uint32_t *const depth) {
    raster_commands<kVariant>(p, DepthSink{depth}, 0u);
}

} // namespace

template <>
uint32_t raster_depth_blocks_per_cu<kVariant>() {
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, ORBIT_RASTER_DEPTH_KERNEL, (int)kRasterThreads, 0);
    return e == hipSuccess && n > 0 ? (uint32_t)n : 2u;
}

template <>
hipError_t launch_raster_depth<kVariant>(const OrbitRasterDepth &job, uint32_t resident_blocks, int32_t *status, hipStream_t s) {
    return launch_raster(ORBIT_RASTER_DEPTH_KERNEL, job, (uint32_t *)job.depth, resident_blocks, status, s, (uint32_t *)job.depth);
}

} // namespace orbit
