// fragments_shade.hip — orbit_fragments_shade (include/orbit_abi_ext.h L1-L9): from a visibility buffer,
// the planes orbit_surface_fragments left, the material and light tables and the cluster chain's light lists to the
// colour of every visible pixel.  The arithmetic is shade_common.h's, shared with the host mirror, which is the pin; the
// slice comes through orbit_device.h's depth_slice, the mark stage's own function.  The two launches, the two forms of the
// light walk and the tile loop are shade_walk.h's, in ShadeTier; the clear serves the two calls on top of this one too.
#include "shade_walk.h"

namespace orbit {
namespace {

// the plain tier on the device: no word, plane or stats block beyond the base job's
struct ShadeDevice : ShadeTier {
    static constexpr uint32_t kWords = kBaseWords;
    __device__ static void count(uint32_t *, bool, const Extra &) {}
    __device__ static void store(const Job &, size_t, const Extra &) {}
    __device__ static void flush(const Job &, const uint32_t *) {}
};

template <bool STAGED>
__global__ __launch_bounds__(kShadeThreads) void shade_kernel(const OrbitFragmentsShade j, const uint32_t tiles_x, const uint32_t tiles,
                                                              int32_t *status) {
    shade_tiles<ShadeDevice, STAGED>(j, tiles_x, tiles, status);
}

// L9, H10, K10: a NULL pointer is a plane not filled or a block not kept
__global__ __launch_bounds__(kShadeThreads) void shade_clear_kernel(uint32_t *color, uint32_t *lights_walked, uint32_t *shadow_factor,
                                                                    uint32_t *cascade, const size_t pixels, uint32_t *stats,
                                                                    uint32_t *shadow_stats, uint32_t *sky_stats) {
    const size_t stride = (size_t)gridDim.x * kShadeThreads, first = (size_t)blockIdx.x * kShadeThreads + threadIdx.x;
    if (stats && first < kBaseWords) stats[first] = 0u;
    if (shadow_stats && first < kShadowEnd - kBaseWords) shadow_stats[first] = 0u;
    if (sky_stats && first < sizeof(OrbitSkyStats) / 4u) sky_stats[first] = 0u;
    if (color)
        for (size_t i = first; i < 4u * pixels; i += stride) color[i] = 0u;
    if (lights_walked)
        for (size_t i = first; i < pixels; i += stride) lights_walked[i] = 0u;
    if (shadow_factor)
        for (size_t i = first; i < pixels; i += stride) shadow_factor[i] = 0x3F800000u; // 1.0f
    if (cascade)
        for (size_t i = first; i < pixels; i += stride) cascade[i] = kNone;
}

} // namespace

hipError_t launch_shade_clear(const OrbitFragmentsShade &b, float *shadow_factor, uint32_t *cascade, OrbitShadowStats *shadow_stats,
                              OrbitSkyStats *sky_stats, uint32_t cap, hipStream_t s) {
    const size_t pixels = (size_t)b.width * b.height; // width, height <= 32768: at most 2^30
    const bool fill = (b.flags & ORBIT_SHADE_CLEAR) != 0u;
    if (!fill && !b.stats && !shadow_stats && !sky_stats) return hipSuccess;
    const size_t need = fill ? (4u * pixels + kShadeThreads * 4u - 1u) / (kShadeThreads * 4u) : 1u;
    hipLaunchKernelGGL(shade_clear_kernel, dim3((uint32_t)(need < cap ? need : cap)), dim3(kShadeThreads), 0, s,
                       fill ? (uint32_t *)b.color : nullptr, fill ? b.lights_walked : nullptr, fill ? (uint32_t *)shadow_factor : nullptr,
                       fill ? cascade : nullptr, pixels, (uint32_t *)b.stats, (uint32_t *)shadow_stats, (uint32_t *)sky_stats);
    return hipGetLastError();
}

hipError_t launch_fragments_shade(const OrbitFragmentsShade &job, uint32_t num_cus, uint32_t grid_cap, int32_t *status, hipStream_t s) {
    const ShadeGrid g = shade_grid(job, num_cus, grid_cap);
    const hipError_t e = launch_shade_clear(job, nullptr, nullptr, nullptr, nullptr, g.cap, s);
    if (e != hipSuccess) return e;
    return launch_shade_tiles(shade_kernel<true>, shade_kernel<false>, job, g, status, s);
}

} // namespace orbit
