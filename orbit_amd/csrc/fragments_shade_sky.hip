// fragments_shade_sky.hip — orbit_fragments_shade_sky (include/orbit_abi_ext.h K1-K10 on top of H1-H10 and L1-L9, DESIGN.md
// §4.31): orbit_fragments_shade_shadowed with the SKY lights served from the environment's three images and the uncovered
// pixels filled from the sky cube.  The arithmetic is shade_common.h's, shadow_common.h's, env_common.h's and
// sky_common.h's, shared with the host mirror, which is the pin.
//
// Two or three launches on the stream, no look-back, no spinning, nothing handed between workgroups:
//   clear  shade_walk.h's: also sky_stats = 0
//   shade  shade_walk.h's tile loop and its two forms of the light walk, in SkyTier<ENV>.  Built twice: without the
//          environment it is the shadowed unit's kernel, and a call that gives none pays nothing for K.  With it, K1's branch sits where
//          shadow_pixel_light is called: in the staged form the light is table[k], one row for the wave, so the branch is
//          taken by every lane of the slice or by none; the cube and table gathers are a lane's own (the offsets of a
//          cube's levels are wave-uniform and picked by a select chain: nothing is indexed by a lane's value).
//   box    K9, where sky is given and the mode is 0: the same tiles in the same trips under the same grid cap, the lanes
//          whose visibility word is 0.  A launch of its own: inside the shade launch it cost the lit path 24 VGPRs and
//          with them a wave per SIMD, with or without an environment.
//          The counters are wave-uniform sums: one atomic each per wave at the end.
#include "shade_walk.h"
#include "sky_common.h"

namespace orbit {
namespace {

// the sky tier on the device: H10's and K10's words, H10's planes, both stats blocks.  ENV: the environment is given (K1-K8
// are built in; without it the kernel is the shadowed unit's, instruction for instruction but for sky_stats)
template <bool ENV>
struct SkyDevice : SkyTier<ENV> {
    using typename SkyTier<ENV>::Job;
    using typename SkyTier<ENV>::Extra;
    static constexpr uint32_t kWords = ENV ? kStatWords : kShadowEnd;
    __device__ static void count(uint32_t *count, bool written, const Extra &e) {
        shadow_count(count, written, e.sp);
        if (!ENV) return;
        const uint64_t sky_lit = __ballot(written && e.k.evaluations != 0u);
        if (sky_lit == 0ull) return; // (wave-uniform)
        count[kSkyLit] += (uint32_t)__popcll(sky_lit);
        count[kSkyEvaluations] += wave_sum(written ? e.k.evaluations : 0u); // at most 256 each
        count[kBad] += wave_sum(written ? e.k.bad : 0u);                    // at most 512 each
    }
    __device__ static void store(const Job &j, size_t p, const Extra &e) { shadow_store(j.shadowed, p, e.sp); }
    __device__ static void flush(const Job &j, const uint32_t *count) {
        shadow_flush(j.shadowed, count);
        if (!ENV || !j.sky_stats) return;
        OrbitSkyStats *stats = j.sky_stats;
        if (count[kSkyEvaluations] != 0u) atomicAdd(&stats->sky_evaluations, count[kSkyEvaluations]);
        if (count[kSkyLit] != 0u) atomicAdd(&stats->sky_lit_pixels, count[kSkyLit]);
        if (count[kBad] != 0u) atomicAdd((unsigned long long *)&stats->bad_directions, (unsigned long long)count[kBad]);
    }
};

template <bool STAGED, bool ENV>
__global__ __launch_bounds__(kShadeThreads) void sky_kernel(const OrbitFragmentsShadeSky js, const uint32_t tiles_x, const uint32_t tiles,
                                                            int32_t *status) {
    shade_tiles<SkyDevice<ENV>, STAGED>(js, tiles_x, tiles, status);
}

// K9, the call's last launch where sky is given and the mode is 0: the same tiles in the same trips, the lanes whose
// visibility word is 0.  A pixel is written by this launch or by the one before it, never by both.
__global__ __launch_bounds__(kShadeThreads) void sky_box_kernel(const OrbitFragmentsShadeSky js, const uint32_t tiles_x, const uint32_t tiles) {
    const OrbitFragmentsShade &b = js.shadowed.shade;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t stride = gridDim.x * kShadeWaves;
    uint32_t boxed = 0u, bad = 0u; // wave-uniform
    for (uint32_t tile = blockIdx.x * kShadeWaves + wave; tile < tiles; tile += stride) { // (wave-uniform)
        const uint32_t x = (tile % tiles_x) * 8u + (lane & 7u), y = (tile / tiles_x) * 8u + (lane >> 3);
        const bool in_target = x < b.width && y < b.height;
        const size_t p = (size_t)y * b.width + x;
        const bool open = in_target && b.visibility[in_target ? p : 0u] == 0ull;
        const uint64_t opened = __ballot(open);
        if (opened == 0ull) continue; // (wave-uniform)
        bool good = true;
        if (open) {
            float color[4];
            good = sky_box_pixel(js, x, y, color);
            Words4 r;
            for (int i = 0; i < 4; i++) r.w[i] = (uint32_t)float_bits(color[i]);
            *(Words4 *)(b.color + 4u * p) = r; // (in_target: p lies inside the plane)
        }
        boxed += (uint32_t)__popcll(opened);
        bad += (uint32_t)__popcll(__ballot(open && !good));
    }
    if (lane != 0u || !js.sky_stats) return;
    if (boxed != 0u) atomicAdd(&js.sky_stats->skybox_pixels, boxed);
    if (bad != 0u) atomicAdd((unsigned long long *)&js.sky_stats->bad_directions, (unsigned long long)bad);
}

} // namespace

hipError_t launch_fragments_shade_sky(const OrbitFragmentsShadeSky &job, uint32_t num_cus, uint32_t grid_cap, int32_t *status, hipStream_t s) {
    const OrbitFragmentsShadeShadowed &j = job.shadowed;
    const ShadeGrid g = shade_grid(j.shade, num_cus, grid_cap);
    hipError_t e = launch_shade_clear(j.shade, j.shadow_factor, j.cascade, j.shadow_stats, job.sky_stats, g.cap, s);
    if (e != hipSuccess) return e;
    if (sky_env_given(job)) e = launch_shade_tiles(sky_kernel<true, true>, sky_kernel<false, true>, job, g, status, s);
    else e = launch_shade_tiles(sky_kernel<true, false>, sky_kernel<false, false>, job, g, status, s);
    if (e != hipSuccess || !sky_box_given(job)) return e;
    hipLaunchKernelGGL(sky_box_kernel, dim3(g.blocks), dim3(kShadeThreads), 0, s, job, g.tiles_x, g.tiles);
    return hipGetLastError();
}

} // namespace orbit
