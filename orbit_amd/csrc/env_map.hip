// env_map.hip — orbit_env_map and orbit_env_sample (include/orbit_abi_ext.h E0-E12): the sky cube of an
// equirectangular panorama with its mip chain, the irradiance cube, the prefiltered cube and the BRDF table, as the
// reference makes them at load time, and the cube sampler on its own.  The arithmetic is env_common.h's, shared with the
// host mirror, which is the pin.  Launches, each ordered behind the one before by the stream:
//   clear        one thread writes the counters' start.
//   equirect     a thread per texel of the sky cube's level 0: four panorama texels in, one cube texel out.
//   mip          per level, a thread per texel: four stored texels in, one out (levels as small as 1 x 1).
//   irradiance   a thread per texel, one wave per workgroup: a texel's taps run one after the other in the rule's order, so
//                the launch is as long as one thread; 64-thread workgroups spread its few waves over four times the CUs.
//                Every tap reads the sky cube through E4.
//   prefilter    per level; a 256-thread workgroup takes a 16 x 16 tile of one face (blockIdx.z) and a thread a texel.
//                What depends on the sample and the roughness alone (2 pi Xi.x, cosTheta, sinTheta) is computed once per
//                workgroup and chunk of kChunk samples, one sample per thread, into LDS; what depends on the texel alone
//                (N, the tangent frame, random's phase) is computed once per thread in front of the sample loop.  A
//                thread whose texel lies beyond the face fills the table with the others and stores nothing.
//   brdf         a thread per texel of the table.
//   sample       a thread per direction.
// There is no bordered copy of the faces: a tap outside its face folds over the edge in integers (env_fold), so no launch
// fills a border and the call needs no scratch.  Every cube index comes out of env_tap's clamp-or-fold to 0 .. n - 1 of a
// face 0 .. 5 of a level below `levels`; panorama indices are taken modulo its size.  Counters: a thread adds what it
// counted, if anything, by one 64-bit atomic per counter.
#include "kernels.h"
#include "orbit_device.h"
#include "env_common.h"

namespace orbit {
namespace {

using namespace raster;

constexpr uint32_t kThreads = 256, kTile = 16, kChunk = 256, kIrradianceThreads = 64;

__device__ __forceinline__ void count(uint64_t *counter, uint64_t n) {
    if (counter && n != 0u) atomicAdd((unsigned long long *)counter, (unsigned long long)n);
}
__device__ __forceinline__ void store_texel(uint16_t *dst, size_t texel, const EnvTexel &t) {
    *(EnvTexel *)(dst + 4u * texel) = t; // 8-B aligned: the plane is, by the entry point
}

__global__ void env_clear_kernel(OrbitEnvMapStats *stats) {
    stats->sky_nonfinite = 0u, stats->irradiance_nonfinite = 0u, stats->prefiltered_nonfinite = 0u, stats->brdf_nonfinite = 0u;
    stats->bad_directions = 0u, stats->_pad = 0u;
}
__global__ void env_clear_counter_kernel(uint64_t *counter) { *counter = 0u; }

__global__ __launch_bounds__(kThreads) void env_equirect_kernel(const float *equirect, uint32_t w, uint32_t h, uint16_t *sky, uint32_t n,
                                                                OrbitEnvMapStats *stats) {
    const uint32_t texel = blockIdx.x * kThreads + threadIdx.x; // below 6 * 4096^2 < 2^27
    if (texel >= 6u * n * n) return;
    const uint32_t face = texel / (n * n), py = (texel / n) % n, px = texel % n;
    float rgb[3];
    env_equirect_texel(equirect, w, h, face, px, py, n, rgb);
    EnvTexel t;
    const bool nonfinite = env_store_rgb(rgb, t);
    store_texel(sky, texel, t);
    if (stats) count(&stats->sky_nonfinite, nonfinite ? 1u : 0u);
}

// src, dst: the two levels' first texels; n: the destination's extent, the source's is 2 n
__global__ __launch_bounds__(kThreads) void env_mip_kernel(const uint16_t *src, uint16_t *dst, uint32_t n, OrbitEnvMapStats *stats) {
    const uint32_t texel = blockIdx.x * kThreads + threadIdx.x;
    if (texel >= 6u * n * n) return;
    const uint32_t face = texel / (n * n), y = (texel / n) % n, x = texel % n;
    EnvTexel t;
    const bool nonfinite = env_mip_texel(src + 4u * ((size_t)face * (2u * n) * (2u * n)), 2u * n, x, y, t);
    store_texel(dst, texel, t);
    if (stats) count(&stats->sky_nonfinite, nonfinite ? 1u : 0u);
}

__global__ __launch_bounds__(kIrradianceThreads) void env_irradiance_kernel(const EnvCube sky, float lod, float sample_delta, uint16_t *irradiance,
                                                                            uint32_t n, OrbitEnvMapStats *stats) {
    const uint32_t texel = blockIdx.x * kIrradianceThreads + threadIdx.x;
    if (texel >= 6u * n * n) return;
    const uint32_t face = texel / (n * n), py = (texel / n) % n, px = texel % n;
    float rgb[3];
    uint64_t bad = 0u;
    env_irradiance_texel(sky, lod, sample_delta, face, px, py, n, rgb, bad);
    EnvTexel t;
    const bool nonfinite = env_store_rgb(rgb, t);
    store_texel(irradiance, texel, t);
    if (stats) count(&stats->irradiance_nonfinite, nonfinite ? 1u : 0u), count(&stats->bad_directions, bad);
}

// dst: the level's first texel; n: its extent
__global__ __launch_bounds__(kThreads) void env_prefilter_kernel(const EnvCube sky, const EnvPrefilterLevel level, uint32_t sample_count,
                                                                 uint16_t *dst, uint32_t n, OrbitEnvMapStats *stats) {
    __shared__ float phi0[kChunk], cos_theta[kChunk], sin_theta[kChunk];
    const uint32_t face = blockIdx.z;
    const uint32_t px = blockIdx.x * kTile + (threadIdx.x & (kTile - 1u)), py = blockIdx.y * kTile + threadIdx.x / kTile;
    const bool live = px < n && py < n;
    EnvPrefilterTexel t;
    env_prefilter_begin(face, live ? px : 0u, live ? py : 0u, n, t);
    uint64_t bad = 0u;
    for (uint32_t first = 0u; first < sample_count; first += kChunk) {
        const uint32_t in_chunk = sample_count - first < kChunk ? sample_count - first : kChunk;
        __syncthreads(); // the chunk before has been read by every thread
        if (threadIdx.x < in_chunk) env_ggx_entry(first + threadIdx.x, sample_count, level.roughness, phi0[threadIdx.x], cos_theta[threadIdx.x], sin_theta[threadIdx.x]);
        __syncthreads();
        if (live)
            for (uint32_t i = 0; i < in_chunk; i++)
                if (env_prefilter_sample(sky, level, phi0[i], cos_theta[i], sin_theta[i], t) == 2u) bad++;
    }
    if (!live) return;
    float rgb[3];
    env_prefilter_end(t, rgb);
    EnvTexel out;
    const bool nonfinite = env_store_rgb(rgb, out);
    store_texel(dst, ((size_t)face * n + py) * n + px, out);
    if (stats) count(&stats->prefiltered_nonfinite, nonfinite ? 1u : 0u), count(&stats->bad_directions, bad);
}

__global__ __launch_bounds__(kThreads) void env_brdf_kernel(uint16_t *brdf, uint32_t n, uint32_t sample_count, OrbitEnvMapStats *stats) {
    const uint32_t texel = blockIdx.x * kThreads + threadIdx.x; // below 4096^2
    if (texel >= n * n) return;
    float ab[2];
    env_brdf_texel(texel % n, texel / n, n, sample_count, ab);
    bool nonfinite = false;
    const uint32_t lo = env_half(ab[0], nonfinite), hi = env_half(ab[1], nonfinite);
    ((uint32_t *)brdf)[texel] = lo | (hi << 16); // 4-B aligned by the entry point
    if (stats) count(&stats->brdf_nonfinite, nonfinite ? 1u : 0u);
}

__global__ __launch_bounds__(kThreads) void env_sample_kernel(const EnvCube cube, const float *directions, const float *lods, float *rgb,
                                                              uint32_t n, uint64_t *bad_directions) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float d[3] = {directions[3u * (size_t)i], directions[3u * (size_t)i + 1u], directions[3u * (size_t)i + 2u]};
    float out[3];
    const bool good = env_sample(cube, d, lods[i], out);
    for (int k = 0; k < 3; k++) rgb[3u * (size_t)i + k] = out[k];
    count(bad_directions, good ? 0u : 1u);
}

uint32_t blocks_of(uint64_t threads) { return (uint32_t)((threads + kThreads - 1u) / kThreads); }

} // namespace

hipError_t launch_env_map(const OrbitEnvMap &j, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (j.stats) {
        hipLaunchKernelGGL(env_clear_kernel, dim3(1), dim3(1), 0, s, j.stats);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const uint32_t sky_levels = j.sky ? env_full_levels(j.sky_size) : 0u;
    const EnvCube sky = env_cube(j.sky, j.sky_size, sky_levels ? sky_levels : 1u);
    if (j.equirect) {
        hipLaunchKernelGGL(env_equirect_kernel, dim3(blocks_of(6ull * j.sky_size * j.sky_size)), dim3(kThreads), 0, s, j.equirect, j.equirect_w,
                           j.equirect_h, j.sky, j.sky_size, j.stats);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        for (uint32_t m = 1; m < sky_levels; m++) {
            const uint32_t n = j.sky_size >> m;
            hipLaunchKernelGGL(env_mip_kernel, dim3(blocks_of(6ull * n * n)), dim3(kThreads), 0, s, (const uint16_t *)j.sky + 4u * (size_t)sky.offset[m - 1u],
                               j.sky + 4u * (size_t)sky.offset[m], n, j.stats);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    if (j.irradiance) {
        const uint32_t n = j.irradiance_size;
        hipLaunchKernelGGL(env_irradiance_kernel, dim3((6u * n * n + kIrradianceThreads - 1u) / kIrradianceThreads), dim3(kIrradianceThreads), 0, s, sky, env_irradiance_lod(j.sky_size, n),
                           j.sample_delta, j.irradiance, n, j.stats);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (j.prefiltered) {
        const EnvCube out = env_cube(j.prefiltered, j.prefiltered_size, j.prefiltered_levels);
        for (uint32_t m = 0; m < j.prefiltered_levels; m++) {
            const uint32_t n = env_level_size(j.prefiltered_size, m), tiles = (n + kTile - 1u) / kTile; // at most 256 x 256 x 6
            hipLaunchKernelGGL(env_prefilter_kernel, dim3(tiles, tiles, 6), dim3(kThreads), 0, s, sky,
                               env_prefilter_level(m, j.prefiltered_levels, j.sample_count, j.sky_size), j.sample_count,
                               j.prefiltered + 4u * (size_t)out.offset[m], n, j.stats);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    if (j.brdf) {
        hipLaunchKernelGGL(env_brdf_kernel, dim3(blocks_of((uint64_t)j.brdf_size * j.brdf_size)), dim3(kThreads), 0, s, j.brdf, j.brdf_size,
                           j.brdf_sample_count, j.stats);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_env_sample(const OrbitEnvSample &j, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (j.bad_directions) {
        hipLaunchKernelGGL(env_clear_counter_kernel, dim3(1), dim3(1), 0, s, j.bad_directions);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (j.n == 0u) return e;
    hipLaunchKernelGGL(env_sample_kernel, dim3(blocks_of(j.n)), dim3(kThreads), 0, s, env_cube(j.cube, j.size, j.levels), j.directions, j.lods,
                       j.rgb, j.n, j.bad_directions);
    return hipGetLastError();
}

} // namespace orbit
