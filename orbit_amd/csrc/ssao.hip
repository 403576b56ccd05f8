// ssao.hip — orbit_ssao (include/orbit_abi_ext.h A1-A9): the reference's SSAO of a depth plane, its blur
// and what forward.frag reads of it per pixel.  The arithmetic is ssao_common.h's, shared with the host mirror, which is
// the pin.  A one-thread launch writes the counters' start, then three launches, each ordered behind the one before by the
// stream:
//   ssao    a workgroup takes a 16 x 16 tile of the SSAO grid (four of the shader's 8 x 8 groups) and a thread a pixel.
//           The 18 x 18 bordered tile of view-space positions (A1; the border left of column 0 and above row 0 is the
//           shader's wrapped pixel) is staged in LDS, three planes, each position computed once; A4's table, which does
//           not depend on the pixel, is computed by the first sample_count threads into LDS, 16 B per sample.  The depth
//           taps of A5 read global memory: a tap's reach depends on the pixel's depth, so no tile bounds them.  The
//           counters are summed per workgroup in LDS, one atomic each per workgroup.
//   blur    a thread per SSAO pixel: 16 bytes of raw in, one byte out.
//   read    a thread per screen pixel: 4 bytes of blurred in, one float out.
// Every index into depth, raw and blurred comes out of bloom_axis' clamp to the plane; noise and samples are indexed modulo
// their sizes; a thread whose pixel lies beyond the grid stores nothing.
#include "kernels.h"
#include "orbit_device.h"
#include "ssao_common.h"

namespace orbit {
namespace {

using namespace raster;

constexpr uint32_t kThreads = 256, kTile = 16, kBordered = kTile + 2u, kTexels = kBordered * kBordered;

struct PlaneFetch { // a float plane as it is
    const float *plane;
    uint32_t w;
    __device__ __forceinline__ float operator()(uint32_t ix, uint32_t iy) const { return plane[(size_t)iy * w + ix]; }
};
struct ByteFetch { // an R8_UNORM plane
    const uint8_t *plane;
    uint32_t w;
    __device__ __forceinline__ float operator()(uint32_t ix, uint32_t iy) const { return (float)plane[(size_t)iy * w + ix] / 255.0f; }
};

__global__ void ssao_begin_kernel(OrbitSsaoStats *stats, uint32_t pixels) {
    stats->pixels = pixels, stats->nonfinite_pixels = 0u, stats->unoccluded_pixels = 0u, stats->_pad = 0u, stats->samples_in_range = 0ull;
}

__global__ __launch_bounds__(kThreads) void ssao_kernel(const OrbitSsao j) {
    __shared__ float tile[3u * kTexels];
    __shared__ float table[4u * kSsaoMaxSamples];
    __shared__ uint32_t block_count[3];
    const PlaneFetch depth{j.depth, j.screen_w};
    const uint32_t x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    const float rcp_w = 1.0f / (float)j.ssao_w, rcp_h = 1.0f / (float)j.ssao_h;
    if (threadIdx.x < 3u) block_count[threadIdx.x] = 0u;
    if (threadIdx.x < j.sample_count) // sample_count <= kSsaoMaxSamples by the entry point
        ssao_table_entry(j.samples, j.samples_size, threadIdx.x, j.sample_count, j.min_radius, j.max_radius, table + 4u * threadIdx.x);
    for (uint32_t t = threadIdx.x; t < kTexels; t += kThreads) {
        // the shader's uvec2 pixel: x0 - 1 wraps to 0xFFFFFFFF at x0 == 0
        const uint32_t px = x0 - 1u + t % kBordered, py = y0 - 1u + t / kBordered;
        float p[3];
        ssao_position(depth, j.inverse_projection, px, py, rcp_w, rcp_h, j.screen_w, j.screen_h, p);
        tile[t] = p[0], tile[kTexels + t] = p[1], tile[2u * kTexels + t] = p[2];
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & (kTile - 1u), ly = threadIdx.x / kTile;
    const uint32_t x = x0 + lx, y = y0 + ly;
    const bool live = x < j.ssao_w && y < j.ssao_h;
    uint32_t in_range = 0u;
    bool nonfinite = false, unoccluded = false;
    if (live) {
        const auto at = [&](uint32_t cx, uint32_t cy, float *p) {
            const uint32_t t = cy * kBordered + cx; // cx, cy <= kTile + 1
            p[0] = tile[t], p[1] = tile[kTexels + t], p[2] = tile[2u * kTexels + t];
        };
        float p0[3], right[3], left[3], down[3], up[3], normal[3], tangent[3], bitangent[3];
        at(lx + 1u, ly + 1u, p0), at(lx + 2u, ly + 1u, right), at(lx, ly + 1u, left), at(lx + 1u, ly + 2u, down), at(lx + 1u, ly, up);
        uint32_t marks = ssao_normal(p0, right, left, down, up, normal);
        ssao_basis(j.noise, j.noise_size, x, y, normal, tangent, bitangent);
        const float occlusion = ssao_occlusion(depth, j.projection, j.screen_w, j.screen_h, p0, tangent, bitangent, normal, table, j.sample_count,
                                               j.min_radius, in_range, nullptr);
        const uint32_t byte = ssao_pixel_byte(occlusion, j.sample_count, marks);
        j.raw[(size_t)y * j.ssao_w + x] = (uint8_t)byte;
        nonfinite = (marks & kSsaoNonfinite) != 0u, unoccluded = byte == 255u;
    }
    if (!j.stats) return; // (uniform)
    const uint32_t n_nonfinite = (uint32_t)__popcll(__ballot(nonfinite)), n_unoccluded = (uint32_t)__popcll(__ballot(unoccluded));
    uint32_t n_in_range = in_range; // at most 64 per lane, 16 384 per workgroup
    for (int off = 32; off > 0; off >>= 1) n_in_range += __shfl_down(n_in_range, off, 64);
    if ((threadIdx.x & 63u) == 0u) {
        if (n_nonfinite != 0u) atomicAdd(&block_count[0], n_nonfinite);
        if (n_unoccluded != 0u) atomicAdd(&block_count[1], n_unoccluded);
        if (n_in_range != 0u) atomicAdd(&block_count[2], n_in_range);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        if (block_count[0] != 0u) atomicAdd(&j.stats->nonfinite_pixels, block_count[0]);
        if (block_count[1] != 0u) atomicAdd(&j.stats->unoccluded_pixels, block_count[1]);
        if (block_count[2] != 0u) atomicAdd((unsigned long long *)&j.stats->samples_in_range, (unsigned long long)block_count[2]);
    }
}

__global__ __launch_bounds__(kThreads) void ssao_blur_kernel(const uint8_t *raw, uint8_t *blurred, uint32_t w, uint32_t h) {
    const uint32_t x = blockIdx.x * kTile + (threadIdx.x & (kTile - 1u)), y = blockIdx.y * kTile + threadIdx.x / kTile;
    if (x >= w || y >= h) return;
    blurred[(size_t)y * w + x] = (uint8_t)ssao_blur_texel(ByteFetch{raw, w}, x, y, w, h);
}

__global__ __launch_bounds__(kThreads) void ssao_read_kernel(const uint8_t *blurred, float *ao_pixel, uint32_t screen_w, uint32_t screen_h,
                                                             uint32_t w, uint32_t h) {
    // 64 x 4 pixels per workgroup: a wave stores 256 contiguous bytes
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + threadIdx.x / 64u;
    if (x >= screen_w || y >= screen_h) return;
    ao_pixel[(size_t)y * screen_w + x] = ssao_pixel_read(ByteFetch{blurred, w}, x, y, screen_w, screen_h, w, h);
}

} // namespace

hipError_t launch_ssao(const OrbitSsao &job, hipStream_t s) {
    if (job.stats) {
        hipLaunchKernelGGL(ssao_begin_kernel, dim3(1), dim3(1), 0, s, job.stats, job.ssao_w * job.ssao_h);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    // ssao_w, ssao_h <= 32768: at most 2048 x 2048 workgroups
    const dim3 grid((job.ssao_w + kTile - 1u) / kTile, (job.ssao_h + kTile - 1u) / kTile);
    hipLaunchKernelGGL(ssao_kernel, grid, dim3(kThreads), 0, s, job);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !job.blurred) return e;
    hipLaunchKernelGGL(ssao_blur_kernel, grid, dim3(kThreads), 0, s, (const uint8_t *)job.raw, job.blurred, job.ssao_w, job.ssao_h);
    e = hipGetLastError();
    if (e != hipSuccess || !job.ao_pixel) return e;
    hipLaunchKernelGGL(ssao_read_kernel, dim3((job.screen_w + 63u) / 64u, (job.screen_h + 3u) / 4u), dim3(kThreads), 0, s,
                       (const uint8_t *)job.blurred, job.ao_pixel, job.screen_w, job.screen_h, job.ssao_w, job.ssao_h);
    return hipGetLastError();
}

} // namespace orbit
