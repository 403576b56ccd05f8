// bloom.hip — orbit_bloom and orbit_post_process (include/orbit_abi_ext.h B1-B9 and T1-T5): the
// reference's bloom chain of a colour plane into B10G11R11 mips, and its tone mapping and sRGB encoding.  The arithmetic is
// post_common.h's, shared with the host mirror, which is the pin.
//
// orbit_bloom: a one-thread launch writes the counters' start, then one launch per level (2 * levels - 1), each ordered
// behind the one before by the stream: no look-back, no spinning, nothing handed between workgroups.
//   level   a workgroup takes a 16 x 16 tile of the destination and a thread a texel.  The source texels the tile's taps
//           can touch form a box, bloom_down_span / bloom_up_span of the tile's first and last texel per axis (exact:
//           post_common.h proves it from monotonicity, rounding included).  When every tile's box of the level fits kBox
//           x kBox (the launch evaluates the same expressions per tile column and row) a workgroup stages its box in LDS
//           once, decoded to floats (colour texels by B8, packed texels by B7), channel planes apart, and every tap reads
//           LDS; otherwise (an upsample whose filter_radius x source size is large, or ORBIT_BLOOM_FORCE_DIRECT) the
//           level runs as a second kernel whose taps read and decode global memory.  The same floats either way, so the
//           same bytes.  A downsample's box is at most 22 wide at level 0 and, below it, (2 + 1 / dst) * 19 + 2 <= 42 for
//           a full tile (a narrower level has at most 31 source texels): it always fits.
//   The counters are sums of per-wave ballots: one atomic each per wave.
// orbit_post_process: a clearing launch for stats, then one pass of a resident grid, a thread per pixel and trip: 16 + 4 B
// in, 4 (+ 16) B out; the counters are summed per workgroup in LDS, one atomic each per workgroup.
#include "kernels.h"
#include "orbit_device.h"
#include "post_common.h"

namespace orbit {
namespace {

using namespace raster;

constexpr uint32_t kThreads = 256, kTile = 16, kBox = 44;
enum BloomMode : int { kDown0 = 0, kDown = 1, kUp = 2 };

struct BloomLevel {
    const float *color;  // kDown0: the source
    const uint32_t *src; // kDown, kUp: the source level
    uint32_t *dst;
    uint32_t src_w, src_h, dst_w, dst_h;
    float tf[4], radius;
    uint32_t direct;
    uint32_t *stats; // OrbitBloomStats or NULL
};

struct alignas(16) Quad {
    float f[4];
};

// texel (ix, iy) of the level's source, decoded
template <int MODE>
struct GlobalFetch {
    const BloomLevel &a;
    __device__ __forceinline__ void operator()(uint32_t ix, uint32_t iy, float *rgb) const {
        const size_t at = (size_t)iy * a.src_w + ix;
        if (MODE == kDown0) {
            const Quad q = *(const Quad *)(a.color + 4u * at);
            bloom_color_texel(q.f, rgb);
        } else {
            bloom_unpack(a.src[at], rgb);
        }
    }
};
// the same from the workgroup's box
struct TileFetch {
    const float *tile; // three planes of kBox * kBox
    uint32_t x_lo, y_lo, pitch;
    __device__ __forceinline__ void operator()(uint32_t ix, uint32_t iy, float *rgb) const {
        const uint32_t at = (iy - y_lo) * pitch + (ix - x_lo);
        rgb[0] = tile[at], rgb[1] = tile[kBox * kBox + at], rgb[2] = tile[2u * kBox * kBox + at];
    }
};

__global__ void bloom_begin_kernel(uint32_t *stats, uint32_t levels, uint32_t texels_written) {
    stats[0] = levels, stats[1] = texels_written, stats[2] = 0u, stats[3] = 0u;
}

// DIRECT: every tap reads global memory; otherwise the launch has made sure that every tile's box fits the LDS tile
template <int MODE, bool DIRECT>
__global__ __launch_bounds__(kThreads) void bloom_level_kernel(const BloomLevel a) {
    __shared__ float tile[DIRECT ? 1u : 3u * kBox * kBox];
    const uint32_t x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    const GlobalFetch<MODE> global{a};
    uint32_t x_lo = 0u, y_lo = 0u, bw = 0u; // (workgroup-uniform)
    if (!DIRECT) {
        const uint32_t x1 = (x0 + kTile < a.dst_w ? x0 + kTile : a.dst_w) - 1u, y1 = (y0 + kTile < a.dst_h ? y0 + kTile : a.dst_h) - 1u;
        uint32_t x_hi, y_hi;
        if (MODE == kUp) {
            bloom_up_span(x0, x1, a.dst_w, a.src_w, a.radius, x_lo, x_hi);
            bloom_up_span(y0, y1, a.dst_h, a.src_h, a.radius, y_lo, y_hi);
        } else {
            bloom_down_span(x0, x1, a.dst_w, a.src_w, x_lo, x_hi);
            bloom_down_span(y0, y1, a.dst_h, a.src_h, y_lo, y_hi);
        }
        bw = x_hi - x_lo + 1u; // x_lo <= x_hi < src_w by the clamps
        const uint32_t bh = y_hi - y_lo + 1u;
        if (bw > kBox || bh > kBox) return; // never: bloom_boxes_fit evaluated the same expressions before the launch
        for (uint32_t i = threadIdx.x; i < bw * bh; i += kThreads) {
            float rgb[3];
            global(x_lo + i % bw, y_lo + i / bw, rgb); // inside the source: the span is clamped to it
            tile[i] = rgb[0], tile[kBox * kBox + i] = rgb[1], tile[2u * kBox * kBox + i] = rgb[2]; // i < bw * bh <= kBox * kBox
        }
        __syncthreads();
    }
    const TileFetch staged{tile, x_lo, y_lo, bw};
    const uint32_t x = x0 + (threadIdx.x & (kTile - 1u)), y = y0 + threadIdx.x / kTile;
    const bool live = x < a.dst_w && y < a.dst_h;
    bool clamped = false, nonfinite = false;
    if (live) {
        const size_t p = (size_t)y * a.dst_w + x;
        float result[3];
        if (MODE == kUp) {
            if (DIRECT)
                bloom_up_texel(global, a.src_w, a.src_h, a.dst_w, a.dst_h, x, y, a.radius, result);
            else
                bloom_up_texel(staged, a.src_w, a.src_h, a.dst_w, a.dst_h, x, y, a.radius, result);
            float old[3];
            bloom_unpack(a.dst[p], old);
            for (int i = 0; i < 3; i++) result[i] = old[i] + result[i];
        } else {
            if (DIRECT)
                bloom_down_texel(global, a.src_w, a.src_h, a.dst_w, a.dst_h, x, y, MODE == kDown0, a.tf, result);
            else
                bloom_down_texel(staged, a.src_w, a.src_h, a.dst_w, a.dst_h, x, y, MODE == kDown0, a.tf, result);
            if (MODE == kDown0) { // B8: the centre tap's pixel (dst and color have one size)
                const Quad q = *(const Quad *)(a.color + 4u * p);
                float rgb[3];
                nonfinite = !bloom_color_texel(q.f, rgb);
            }
        }
        a.dst[p] = bloom_pack(result, clamped);
    }
    if (!a.stats) return; // (uniform)
    const uint32_t n_clamped = (uint32_t)__popcll(__ballot(clamped)), n_nonfinite = (uint32_t)__popcll(__ballot(nonfinite));
    if ((threadIdx.x & 63u) != 0u) return;
    if (n_nonfinite != 0u) atomicAdd(&a.stats[2], n_nonfinite);
    if (n_clamped != 0u) atomicAdd(&a.stats[3], n_clamped);
}

// every tile's box of the level fits the LDS tile: the kernel's own expressions, per tile column and per tile row
template <int MODE>
bool bloom_boxes_fit(const BloomLevel &a) {
    const auto axis_fits = [&](uint32_t dst_n, uint32_t src_n) {
        for (uint32_t first = 0; first < dst_n; first += kTile) {
            const uint32_t last = (first + kTile < dst_n ? first + kTile : dst_n) - 1u;
            uint32_t lo, hi;
            if (MODE == kUp)
                bloom_up_span(first, last, dst_n, src_n, a.radius, lo, hi);
            else
                bloom_down_span(first, last, dst_n, src_n, lo, hi);
            if (hi - lo + 1u > kBox) return false;
        }
        return true;
    };
    return axis_fits(a.dst_w, a.src_w) && axis_fits(a.dst_h, a.src_h);
}

template <int MODE>
hipError_t launch_level(const BloomLevel &a, hipStream_t s) {
    // dst_w, dst_h <= 32768: at most 2048 x 2048 workgroups
    const dim3 grid((a.dst_w + kTile - 1u) / kTile, (a.dst_h + kTile - 1u) / kTile);
    if (a.direct != 0u || !bloom_boxes_fit<MODE>(a))
        hipLaunchKernelGGL((bloom_level_kernel<MODE, true>), grid, dim3(kThreads), 0, s, a);
    else
        hipLaunchKernelGGL((bloom_level_kernel<MODE, false>), grid, dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

__global__ void post_begin_kernel(uint32_t *stats, uint32_t pixels) { stats[0] = pixels, stats[1] = 0u, stats[2] = 0u, stats[3] = 0u; }

__global__ __launch_bounds__(kThreads) void post_process_kernel(const OrbitPostProcess j, const size_t pixels) {
    __shared__ uint32_t block_count[2];
    if (threadIdx.x < 2u) block_count[threadIdx.x] = 0u;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * kThreads;
    const bool with_bloom = j.render_mode == 0u && j.bloom != nullptr, bgra = (j.flags & ORBIT_POST_BGRA) != 0u;
    uint32_t n_nonfinite = 0u, n_bloom = 0u; // wave-uniform
    // every wave makes the same number of trips, its lanes' pixels in range or not: the ballots see whole waves
    for (size_t base = (size_t)blockIdx.x * kThreads; base < pixels; base += stride) {
        const size_t p = base + threadIdx.x;
        uint32_t marks = 0u;
        if (p < pixels) {
            const Quad q = *(const Quad *)(j.color + 4u * p);
            uint32_t word = 0u;
            if (with_bloom) word = j.bloom[p];
            Quad ldr;
            uint32_t rgba8;
            marks = post_pixel(q.f, with_bloom, word, j.exposure, j.bloom_intensity, bgra, ldr.f, rgba8);
            if (j.ldr) *(Quad *)(j.ldr + 4u * p) = ldr;
            if (j.rgba8) ((uint32_t *)j.rgba8)[p] = rgba8;
        }
        n_nonfinite += (uint32_t)__popcll(__ballot((marks & kPostNonfinite) != 0u));
        n_bloom += (uint32_t)__popcll(__ballot((marks & kPostBloom) != 0u));
    }
    if (!j.stats) return; // (uniform)
    // one atomic per counter and workgroup: nearly every wave has bloom pixels, and 32 000 atomics on one word serialise
    if ((threadIdx.x & 63u) == 0u) {
        if (n_nonfinite != 0u) atomicAdd(&block_count[0], n_nonfinite);
        if (n_bloom != 0u) atomicAdd(&block_count[1], n_bloom);
    }
    __syncthreads();
    uint32_t *stats = (uint32_t *)j.stats;
    if (threadIdx.x < 2u && block_count[threadIdx.x] != 0u) atomicAdd(&stats[1u + threadIdx.x], block_count[threadIdx.x]);
}

} // namespace

hipError_t launch_bloom(const OrbitBloom &job, hipStream_t s) {
    OrbitBloomLayout lay;
    bloom_layout(job.width, job.height, job.max_levels, lay);
    const uint32_t levels = lay.levels;
    if (job.stats) {
        const uint32_t written = 2u * lay.total_texels - lay.level_width[levels - 1u] * lay.level_height[levels - 1u];
        hipLaunchKernelGGL(bloom_begin_kernel, dim3(1), dim3(1), 0, s, (uint32_t *)job.stats, levels, written);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    BloomLevel a{};
    a.color = job.color, a.radius = job.filter_radius, a.stats = (uint32_t *)job.stats;
    a.direct = (job.flags & ORBIT_BLOOM_FORCE_DIRECT) != 0u ? 1u : 0u;
    bloom_threshold_filter(job.threshold, job.soft_threshold, a.tf); // B2
    for (uint32_t k = 0; k < levels; k++) {
        a.dst = job.mips + lay.level_offset[k], a.dst_w = lay.level_width[k], a.dst_h = lay.level_height[k];
        if (k == 0u) {
            a.src = nullptr, a.src_w = job.width, a.src_h = job.height;
        } else {
            a.src = job.mips + lay.level_offset[k - 1u], a.src_w = lay.level_width[k - 1u], a.src_h = lay.level_height[k - 1u];
        }
        const hipError_t e = k == 0u ? launch_level<kDown0>(a, s) : launch_level<kDown>(a, s);
        if (e != hipSuccess) return e;
    }
    for (uint32_t k = levels - 1u; k >= 1u; k--) {
        a.src = job.mips + lay.level_offset[k], a.src_w = lay.level_width[k], a.src_h = lay.level_height[k];
        a.dst = job.mips + lay.level_offset[k - 1u], a.dst_w = lay.level_width[k - 1u], a.dst_h = lay.level_height[k - 1u];
        const hipError_t e = launch_level<kUp>(a, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_post_process(const OrbitPostProcess &job, uint32_t num_cus, uint32_t grid_cap, hipStream_t s) {
    const size_t pixels = (size_t)job.width * job.height; // at most 2^30
    if (job.stats) {
        hipLaunchKernelGGL(post_begin_kernel, dim3(1), dim3(1), 0, s, (uint32_t *)job.stats, (uint32_t)pixels);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const size_t need = (pixels + kThreads - 1u) / kThreads, resident = (size_t)(num_cus ? num_cus : 64u) * 8u; // a resident grid, striding
    const size_t cap = grid_cap != 0u && grid_cap < resident ? grid_cap : resident; // orbit_ctx_set_visibility_grid
    hipLaunchKernelGGL(post_process_kernel, dim3((uint32_t)(need < cap ? need : cap)), dim3(kThreads), 0, s, job, pixels);
    return hipGetLastError();
}

} // namespace orbit
