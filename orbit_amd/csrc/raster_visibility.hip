// raster_visibility.hip — orbit_raster_visibility and orbit_visibility_resolve (include/orbit_abi_ext.h V1-V4, DESIGN.md
// §4.13): the depth prepass of raster_depth.hip with the identity of the winner kept, and the pass that turns the
// buffer into depth, per-command pixel counts and the visible set.
//
// The raster kernel is the walker of raster_walk.h (a resident grid striding over the list, a wave per command, vertices
// in LDS, a lane per triangle for setup, the lane walk for small boxes and the wave walk for large ones) over a sink
// that builds the word of V2 — depth bits above, command and triangle below — and merges it by one 64-bit atomicMax on
// the u64 view, behind a relaxed 8-B atomic load that skips the atomic where the buffer already holds at least as much:
// the buffer only grows, so a stale smaller value costs an atomic, never a pixel.
//
// The resolve reads each word once.  A wave takes an 8 x 8 pixel tile; neighbouring pixels mostly share a command, so the
// wave aggregates before it touches memory: the first remaining lane's command, a ballot of the lanes that hold the
// same, one atomicAdd of their number from one lane, until no lane remains.  All outputs are integer sums.
#include "raster_walk.h"

#ifndef ORBIT_RASTER_VARIANT // raster_visibility_clip.hip and raster_visibility_wide.hip compile this file with theirs
#define ORBIT_RASTER_VARIANT Plain
#define ORBIT_RASTER_WITH_RESOLVE 1 // the resolve is compiled once, in the unit that sets no variant
#endif
// the variant's kernel, under the name the profiles know it by
#define ORBIT_RASTER_KERNEL_Plain raster_visibility_kernel
#define ORBIT_RASTER_KERNEL_ClipNear raster_visibility_clip_kernel
#define ORBIT_RASTER_KERNEL_Wide raster_visibility_wide_kernel
#define ORBIT_RASTER_VISIBILITY_KERNEL ORBIT_RASTER_PASTE(ORBIT_RASTER_KERNEL_, ORBIT_RASTER_VARIANT)

namespace orbit {
namespace {

using namespace raster;

// R7 and V2 of one inside sample -> it is a fragment (d > 0)
struct VisibilitySink {
    static constexpr uint32_t kMaxTriangles = 256u; // V3: the triangle index has 8 bits
    unsigned long long *visibility;
    template <class AnySetup> // Setup (R7) or SetupW (R7w)
    __device__ __forceinline__ bool write(const AnySetup &s, int32_t x, int32_t y, uint32_t width, uint32_t id) const {
        const float d = depth_at(s, 256 * x + 128, 256 * y + 128);
        if (!(d > 0.0f)) return false;
        const unsigned long long word = (unsigned long long)__float_as_uint(d) << 32 | id;
        unsigned long long *dst = visibility + (size_t)y * width + (uint32_t)x;
        if (word > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dst, word);
        return true;
    }
};

constexpr RasterVariant kVariant = RasterVariant::ORBIT_RASTER_VARIANT;

// (with ClipNear and Wide every piece carries the original triangle's index)
__global__ __launch_bounds__(kRasterThreads) void ORBIT_RASTER_VISIBILITY_KERNEL(const RasterParams p, const VisibilitySink sink,
                                                                                 const uint32_t command_base) {
    raster_commands<kVariant>(p, sink, command_base);
}

} // namespace

template <>
uint32_t raster_visibility_blocks_per_cu<kVariant>() {
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, ORBIT_RASTER_VISIBILITY_KERNEL, (int)kRasterThreads, 0);
    return e == hipSuccess && n > 0 ? (uint32_t)n : 2u;
}

template <>
hipError_t launch_raster_visibility<kVariant>(const OrbitRasterVisibility &job, uint32_t resident_blocks, int32_t *status,
                                              hipStream_t s) {
    return launch_raster(ORBIT_RASTER_VISIBILITY_KERNEL, job, (unsigned long long *)job.visibility, resident_blocks, status, s,
                         VisibilitySink{(unsigned long long *)job.visibility}, job.command_base);
}

#ifdef ORBIT_RASTER_WITH_RESOLVE
namespace {

constexpr uint32_t kResolveThreads = 256, kResolveWaves = kResolveThreads / 64;

// command_pixels[0, commands) = 0 and, if given, the four counters = 0
__global__ __launch_bounds__(kResolveThreads) void resolve_clear_kernel(uint32_t *command_pixels, uint32_t commands,
                                                                        uint32_t *stats) {
    const uint32_t stride = gridDim.x * kResolveThreads;
    if (command_pixels)
        for (uint32_t i = blockIdx.x * kResolveThreads + threadIdx.x; i < commands; i += stride) command_pixels[i] = 0u;
    if (stats && blockIdx.x == 0u && threadIdx.x < 4u) stats[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(kResolveThreads) void visibility_resolve_kernel(const OrbitVisibilityResolve j, const uint32_t tiles_x,
                                                                             const uint32_t tiles) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t stride = gridDim.x * kResolveWaves;
    uint32_t n_covered = 0, n_foreign = 0, n_visible = 0; // n_covered, n_foreign: wave-uniform; n_visible: this lane's share
    for (uint32_t tile = blockIdx.x * kResolveWaves + wave; tile < tiles; tile += stride) { // (wave-uniform)
        const uint32_t x = (tile % tiles_x) * 8u + (lane & 7u), y = (tile / tiles_x) * 8u + (lane >> 3);
        const bool in_target = x < j.width && y < j.height;
        const size_t pixel = (size_t)y * j.width + x;
        const uint64_t word = in_target ? j.visibility[pixel] : 0ull;
        if (j.depth && in_target) j.depth[pixel] = __uint_as_float((uint32_t)(word >> 32));
        const bool covered = word != 0ull;
        const uint32_t k = ((uint32_t)(word >> 8) & 0xFFFFFFu) - j.command_base; // (below the base it wraps far above max_commands)
        const bool own = covered && k < j.max_commands;
        n_covered += (uint32_t)__popcll(__ballot(covered));
        n_foreign += (uint32_t)__popcll(__ballot(covered && !own));
        if (!j.command_pixels) continue;
        uint64_t left = __ballot(own);
        while (left != 0ull) {
            const uint32_t src = (uint32_t)__builtin_ctzll(left);
            const uint32_t k_src = (uint32_t)__builtin_amdgcn_readlane((int)k, (int)src);
            const uint64_t same = __ballot(own && k == k_src);
            left &= ~same;
            // k_src < max_commands: lane src is `own`.  The one wave that finds the entry 0 counts the command as visible
            if (lane == src && atomicAdd(&j.command_pixels[k_src], (uint32_t)__popcll(same)) == 0u) n_visible++;
        }
    }
    if (!j.stats) return;
    for (uint32_t d = 1; d < 64u; d <<= 1) n_visible += (uint32_t)__shfl_xor((int)n_visible, (int)d, 64);
    if (lane != 0u) return;
    uint32_t *stats = (uint32_t *)j.stats; // OrbitVisibilityStats' order
    if (n_covered != 0u) atomicAdd(&stats[0], n_covered);
    if (n_visible != 0u) atomicAdd(&stats[1], n_visible);
    if (n_foreign != 0u) atomicAdd(&stats[2], n_foreign);
}

} // namespace

hipError_t launch_visibility_resolve(const OrbitVisibilityResolve &job, uint32_t num_cus, uint32_t grid_cap, hipStream_t s) {
    const uint32_t resident = (num_cus ? num_cus : 64u) * 8u;
    const uint32_t cap = grid_cap != 0u && grid_cap < resident ? grid_cap : resident; // orbit_ctx_set_visibility_grid
    if (job.stats || (job.command_pixels && job.max_commands != 0u)) {
        const uint32_t need = job.command_pixels ? (job.max_commands + kResolveThreads * 4u - 1u) / (kResolveThreads * 4u) : 1u;
        hipLaunchKernelGGL(resolve_clear_kernel, dim3(need < 1u ? 1u : need < cap ? need : cap), dim3(kResolveThreads), 0, s,
                           job.command_pixels, job.max_commands, (uint32_t *)job.stats);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    // width, height <= 32768: at most 2^24 tiles
    const uint32_t tiles_x = (job.width + 7u) / 8u, tiles = tiles_x * ((job.height + 7u) / 8u);
    const uint32_t need = (tiles + kResolveWaves - 1u) / kResolveWaves;
    hipLaunchKernelGGL(visibility_resolve_kernel, dim3(need < cap ? need : cap), dim3(kResolveThreads), 0, s, job, tiles_x, tiles);
    return hipGetLastError();
}
#endif // ORBIT_RASTER_WITH_RESOLVE

} // namespace orbit
