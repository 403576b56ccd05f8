// surface_fragments.hip — orbit_surface_fragments (include/orbit_abi_ext.h F1-F8): from a visibility
// buffer, the list that made it, a surface call's bary / grad / triangle and the vertex attributes to the inputs of the
// reference's fragment shader per owned pixel.  The arithmetic is fragment_common.h's, shared with the host mirror,
// which is the pin.
//
// Two launches on the stream, no look-back, no spinning, nothing handed from one workgroup to another:
//   clear      stats = 0, and with ORBIT_FRAGMENTS_CLEAR the given outputs' fill
//   fragments  a wave takes an 8 x 8 pixel tile (out-of-target lanes carry 0) and a lane a pixel, as the buffer's other
//              readers do.  There is no work per command or per triangle to share: a lane runs its own vertex stage
//              (F3, about 400 flops) and neighbouring lanes mostly name the same three vertices and the same entity, so
//              the gathers of a wave fall into a few cache lines.  Each output leaves as one store per pixel (4, 8, 12 or
//              16 B, 4-B aligned); a tile row is a contiguous run.
//              The counters are wave-uniform popcounts: one atomic each per wave at the end.
#include "kernels.h"
#include "orbit_device.h"
#include "fragment_common.h"

namespace orbit {
namespace {

using namespace raster;

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;

// OrbitFragmentStats' order
enum : uint32_t { kCovered, kWritten, kForeign, kUnshaded, kStale, kDegenerate, kStatWords = 8 };

// a pixel's record of an output that is only known to be 4-B aligned: one store of 8, 12 or 16 bytes
struct __attribute__((packed, aligned(4))) Words2 {
    uint32_t w[2];
};
struct __attribute__((packed, aligned(4))) Words3 {
    uint32_t w[3];
};
struct __attribute__((packed, aligned(4))) Words4 {
    uint32_t w[4];
};

struct FragmentFill { // the outputs to fill (NULL: not given, or no ORBIT_FRAGMENTS_CLEAR)
    uint32_t *zero[5];
    uint32_t words[5]; // per pixel
    uint32_t *material;
};

__global__ __launch_bounds__(kThreads) void fragments_clear_kernel(const FragmentFill f, const size_t pixels, uint32_t *stats) {
    const size_t stride = (size_t)gridDim.x * kThreads, first = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (stats && first < kStatWords) stats[first] = 0u;
    for (int o = 0; o < 5; o++)
        if (f.zero[o])
            for (size_t i = first; i < (size_t)f.words[o] * pixels; i += stride) f.zero[o][i] = 0u;
    if (f.material)
        for (size_t i = first; i < pixels; i += stride) f.material[i] = 0xFFFFFFFFu;
}

__global__ __launch_bounds__(kThreads) void fragments_kernel(const OrbitSurfaceFragments j, const uint32_t tiles_x,
                                                             const uint32_t tiles, int32_t *status) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t stride = gridDim.x * kWaves;
    const uint32_t listed = ((const uint32_t *)j.draw_commands)[0];
    const uint32_t n = listed < j.max_commands ? listed : j.max_commands;
    uint32_t n_covered = 0, n_written = 0, n_foreign = 0, n_unshaded = 0, n_stale = 0, n_degenerate = 0; // wave-uniform
    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < tiles; tile += stride) { // (wave-uniform)
        const uint32_t x = (tile % tiles_x) * 8u + (lane & 7u), y = (tile / tiles_x) * 8u + (lane >> 3);
        const bool in_target = x < j.width && y < j.height;
        const size_t p = (size_t)y * j.width + x;
        const uint64_t word = in_target ? j.visibility[p] : 0ull;
        const bool covered = word != 0ull;
        const uint32_t k = ((uint32_t)word >> 8) - j.command_base; // (below the base it wraps far above n)
        const bool own = covered && k < n; // F1
        n_covered += (uint32_t)__popcll(__ballot(covered));
        n_foreign += (uint32_t)__popcll(__ballot(covered && !own));
        if (__ballot(own) == 0ull) continue; // (wave-uniform)
        float out[kFragmentFloats];
        uint32_t material = 0xFFFFFFFFu, verdict = kFragmentStale;
        bool degenerate = false;
        if (own) verdict = fragment_pixel(j, k, p, out, material, degenerate); // (in_target: p lies inside every buffer)
        const bool written = own && verdict == kFragmentWritten;
        n_written += (uint32_t)__popcll(__ballot(written));
        n_unshaded += (uint32_t)__popcll(__ballot(own && verdict == kFragmentUnshaded));
        n_stale += (uint32_t)__popcll(__ballot(own && verdict == kFragmentStale));
        n_degenerate += (uint32_t)__popcll(__ballot(written && degenerate));
        if (written) { // (the next tile's ballots see the whole wave again)
            if (j.world_pos) {
                Words4 r;
                for (int i = 0; i < 4; i++) r.w[i] = (uint32_t)float_bits(out[i]);
                *(Words4 *)(j.world_pos + 4u * p) = r;
            }
            if (j.normal) {
                Words3 r;
                for (int i = 0; i < 3; i++) r.w[i] = (uint32_t)float_bits(out[4 + i]);
                *(Words3 *)(j.normal + 3u * p) = r;
            }
            if (j.tangent) {
                Words4 r;
                for (int i = 0; i < 4; i++) r.w[i] = (uint32_t)float_bits(out[7 + i]);
                *(Words4 *)(j.tangent + 4u * p) = r;
            }
            if (j.uv) {
                Words2 r;
                r.w[0] = (uint32_t)float_bits(out[11]), r.w[1] = (uint32_t)float_bits(out[12]);
                *(Words2 *)(j.uv + 2u * p) = r;
            }
            if (j.uv_grad) {
                Words4 r;
                for (int i = 0; i < 4; i++) r.w[i] = (uint32_t)float_bits(out[13 + i]);
                *(Words4 *)(j.uv_grad + 4u * p) = r;
            }
            if (j.material) j.material[p] = material;
        }
    }
    if (lane != 0u) return;
    if (n_stale != 0u) latch_status(status, ORBIT_E_RANGE);
    if (!j.stats) return;
    uint32_t *stats = (uint32_t *)j.stats;
    if (n_covered != 0u) atomicAdd(&stats[kCovered], n_covered);
    if (n_written != 0u) atomicAdd(&stats[kWritten], n_written);
    if (n_foreign != 0u) atomicAdd(&stats[kForeign], n_foreign);
    if (n_unshaded != 0u) atomicAdd(&stats[kUnshaded], n_unshaded);
    if (n_stale != 0u) atomicAdd(&stats[kStale], n_stale);
    if (n_degenerate != 0u) atomicAdd(&stats[kDegenerate], n_degenerate);
}

} // namespace

hipError_t launch_surface_fragments(const OrbitSurfaceFragments &job, uint32_t num_cus, uint32_t grid_cap, int32_t *status,
                                    hipStream_t s) {
    const uint32_t resident = (num_cus ? num_cus : 64u) * 8u;
    const uint32_t cap = grid_cap != 0u && grid_cap < resident ? grid_cap : resident; // orbit_ctx_set_visibility_grid
    const size_t pixels = (size_t)job.width * job.height; // width, height <= 32768: at most 2^30
    const bool fill = (job.flags & ORBIT_FRAGMENTS_CLEAR) != 0u;
    if (fill || job.stats) {
        FragmentFill f;
        float *const outs[5] = {job.world_pos, job.normal, job.tangent, job.uv, job.uv_grad};
        const uint32_t words[5] = {4u, 3u, 4u, 2u, 4u};
        for (int o = 0; o < 5; o++) f.zero[o] = fill ? (uint32_t *)outs[o] : nullptr, f.words[o] = words[o];
        f.material = fill ? job.material : nullptr;
        const size_t need = fill ? (4u * pixels + kThreads * 4u - 1u) / (kThreads * 4u) : 1u;
        hipLaunchKernelGGL(fragments_clear_kernel, dim3((uint32_t)(need < cap ? need : cap)), dim3(kThreads), 0, s, f, pixels,
                           (uint32_t *)job.stats);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint32_t tiles_x = (job.width + 7u) / 8u, tiles = tiles_x * ((job.height + 7u) / 8u); // at most 2^24
    const uint32_t need = (tiles + kWaves - 1u) / kWaves;
    hipLaunchKernelGGL(fragments_kernel, dim3(need < cap ? need : cap), dim3(kThreads), 0, s, job, tiles_x, tiles, status);
    return hipGetLastError();
}

} // namespace orbit
