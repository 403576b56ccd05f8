// visibility_surface_drawn.hip — orbit_visibility_surface_drawn (include/orbit_abi_ext.h S2d, S3c, S3w):
// orbit_visibility_surface for a buffer drawn with ORBIT_RASTER_CLIP_NEAR and / or ORBIT_RASTER_WIDE_GUARD.  The
// arithmetic is surface_common.h's, shared with the host mirror, which is the pin.  (With raster_flags == 0 the entry
// point launches visibility_surface.hip's kernels; these run only with a flag.)
//
// Two launches on the stream, no look-back, no spinning, nothing handed from one workgroup to another:
//   clear    visibility_surface.hip's, restated: stats = 0, and with ORBIT_SURFACE_CLEAR the given outputs' fill
//   surface  visibility_surface.hip's walk — a wave per 8 x 8 tile, R9 and V3 per distinct command by the whole wave,
//            the distinct keys numbered by the broadcast-and-ballot loop, lane j sets up key j — and then
//            class    the lane that sets up a key classifies it (S2d): (a), or a class with a fixed verdict, is FAST
//                     and leaves the 17 words of §4.21; a key with candidates (a wide triangle, the pieces of a cut one)
//                     is SLOW: its lane also makes the one or two 28-word records of its candidates
//            pixel    every lane fetches its key's 17 words over ds_bpermute and runs surface_pixel.  One ballot decides
//                     whether the tile holds a slow key at all: if not, that was §4.21's path and the tile is done.
//                     Otherwise the pixel lanes fetch candidate 0 of their key over ds_bpermute (28 words), the lanes of
//                     slow keys test it, and candidate 1 is fetched only if a ballot says some lane still needs it.
//            The records travel over the cross-lane fetch, not an LDS table: a table of 64 keys x 2 candidates x 28
//            words is 14 KB per wave, 56 KB per workgroup, which would hold the CU to 2 workgroups where the registers
//            allow more, and would need the tile loop to fence the table between tiles; ds_bpermute allocates nothing.
//            The 128-bit arithmetic is behind kCandWide: it runs only for lanes whose candidate is a wide setup.
#include "kernels.h"
#include "orbit_device.h"
#include "surface_common.h"

namespace orbit {
namespace {

using namespace raster;

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;

// OrbitSurfaceStats' order
enum : uint32_t { kCovered, kWritten, kForeign, kUnsupported, kStale, kDegenerate, kCut, kWide, kStatWords = 8 };

// a pixel's record of an output that is only known to be 4-B aligned: one store of 8 or 16 bytes
struct __attribute__((packed, aligned(4))) Words2 {
    uint32_t w[2];
};
struct __attribute__((packed, aligned(4))) Words4 {
    uint32_t w[4];
};

__global__ __launch_bounds__(kThreads) void surface_drawn_clear_kernel(uint32_t *bary, uint32_t *grad, uint32_t *triangle,
                                                                       const size_t pixels, uint32_t *stats) {
    const size_t stride = (size_t)gridDim.x * kThreads, first = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (stats && first < kStatWords) stats[first] = 0u;
    // (NULL: not given, or no ORBIT_SURFACE_CLEAR)
    if (bary)
        for (size_t i = first; i < 2u * pixels; i += stride) bary[i] = 0u;
    if (grad)
        for (size_t i = first; i < 4u * pixels; i += stride) grad[i] = 0u;
    if (triangle)
        for (size_t i = first; i < 4u * pixels; i += stride) triangle[i] = 0xFFFFFFFFu;
}

__device__ __forceinline__ SurfaceTriangle fetch_triangle(const SurfaceTriangle &t, uint32_t src) {
    SurfaceTriangle out;
    for (int i = 0; i < 3; i++) {
        out.ax[i] = __shfl(t.ax[i], (int)src), out.ay[i] = __shfl(t.ay[i], (int)src);
        out.iw[i] = __shfl(t.iw[i], (int)src);
    }
    out.d0 = __shfl(t.d0, (int)src), out.gx = __shfl(t.gx, (int)src), out.gy = __shfl(t.gy, (int)src);
    out.flags = (uint32_t)__shfl((int)t.flags, (int)src);
    for (int i = 0; i < 4; i++) out.ids[i] = (uint32_t)__shfl((int)t.ids[i], (int)src);
    return out;
}

__device__ __forceinline__ int64_t fetch_i64(int64_t v, uint32_t src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src), hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), (int)src);
    return (int64_t)((uint64_t)hi << 32 | lo);
}

__device__ __forceinline__ SurfaceCandidate fetch_candidate(const SurfaceCandidate &c, uint32_t src) {
    SurfaceCandidate out;
    for (int i = 0; i < 3; i++) {
        out.x[i] = fetch_i64(c.x[i], src), out.y[i] = fetch_i64(c.y[i], src);
        out.iw[i] = __shfl(c.iw[i], (int)src), out.t[i] = __shfl(c.t[i], (int)src);
    }
    out.io = (uint32_t)__shfl((int)c.io, (int)src);
    for (int i = 0; i < 6; i++) out.plane[i] = (uint32_t)__shfl((int)c.plane[i], (int)src);
    out.flags = (uint32_t)__shfl((int)c.flags, (int)src);
    return out;
}

__global__ __launch_bounds__(kThreads) void surface_drawn_kernel(const OrbitVisibilitySurface j, const uint32_t raster_flags,
                                                                 const uint32_t tiles_x, const uint32_t tiles, int32_t *status) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t stride = gridDim.x * kWaves;
    const uint32_t listed = ((const uint32_t *)j.draw_commands)[0];
    const uint32_t n = listed < j.max_commands ? listed : j.max_commands;
    uint32_t n_covered = 0, n_written = 0, n_foreign = 0, n_unsupported = 0, n_stale = 0, n_degenerate = 0, n_cut = 0, n_wide = 0; // wave-uniform
    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < tiles; tile += stride) { // (wave-uniform)
        const uint32_t x = (tile % tiles_x) * 8u + (lane & 7u), y = (tile / tiles_x) * 8u + (lane >> 3);
        const bool in_target = x < j.width && y < j.height;
        const size_t p = (size_t)y * j.width + x;
        const uint64_t word = in_target ? j.visibility[p] : 0ull;
        const bool covered = word != 0ull;
        const uint32_t key = (uint32_t)word; // command << 8 | triangle
        const uint32_t k = (key >> 8) - j.command_base; // (below the base it wraps far above n)
        const bool own = covered && k < n; // S1
        const uint64_t own_lanes = __ballot(own);
        n_covered += (uint32_t)__popcll(__ballot(covered));
        n_foreign += (uint32_t)__popcll(__ballot(covered && !own));
        if (own_lanes == 0ull) continue; // (wave-uniform)
        // R9 and V3 of each distinct command, by the whole wave (k_src < n <= max_commands: inside the list)
        bool command_ok = false;
        uint64_t left = own_lanes;
        while (left != 0ull) {
            const uint32_t src = (uint32_t)__builtin_ctzll(left);
            const uint32_t k_src = (uint32_t)__builtin_amdgcn_readlane((int)k, (int)src);
            const bool mine = own && k == k_src;
            left &= ~__ballot(mine);
            const SurfaceCommand c = surface_command(j, k_src);
            bool bad = false;
            if (c.in_range) { // (wave-uniform) its index words and corner bytes lie inside meshlet_data
                for (uint32_t v = lane; v < c.vcount; v += 64u) bad = bad || !surface_index_word_ok(j, c, v);
                for (uint32_t b = lane; b < 3u * c.nt; b += 64u) bad = bad || !surface_corner_byte_ok(j, c, b);
            }
            const bool ok = c.in_range && __ballot(bad) == 0ull;
            if (mine) command_ok = ok;
        }
        // the distinct keys numbered: `slot` of a pixel lane, and key n_keys handed to lane n_keys for its setup
        uint32_t slot = 0, setup_key = 0, n_keys = 0;
        bool setup_ok = false;
        left = own_lanes;
        while (left != 0ull) {
            const uint32_t src = (uint32_t)__builtin_ctzll(left);
            const uint32_t key_src = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)src);
            const bool ok_src = __builtin_amdgcn_readlane(command_ok ? 1 : 0, (int)src) != 0;
            const bool mine = own && key == key_src;
            left &= ~__ballot(mine);
            if (mine) slot = n_keys;
            if (lane == n_keys) setup_key = key_src, setup_ok = ok_src;
            n_keys++; // at most 64
        }
        SurfaceTriangle made;
        for (int i = 0; i < 3; i++) made.ax[i] = made.ay[i] = 0, made.iw[i] = 0.0f;
        made.d0 = made.gx = made.gy = 0.0f, made.flags = kSurfaceStale;
        for (int i = 0; i < 4; i++) made.ids[i] = 0u;
        SurfaceSlow slow;
        candidate_none(slow.c[0]), candidate_none(slow.c[1]);
        slow.count = 0u, slow.miss = kSurfaceStale;
        bool is_slow = false;
        if (lane < n_keys)
            is_slow = surface_triangle_drawn(j, (setup_key >> 8) - j.command_base, setup_key & 255u, setup_ok, raster_flags, made, slow);
        const bool tile_slow = __ballot(is_slow) != 0ull; // (wave-uniform)
        // (every lane of the wave is here: the loops above are wave-uniform)
        const SurfaceTriangle t = fetch_triangle(made, slot);
        float out[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        bool degenerate = false;
        uint32_t verdict = kSurfaceStale, cand_flags = 0u;
        if (own) verdict = surface_pixel(t, (int32_t)x, (int32_t)y, (uint32_t)(word >> 32), out, degenerate);
        if (tile_slow) { // a lane of a slow key has verdict kSurfaceSlow: its candidates in turn, the first that owns it
            const uint32_t count = (uint32_t)__shfl((int)slow.count, (int)slot), miss = (uint32_t)__shfl((int)slow.miss, (int)slot);
            bool need = own && verdict == kSurfaceSlow;
            {
                const SurfaceCandidate c = fetch_candidate(slow.c[0], slot);
                if (need && surface_candidate_pixel(c, (int32_t)x, (int32_t)y, (uint32_t)(word >> 32), out, degenerate))
                    verdict = kSurfaceWritten, cand_flags = c.flags, need = false;
            }
            if (__ballot(need && count > 1u) != 0ull) { // (wave-uniform)
                const SurfaceCandidate c = fetch_candidate(slow.c[1], slot);
                if (need && count > 1u && surface_candidate_pixel(c, (int32_t)x, (int32_t)y, (uint32_t)(word >> 32), out, degenerate))
                    verdict = kSurfaceWritten, cand_flags = c.flags, need = false;
            }
            if (need) verdict = miss;
        }
        const bool written = own && verdict == kSurfaceWritten;
        n_written += (uint32_t)__popcll(__ballot(written));
        n_unsupported += (uint32_t)__popcll(__ballot(own && verdict == kSurfaceUnsupported));
        n_stale += (uint32_t)__popcll(__ballot(own && verdict == kSurfaceStale));
        n_degenerate += (uint32_t)__popcll(__ballot(written && degenerate));
        n_cut += (uint32_t)__popcll(__ballot(written && (cand_flags & kCandCut) != 0u));
        n_wide += (uint32_t)__popcll(__ballot(written && (cand_flags & kCandWide) != 0u));
        if (written) { // (in_target: p lies inside every output; the next tile's ballots see the whole wave again)
            if (j.bary) {
                Words2 r;
                r.w[0] = (uint32_t)float_bits(out[0]), r.w[1] = (uint32_t)float_bits(out[1]);
                *(Words2 *)(j.bary + 2u * p) = r;
            }
            if (j.grad) {
                Words4 r;
                for (int i = 0; i < 4; i++) r.w[i] = (uint32_t)float_bits(out[2 + i]);
                *(Words4 *)(j.grad + 4u * p) = r;
            }
            if (j.triangle) {
                Words4 r;
                for (int i = 0; i < 4; i++) r.w[i] = t.ids[i];
                *(Words4 *)(j.triangle + 4u * p) = r;
            }
        }
    }
    if (lane != 0u) return;
    if (n_stale != 0u) latch_status(status, ORBIT_E_RANGE);
    if (!j.stats) return;
    uint32_t *stats = (uint32_t *)j.stats;
    if (n_covered != 0u) atomicAdd(&stats[kCovered], n_covered);
    if (n_written != 0u) atomicAdd(&stats[kWritten], n_written);
    if (n_foreign != 0u) atomicAdd(&stats[kForeign], n_foreign);
    if (n_unsupported != 0u) atomicAdd(&stats[kUnsupported], n_unsupported);
    if (n_stale != 0u) atomicAdd(&stats[kStale], n_stale);
    if (n_degenerate != 0u) atomicAdd(&stats[kDegenerate], n_degenerate);
    if (n_cut != 0u) atomicAdd(&stats[kCut], n_cut);
    if (n_wide != 0u) atomicAdd(&stats[kWide], n_wide);
}

} // namespace

hipError_t launch_visibility_surface_drawn(const OrbitVisibilitySurface &job, uint32_t raster_flags, uint32_t num_cus,
                                           uint32_t grid_cap, int32_t *status, hipStream_t s) {
    const uint32_t resident = (num_cus ? num_cus : 64u) * 8u;
    const uint32_t cap = grid_cap != 0u && grid_cap < resident ? grid_cap : resident; // orbit_ctx_set_visibility_grid
    const size_t pixels = (size_t)job.width * job.height; // width, height <= 32768: at most 2^30
    const bool fill = (job.flags & ORBIT_SURFACE_CLEAR) != 0u;
    if (fill || job.stats) {
        const size_t need = fill ? (4u * pixels + kThreads * 4u - 1u) / (kThreads * 4u) : 1u;
        hipLaunchKernelGGL(surface_drawn_clear_kernel, dim3((uint32_t)(need < cap ? need : cap)), dim3(kThreads), 0, s,
                           fill ? (uint32_t *)job.bary : nullptr, fill ? (uint32_t *)job.grad : nullptr,
                           fill ? job.triangle : nullptr, pixels, (uint32_t *)job.stats);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint32_t tiles_x = (job.width + 7u) / 8u, tiles = tiles_x * ((job.height + 7u) / 8u); // at most 2^24
    const uint32_t need = (tiles + kWaves - 1u) / kWaves;
    hipLaunchKernelGGL(surface_drawn_kernel, dim3(need < cap ? need : cap), dim3(kThreads), 0, s, job, raster_flags, tiles_x, tiles,
                       status);
    return hipGetLastError();
}

} // namespace orbit
