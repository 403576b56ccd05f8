// fragments_shade.hip — orbit_fragments_shade (include/orbit_abi_ext.h L1-L9): from a visibility buffer,
// the planes orbit_surface_fragments left, the material and light tables and the cluster chain's light lists to the
// colour of every visible pixel.  The arithmetic is shade_common.h's, shared with the host mirror, which is the pin; the
// slice comes through orbit_device.h's depth_slice, the mark stage's own function.
//
// Two launches on the stream, no look-back, no spinning, nothing handed from one workgroup to another:
//   clear  stats = 0, and with ORBIT_SHADE_CLEAR color and lights_walked
//   shade  a wave takes an 8 x 8 pixel tile (out-of-target lanes carry 0) and a lane a pixel, as the buffer's other
//          readers do.  Two forms, equal bytes (every pixel adds its own list in list order):
//          per lane  each lane runs shade_pixel: its own (offset, n), its own gathers of index and 64-B light row.
//          staged    tile_size_px % 8 == 0: the wave's 64 pixels share one cluster column.  The wave loops over the
//                    distinct slices among its lanes (a wave-uniform ballot); per slice the cluster's list goes in
//                    chunks of 64: lane i loads index i and its light row, range-checks it and writes the 16 words
//                    L5 / L6 read to the wave's own 4-KB LDS table; then every lane of that slice runs L5 over the
//                    chunk from LDS at a wave-uniform address (a broadcast: no bank conflict).  A bad index marks
//                    the pixels of that slice stale: exactly those whose walk contains it.  No __syncthreads: the
//                    table is the wave's own, a wave-level fence orders its writes and reads.
//          The counters are wave-uniform popcounts: one atomic each per wave at the end.
#include "kernels.h"
#include "orbit_device.h"
#include "shade_common.h"

namespace orbit {
namespace {

using namespace raster;

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;

// OrbitShadeStats' order
enum : uint32_t { kCovered, kWritten, kUnshaded, kStale, kOutside, kDegenerate, kTextured, kUnserved, kStatWords = 8 };

// a pixel's record of a plane that is only known to be 4-B aligned: one access of 12 or 16 bytes
struct __attribute__((packed, aligned(4))) Words3 {
    uint32_t w[3];
};
struct __attribute__((packed, aligned(4))) Words4 {
    uint32_t w[4];
};

__global__ __launch_bounds__(kThreads) void shade_clear_kernel(uint32_t *color, uint32_t *lights_walked, const size_t pixels,
                                                               uint32_t *stats) {
    const size_t stride = (size_t)gridDim.x * kThreads, first = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (stats && first < kStatWords) stats[first] = 0u;
    if (color)
        for (size_t i = first; i < 4u * pixels; i += stride) color[i] = 0u;
    if (lights_walked)
        for (size_t i = first; i < pixels; i += stride) lights_walked[i] = 0u;
}

// the wave's LDS writes before, its LDS reads behind (handoff.h's idiom)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The staged form of one tile: L1-L8 of the lane's covered pixel p through the wave's table -> the verdict, as
// shade_pixel's.  Called by the whole wave; `covered` lanes lie in the target.  tx, ty: the tile's cluster column.
__device__ __forceinline__ uint32_t shade_pixel_staged(const OrbitFragmentsShade &j, ShadeLight *table, uint32_t lane, bool covered,
                                                       uint32_t tx, uint32_t ty, size_t p, uint32_t slice, float *color, uint32_t &n,
                                                       uint32_t &marks) {
    n = 0u, marks = 0u;
    for (int i = 0; i < 4; i++) color[i] = 0.0f;
    uint32_t verdict = kShadeUnshaded;
    ShadePixel px = {};
    if (covered) {
        const uint32_t material = j.material[p];
        verdict = shade_material_verdict(j, material);
        if (verdict == kShadeWritten) {
            const OrbitMaterialData m = shade_load_row(j.materials, material);
            Words4 wp = *(const Words4 *)(j.world_pos + 4u * p);
            Words3 nrm = *(const Words3 *)(j.normal + 3u * p);
            float wpf[4], nf[3];
            __builtin_memcpy(wpf, &wp, 16);
            __builtin_memcpy(nf, &nrm, 12);
            shade_pixel_begin(j, m, wpf, nf, px);
        }
    }
    const bool live = covered && verdict == kShadeWritten;
    const uint32_t cx = j.cluster_count[0], cy = j.cluster_count[1], cz = j.cluster_count[2];
    const bool inside = live && tx < cx && ty < cy && slice < cz;
    const uint32_t *indices = shade_indices(j);
    uint64_t rest = __ballot(inside); // (wave-uniform)
    while (rest != 0ull) {
        const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)slice, (int)__builtin_ctzll(rest)); // < cz
        const bool mine = inside && slice == s;
        rest &= ~__ballot(mine);
        const uint32_t *pair = j.cluster_offset_image + 2u * ((size_t)tx + (size_t)ty * cx + (size_t)s * cx * cy);
        const uint32_t offset = pair[0], count = pair[1];
        const uint32_t cn = count < ORBIT_SHADE_MAX_WALK ? count : ORBIT_SHADE_MAX_WALK;
        bool bad = (uint64_t)offset + cn > (uint64_t)j.index_capacity; // (wave-uniform)
        for (uint32_t c = 0; c < cn && !bad; c += 64u) {
            const uint32_t i = c + lane;
            const bool have = i < cn;
            const uint32_t index = have ? indices[(size_t)offset + i] : 0u;
            if (__ballot(have && index >= j.light_count) != 0ull) {
                bad = true;
                break;
            }
            if (j.render_mode != 0u) continue;
            if (have) shade_light_row(shade_load_row(j.lights, index), table[lane]);
            wave_lds_sync();
            const uint32_t m = cn - c < 64u ? cn - c : 64u;
            for (uint32_t k = 0; k < m; k++) { // (wave-uniform: table[k] is one address for the wave)
                const ShadeLight l = table[k];
                if (mine) shade_pixel_light(l, j.luminance_cutoff, px);
            }
            wave_lds_sync(); // (the next chunk's writes stay behind these reads)
        }
        if (mine) {
            if (bad) verdict = kShadeStale;
            else n = cn;
        }
    }
    if (!live || verdict != kShadeWritten) return verdict;
    marks = (inside ? 0u : kShadeOutside) | (px.textured ? kShadeTextured : 0u);
    if (j.render_mode == 0u) {
        if (shade_pixel_end(px, color)) marks |= kShadeDegenerate;
        if (px.unserved) marks |= kShadeUnserved;
    } else {
        shade_heat(n, color);
    }
    return kShadeWritten;
}

template <bool STAGED>
__global__ __launch_bounds__(kThreads) void shade_kernel(const OrbitFragmentsShade j, const uint32_t tiles_x, const uint32_t tiles,
                                                         int32_t *status) {
    __shared__ ShadeLight table[STAGED ? kWaves : 1u][STAGED ? 64u : 1u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t stride = gridDim.x * kWaves;
    uint32_t count[kStatWords] = {}; // wave-uniform
    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < tiles; tile += stride) { // (wave-uniform)
        const uint32_t x0 = (tile % tiles_x) * 8u, y0 = (tile / tiles_x) * 8u;
        const uint32_t x = x0 + (lane & 7u), y = y0 + (lane >> 3);
        const bool in_target = x < j.width && y < j.height;
        const size_t p = (size_t)y * j.width + x;
        const uint64_t word = in_target ? j.visibility[p] : 0ull;
        const bool covered = word != 0ull;
        const uint64_t any = __ballot(covered);
        count[kCovered] += (uint32_t)__popcll(any);
        if (any == 0ull) continue; // (wave-uniform)
        // L2's slice by the mark stage's own function (the whole wave calls it: an uncovered lane takes a harmless depth)
        const float d = __uint_as_float((uint32_t)(word >> 32));
        const uint32_t slice = depth_slice(covered ? j.z_near / d : 1.5f, j.z_scale, j.z_bias);
        float color[4];
        uint32_t n = 0u, marks = 0u, verdict = kShadeUnshaded;
        if (STAGED) {
            verdict = shade_pixel_staged(j, table[wave], lane, covered, x0 / j.tile_size_px, y0 / j.tile_size_px, p, slice, color, n, marks);
        } else if (covered) {
            verdict = shade_pixel(j, x, y, p, slice, color, n, marks); // (in_target: p lies inside every plane)
        }
        const bool written = covered && verdict == kShadeWritten;
        count[kWritten] += (uint32_t)__popcll(__ballot(written));
        count[kUnshaded] += (uint32_t)__popcll(__ballot(covered && verdict == kShadeUnshaded));
        count[kStale] += (uint32_t)__popcll(__ballot(covered && verdict == kShadeStale));
        count[kOutside] += (uint32_t)__popcll(__ballot(written && (marks & kShadeOutside) != 0u));
        count[kDegenerate] += (uint32_t)__popcll(__ballot(written && (marks & kShadeDegenerate) != 0u));
        count[kTextured] += (uint32_t)__popcll(__ballot(written && (marks & kShadeTextured) != 0u));
        count[kUnserved] += (uint32_t)__popcll(__ballot(written && (marks & kShadeUnserved) != 0u));
        if (written) { // (the next tile's ballots see the whole wave again)
            Words4 r;
            for (int i = 0; i < 4; i++) r.w[i] = (uint32_t)float_bits(color[i]);
            *(Words4 *)(j.color + 4u * p) = r;
            if (j.lights_walked) j.lights_walked[p] = n;
        }
    }
    if (lane != 0u) return;
    if (count[kStale] != 0u) latch_status(status, ORBIT_E_RANGE);
    if (!j.stats) return;
    uint32_t *stats = (uint32_t *)j.stats;
    for (uint32_t i = 0; i < kStatWords; i++)
        if (count[i] != 0u) atomicAdd(&stats[i], count[i]);
}

} // namespace

static bool fragments_shade_staged(const OrbitFragmentsShade &job) {
    if (job.flags & ORBIT_SHADE_FORCE_PER_LANE) return false;
    return job.tile_size_px % 8u == 0u; // the default of eligible grids: DESIGN.md §4.25's decision rule
}

hipError_t launch_fragments_shade(const OrbitFragmentsShade &job, uint32_t num_cus, uint32_t grid_cap, int32_t *status, hipStream_t s) {
    const uint32_t resident = (num_cus ? num_cus : 64u) * 8u;
    const uint32_t cap = grid_cap != 0u && grid_cap < resident ? grid_cap : resident; // orbit_ctx_set_visibility_grid
    const size_t pixels = (size_t)job.width * job.height; // width, height <= 32768: at most 2^30
    const bool fill = (job.flags & ORBIT_SHADE_CLEAR) != 0u;
    if (fill || job.stats) {
        const size_t need = fill ? (4u * pixels + kThreads * 4u - 1u) / (kThreads * 4u) : 1u;
        hipLaunchKernelGGL(shade_clear_kernel, dim3((uint32_t)(need < cap ? need : cap)), dim3(kThreads), 0, s,
                           fill ? (uint32_t *)job.color : nullptr, fill ? job.lights_walked : nullptr, pixels, (uint32_t *)job.stats);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint32_t tiles_x = (job.width + 7u) / 8u, tiles = tiles_x * ((job.height + 7u) / 8u); // at most 2^24
    const uint32_t need = (tiles + kWaves - 1u) / kWaves;
    if (fragments_shade_staged(job))
        hipLaunchKernelGGL(shade_kernel<true>, dim3(need < cap ? need : cap), dim3(kThreads), 0, s, job, tiles_x, tiles, status);
    else
        hipLaunchKernelGGL(shade_kernel<false>, dim3(need < cap ? need : cap), dim3(kThreads), 0, s, job, tiles_x, tiles, status);
    return hipGetLastError();
}

} // namespace orbit
