// shade_walk.h — what the three shade calls' kernel units (fragments_shade.hip, fragments_shade_shadowed.hip,
// fragments_shade_sky.hip) share beyond the arithmetic: the staged walk, the tile loop and the launch, each over a tier
// (shade_common.h ShadeTier, shadow_common.h ShadowedTier, sky_common.h SkyTier).  Device only.
//
// A call is two launches on the stream, no look-back, no spinning, nothing handed from one workgroup to another:
//   clear  fragments_shade.hip's launch_shade_clear: the stats blocks = 0, and with ORBIT_SHADE_CLEAR the planes
//   shade  a wave takes an 8 x 8 pixel tile (out-of-target lanes carry 0) and a lane a pixel, as the buffer's other
//          readers do.  Two forms, equal bytes (every pixel adds its own list in list order):
//          per lane  each lane runs shade_walk_pixel: its own (offset, n), its own gathers of index and 64-B light row,
//                    its own check of the row.
//          staged    tile_size_px % 8 == 0: the wave's 64 pixels share one cluster column.  The wave loops over the
//                    distinct slices among its lanes (a wave-uniform ballot); per slice the cluster's list goes in
//                    chunks of 64: lane i loads index i and its light row, range-checks both and writes the 16 words
//                    L5 / L6 read to the wave's own 4-KB LDS table; then every lane of that slice runs the tier's light
//                    over the chunk from LDS at a wave-uniform address (a broadcast: no bank conflict).  A bad index or
//                    row marks the pixels of that slice stale: exactly those whose walk contains it.  No __syncthreads:
//                    the table is the wave's own, a wave-level fence orders its writes and reads.
//          The counters are wave-uniform popcounts and sums: one atomic each per wave at the end.
// A unit adds its tier's device half to the tier: kWords (how far into the stat words below it counts), count (its words
// of one tile), store (its planes of a written pixel) and flush (its stats blocks, by lane 0 at the end).
#pragma once
#include "kernels.h"
#include "orbit_device.h"
#include "shadow_common.h"

namespace orbit {

using namespace raster;

constexpr uint32_t kShadeThreads = 256, kShadeWaves = kShadeThreads / 64;

// OrbitShadeStats' order, then OrbitShadowStats', then OrbitSkyStats' (bad_directions: the u64 at word 4 of its block)
enum : uint32_t {
    kCovered, kWritten, kUnshaded, kStale, kOutside, kDegenerate, kTextured, kUnserved, kBaseWords = 8,
    kShadowed = 8, kNoCascade, kEarlyOut, kEvaluations, kShadowEnd = 12,
    kSkyEvaluations = 12, kSkyLit, kSkybox, kBad, kStatWords = 16
};

// a pixel's record of a plane that is only known to be 4-B aligned: one access of 12 or 16 bytes
struct __attribute__((packed, aligned(4))) Words3 {
    uint32_t w[3];
};
struct __attribute__((packed, aligned(4))) Words4 {
    uint32_t w[4];
};

// the wave's LDS writes before, its LDS reads behind (handoff.h's idiom)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a wave's sum of a lane value (each at most 2^9: the sum fits)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

__device__ __forceinline__ uint32_t wave_count(bool b) { return (uint32_t)__popcll(__ballot(b)); }

// The device half of ShadowPixel, for the shadowed tier and the sky tier: H10's counters, planes and stats block
__device__ __forceinline__ void shadow_count(uint32_t *count, bool written, const ShadowPixel &sp) {
    const uint64_t shadowed = __ballot(written && (sp.marks & kShadowEvaluated) != 0u);
    if (shadowed == 0ull) return; // (wave-uniform)
    count[kShadowed] += (uint32_t)__popcll(shadowed);
    count[kNoCascade] += wave_count(written && (sp.marks & kShadowOutOfCascades) != 0u);
    count[kEarlyOut] += wave_count(written && (sp.marks & kShadowEarlyOut) != 0u);
    count[kEvaluations] += wave_sum(written ? sp.evaluations : 0u); // at most 256 each
}
__device__ __forceinline__ void shadow_store(const OrbitFragmentsShadeShadowed &j, size_t p, const ShadowPixel &sp) {
    if (j.shadow_factor) j.shadow_factor[p] = sp.factor;
    if (j.cascade) j.cascade[p] = sp.cascade;
}
__device__ __forceinline__ void shadow_flush(const OrbitFragmentsShadeShadowed &j, const uint32_t *count) {
    if (!j.shadow_stats) return;
    uint32_t *stats = (uint32_t *)j.shadow_stats;
    for (uint32_t i = kBaseWords; i < kShadowEnd; i++)
        if (count[i] != 0u) atomicAdd(&stats[i - kBaseWords], count[i]);
}

// The staged form of one tile: L1-L8 of the lane's covered pixel p = (x, y) through the wave's table in tier t -> the
// verdict, as shade_walk_pixel's.  Called by the whole wave; `covered` lanes lie in the target.  tx, ty: the tile's
// cluster column.
template <class Tier>
__device__ __forceinline__ uint32_t shade_walk_staged(const Tier &t, const typename Tier::Job &j, ShadeLight *table, uint32_t lane, bool covered,
                                                      uint32_t tx, uint32_t ty, uint32_t x, uint32_t y, size_t p, uint32_t slice, float *color,
                                                      uint32_t &n, uint32_t &marks, typename Tier::Extra &e) {
    const OrbitFragmentsShade &b = Tier::base(j);
    n = 0u, marks = 0u;
    for (int i = 0; i < 4; i++) color[i] = 0.0f;
    uint32_t verdict = kShadeUnshaded;
    ShadePixel px = {};
    if (covered) {
        const uint32_t material = b.material[p];
        verdict = shade_material_verdict(b, material);
        if (verdict == kShadeWritten) {
            const OrbitMaterialData m = shade_load_row(b.materials, material);
            Words4 wp = *(const Words4 *)(b.world_pos + 4u * p);
            Words3 nrm = *(const Words3 *)(b.normal + 3u * p);
            float wpf[4], nf[3];
            __builtin_memcpy(wpf, &wp, 16);
            __builtin_memcpy(nf, &nrm, 12);
            shade_pixel_begin(b, m, wpf, nf, px);
            t.begin(j, m, wpf, p, e);
        }
    }
    const bool live = covered && verdict == kShadeWritten;
    const uint32_t cx = b.cluster_count[0], cy = b.cluster_count[1], cz = b.cluster_count[2];
    const bool inside = live && tx < cx && ty < cy && slice < cz;
    const uint32_t *indices = shade_indices(b);
    uint64_t rest = __ballot(inside); // (wave-uniform)
    while (rest != 0ull) {
        const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)slice, (int)__builtin_ctzll(rest)); // < cz
        const bool mine = inside && slice == s;
        rest &= ~__ballot(mine);
        const uint32_t *pair = b.cluster_offset_image + 2u * ((size_t)tx + (size_t)ty * cx + (size_t)s * cx * cy);
        const uint32_t offset = pair[0], count = pair[1];
        const uint32_t cn = count < ORBIT_SHADE_MAX_WALK ? count : ORBIT_SHADE_MAX_WALK;
        bool bad = (uint64_t)offset + cn > (uint64_t)b.index_capacity; // (wave-uniform)
        for (uint32_t c = 0; c < cn && !bad; c += 64u) {
            const uint32_t i = c + lane;
            const bool have = i < cn;
            const uint32_t index = have ? indices[(size_t)offset + i] : 0u;
            if (__ballot(have && index >= b.light_count) != 0ull) {
                bad = true;
                break;
            }
            if (b.render_mode != 0u) { // the type and the shadow index for the tier's check, nothing else of the row
                const bool ok = !have || Tier::light_checked(j, b.lights[index].light_type, b.lights[index].shadow_data_index);
                if (__ballot(!ok) != 0ull) {
                    bad = true;
                    break;
                }
                continue;
            }
            ShadeLight row = {};
            if (have) shade_light_row(shade_load_row(b.lights, index), row);
            if (__ballot(have && !Tier::light_checked(j, row.type, row.shadow)) != 0ull) {
                bad = true;
                break;
            }
            if (have) table[lane] = row;
            wave_lds_sync();
            const uint32_t m = cn - c < 64u ? cn - c : 64u;
            for (uint32_t k = 0; k < m; k++) { // (wave-uniform: table[k] is one address for the wave)
                const ShadeLight l = table[k];
                if (mine && !Tier::stale(e)) t.light(j, l, x, y, px, e);
            }
            wave_lds_sync(); // (the next chunk's writes stay behind these reads)
        }
        if (mine) {
            if (bad || Tier::stale(e)) verdict = kShadeStale;
            else n = cn;
        }
    }
    if (!live || verdict != kShadeWritten) return verdict;
    marks = shade_walk_end<Tier>(b, !inside, n, px, color, e);
    return kShadeWritten;
}

// The body of a shade kernel: the tiles of a wave in trips of the grid, in the form STAGED says
template <class Tier, bool STAGED>
__device__ __forceinline__ void shade_tiles(const typename Tier::Job &j, const uint32_t tiles_x, const uint32_t tiles, int32_t *status) {
    __shared__ ShadeLight table[STAGED ? kShadeWaves : 1u][STAGED ? 64u : 1u];
    const Tier t = {};
    const OrbitFragmentsShade &b = Tier::base(j);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t stride = gridDim.x * kShadeWaves;
    uint32_t count[Tier::kWords] = {}; // wave-uniform
    for (uint32_t tile = blockIdx.x * kShadeWaves + wave; tile < tiles; tile += stride) { // (wave-uniform)
        const uint32_t x0 = (tile % tiles_x) * 8u, y0 = (tile / tiles_x) * 8u;
        const uint32_t x = x0 + (lane & 7u), y = y0 + (lane >> 3);
        const bool in_target = x < b.width && y < b.height;
        const size_t p = (size_t)y * b.width + x;
        const uint64_t word = in_target ? b.visibility[p] : 0ull;
        const bool covered = word != 0ull;
        const uint64_t any = __ballot(covered);
        count[kCovered] += (uint32_t)__popcll(any);
        if (any == 0ull) continue; // (wave-uniform)
        // L2's slice by the mark stage's own function (the whole wave calls it: an uncovered lane takes a harmless depth)
        const float d = __uint_as_float((uint32_t)(word >> 32));
        const uint32_t slice = depth_slice(covered ? b.z_near / d : 1.5f, b.z_scale, b.z_bias);
        float color[4];
        uint32_t n = 0u, marks = 0u, verdict = kShadeUnshaded;
        typename Tier::Extra e;
        Tier::reset(e);
        if (STAGED) {
            verdict = shade_walk_staged(t, j, table[wave], lane, covered, x0 / b.tile_size_px, y0 / b.tile_size_px, x, y, p, slice, color, n, marks, e);
        } else if (covered) {
            verdict = shade_walk_pixel(t, j, x, y, p, slice, color, n, marks, e); // (in_target: p lies inside every plane)
        }
        const bool written = covered && verdict == kShadeWritten;
        count[kWritten] += wave_count(written);
        count[kUnshaded] += wave_count(covered && verdict == kShadeUnshaded);
        count[kStale] += wave_count(covered && verdict == kShadeStale);
        count[kOutside] += wave_count(written && (marks & kShadeOutside) != 0u);
        count[kDegenerate] += wave_count(written && (marks & kShadeDegenerate) != 0u);
        count[kTextured] += wave_count(written && (marks & kShadeTextured) != 0u);
        count[kUnserved] += wave_count(written && (marks & kShadeUnserved) != 0u);
        Tier::count(count, written, e);
        if (written) { // (the next tile's ballots see the whole wave again)
            Words4 r;
            for (int i = 0; i < 4; i++) r.w[i] = (uint32_t)float_bits(color[i]);
            *(Words4 *)(b.color + 4u * p) = r;
            if (b.lights_walked) b.lights_walked[p] = n;
            Tier::store(j, p, e);
        }
    }
    if (lane != 0u) return;
    if (count[kStale] != 0u) latch_status(status, ORBIT_E_RANGE);
    if (b.stats) {
        uint32_t *stats = (uint32_t *)b.stats;
        for (uint32_t i = 0; i < kBaseWords; i++)
            if (count[i] != 0u) atomicAdd(&stats[i], count[i]);
    }
    Tier::flush(j, count);
}

// The launch shape of a call: the grid cap (orbit_ctx_set_visibility_grid), the 8 x 8 tiles, the workgroups of the tile
// loop and its form — staged by default on eligible grids (DESIGN.md §4.25's decision rule)
struct ShadeGrid {
    uint32_t cap, tiles_x, tiles, blocks;
    bool staged;
};
inline ShadeGrid shade_grid(const OrbitFragmentsShade &b, uint32_t num_cus, uint32_t grid_cap) {
    ShadeGrid g;
    const uint32_t resident = (num_cus ? num_cus : 64u) * 8u;
    g.cap = grid_cap != 0u && grid_cap < resident ? grid_cap : resident;
    g.tiles_x = (b.width + 7u) / 8u, g.tiles = g.tiles_x * ((b.height + 7u) / 8u); // at most 2^24
    const uint32_t need = (g.tiles + kShadeWaves - 1u) / kShadeWaves;
    g.blocks = need < g.cap ? need : g.cap;
    g.staged = !(b.flags & ORBIT_SHADE_FORCE_PER_LANE) && b.tile_size_px % 8u == 0u;
    return g;
}

// the tile loop of a call in its form
template <class Job>
hipError_t launch_shade_tiles(void (*staged)(Job, uint32_t, uint32_t, int32_t *), void (*per_lane)(Job, uint32_t, uint32_t, int32_t *),
                              const Job &job, const ShadeGrid &g, int32_t *status, hipStream_t s) {
    hipLaunchKernelGGL(g.staged ? staged : per_lane, dim3(g.blocks), dim3(kShadeThreads), 0, s, job, g.tiles_x, g.tiles, status);
    return hipGetLastError();
}

} // namespace orbit
