// fragments_shade_shadowed.hip — orbit_fragments_shade_shadowed (include/orbit_abi_ext.h H1-H10 on top of L1-L9,
// DESIGN.md §4.26): orbit_fragments_shade with the shadowed directional lights served — cascade selection, bias, the
// 12-tap blocker search and the 32 x 4-tap filter over the caller's float depth maps.  The arithmetic is shade_common.h's
// and shadow_common.h's, shared with the host mirror, which is the pin.
//
// Two launches on the stream, as fragments_shade.hip's, no look-back, no spinning, nothing handed between workgroups:
//   clear  stats and shadow_stats = 0, and with ORBIT_SHADE_CLEAR color, lights_walked, shadow_factor (1.0f) and cascade
//          (0xFFFFFFFF)
//   shade  a wave takes an 8 x 8 pixel tile and a lane a pixel.  The two forms of the light walk are fragments_shade.hip's
//          (per lane; staged through the wave's own LDS table when tile_size_px % 8 == 0), chosen by the same flags under
//          the same rule.  H1's range check of a shadow row runs where the light's index is checked: per lane in the one
//          form, by the staging lane in the other (a bad row marks the pixels of that slice stale: exactly those whose
//          walk contains the light).  H2-H8 run per lane inside either form: the taps are a pixel's own gathers, the
//          offset table is read at wave-uniform indices from constant memory.  Lanes whose blocker count is 0 or 12 idle
//          while their neighbours filter (DESIGN.md §4.26 counts how often).
//          The counters are wave-uniform sums: one atomic each per wave at the end.
#include "kernels.h"
#include "orbit_device.h"
#include "shadow_common.h"

namespace orbit {
namespace {

using namespace raster;

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;

// OrbitShadeStats' order, then OrbitShadowStats'
enum : uint32_t {
    kCovered, kWritten, kUnshaded, kStale, kOutside, kDegenerate, kTextured, kUnserved, kBaseWords = 8,
    kShadowed = 8, kNoCascade, kEarlyOut, kEvaluations, kStatWords = 12
};

// a pixel's record of a plane that is only known to be 4-B aligned: one access of 12 or 16 bytes
struct __attribute__((packed, aligned(4))) Words3 {
    uint32_t w[3];
};
struct __attribute__((packed, aligned(4))) Words4 {
    uint32_t w[4];
};

__global__ __launch_bounds__(kThreads) void shadowed_clear_kernel(uint32_t *color, uint32_t *lights_walked, uint32_t *shadow_factor,
                                                                  uint32_t *cascade, const size_t pixels, uint32_t *stats,
                                                                  uint32_t *shadow_stats) {
    const size_t stride = (size_t)gridDim.x * kThreads, first = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (stats && first < kBaseWords) stats[first] = 0u;
    if (shadow_stats && first < kStatWords - kBaseWords) shadow_stats[first] = 0u;
    if (color)
        for (size_t i = first; i < 4u * pixels; i += stride) color[i] = 0u;
    if (lights_walked)
        for (size_t i = first; i < pixels; i += stride) lights_walked[i] = 0u;
    if (shadow_factor)
        for (size_t i = first; i < pixels; i += stride) shadow_factor[i] = 0x3F800000u; // 1.0f
    if (cascade)
        for (size_t i = first; i < pixels; i += stride) cascade[i] = kNone;
}

// the wave's LDS writes before, its LDS reads behind (handoff.h's idiom)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The staged form of one tile: L1-L8 with H of the lane's covered pixel p = (x, y) through the wave's table -> the
// verdict, as shadow_shade_pixel's.  Called by the whole wave; `covered` lanes lie in the target.  tx, ty: the tile's
// cluster column.
__device__ __forceinline__ uint32_t shadowed_pixel_staged(const OrbitFragmentsShadeShadowed &j, ShadeLight *table, uint32_t lane, bool covered,
                                                          uint32_t tx, uint32_t ty, uint32_t x, uint32_t y, size_t p, uint32_t slice,
                                                          float *color, uint32_t &n, uint32_t &marks, ShadowPixel &sp) {
    const OrbitFragmentsShade &b = j.shade;
    n = 0u, marks = 0u;
    for (int i = 0; i < 4; i++) color[i] = 0.0f;
    shadow_pixel_begin(1.0f, sp);
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
            sp.w = wpf[3];
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
            if (b.render_mode != 0u) { // H9: the type and the shadow index for H1, nothing else of the row
                const bool ok = !have || shadow_light_checked(j, b.lights[index].light_type, b.lights[index].shadow_data_index);
                if (__ballot(!ok) != 0ull) {
                    bad = true;
                    break;
                }
                continue;
            }
            ShadeLight row = {};
            if (have) shade_light_row(shade_load_row(b.lights, index), row);
            if (__ballot(have && !shadow_light_checked(j, row.type, row.shadow)) != 0ull) { // H1
                bad = true;
                break;
            }
            if (have) table[lane] = row;
            wave_lds_sync();
            const uint32_t m = cn - c < 64u ? cn - c : 64u;
            for (uint32_t k = 0; k < m; k++) { // (wave-uniform: table[k] is one address for the wave)
                const ShadeLight l = table[k];
                if (mine && !sp.stale) shadow_pixel_light(j, l, x, y, px, sp);
            }
            wave_lds_sync(); // (the next chunk's writes stay behind these reads)
        }
        if (mine) {
            if (bad || sp.stale) verdict = kShadeStale;
            else n = cn;
        }
    }
    if (!live || verdict != kShadeWritten) return verdict;
    marks = (inside ? 0u : kShadeOutside) | (px.textured ? kShadeTextured : 0u);
    if (b.render_mode == 0u) {
        if (shade_pixel_end(px, color)) marks |= kShadeDegenerate;
        if (px.unserved) marks |= kShadeUnserved;
        finite_or_zero(sp.factor);
    } else {
        shade_heat(n, color);
    }
    return kShadeWritten;
}

template <bool STAGED>
__global__ __launch_bounds__(kThreads) void shadowed_kernel(const OrbitFragmentsShadeShadowed j, const uint32_t tiles_x, const uint32_t tiles,
                                                            int32_t *status) {
    __shared__ ShadeLight table[STAGED ? kWaves : 1u][STAGED ? 64u : 1u];
    const OrbitFragmentsShade &b = j.shade;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t stride = gridDim.x * kWaves;
    uint32_t count[kStatWords] = {}; // wave-uniform
    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < tiles; tile += stride) { // (wave-uniform)
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
        ShadowPixel sp;
        shadow_pixel_begin(1.0f, sp);
        if (STAGED) {
            verdict = shadowed_pixel_staged(j, table[wave], lane, covered, x0 / b.tile_size_px, y0 / b.tile_size_px, x, y, p, slice, color, n,
                                            marks, sp);
        } else if (covered) {
            verdict = shadow_shade_pixel(j, x, y, p, slice, color, n, marks, sp); // (in_target: p lies inside every plane)
        }
        const bool written = covered && verdict == kShadeWritten;
        count[kWritten] += (uint32_t)__popcll(__ballot(written));
        count[kUnshaded] += (uint32_t)__popcll(__ballot(covered && verdict == kShadeUnshaded));
        count[kStale] += (uint32_t)__popcll(__ballot(covered && verdict == kShadeStale));
        count[kOutside] += (uint32_t)__popcll(__ballot(written && (marks & kShadeOutside) != 0u));
        count[kDegenerate] += (uint32_t)__popcll(__ballot(written && (marks & kShadeDegenerate) != 0u));
        count[kTextured] += (uint32_t)__popcll(__ballot(written && (marks & kShadeTextured) != 0u));
        count[kUnserved] += (uint32_t)__popcll(__ballot(written && (marks & kShadeUnserved) != 0u));
        const uint64_t shadowed = __ballot(written && (sp.marks & kShadowEvaluated) != 0u);
        if (shadowed != 0ull) { // (wave-uniform)
            count[kShadowed] += (uint32_t)__popcll(shadowed);
            count[kNoCascade] += (uint32_t)__popcll(__ballot(written && (sp.marks & kShadowOutOfCascades) != 0u));
            count[kEarlyOut] += (uint32_t)__popcll(__ballot(written && (sp.marks & kShadowEarlyOut) != 0u));
            uint32_t evaluations = written ? sp.evaluations : 0u; // at most 256 each: the wave's sum fits
            for (int o = 32; o > 0; o >>= 1) evaluations += (uint32_t)__shfl_xor((int)evaluations, o, 64);
            count[kEvaluations] += (uint32_t)__builtin_amdgcn_readfirstlane((int)evaluations);
        }
        if (written) { // (the next tile's ballots see the whole wave again)
            Words4 r;
            for (int i = 0; i < 4; i++) r.w[i] = (uint32_t)float_bits(color[i]);
            *(Words4 *)(b.color + 4u * p) = r;
            if (b.lights_walked) b.lights_walked[p] = n;
            if (j.shadow_factor) j.shadow_factor[p] = sp.factor;
            if (j.cascade) j.cascade[p] = sp.cascade;
        }
    }
    if (lane != 0u) return;
    if (count[kStale] != 0u) latch_status(status, ORBIT_E_RANGE);
    if (b.stats) {
        uint32_t *stats = (uint32_t *)b.stats;
        for (uint32_t i = 0; i < kBaseWords; i++)
            if (count[i] != 0u) atomicAdd(&stats[i], count[i]);
    }
    if (j.shadow_stats) {
        uint32_t *stats = (uint32_t *)j.shadow_stats;
        for (uint32_t i = kBaseWords; i < kStatWords; i++)
            if (count[i] != 0u) atomicAdd(&stats[i - kBaseWords], count[i]);
    }
}

} // namespace

static bool fragments_shade_shadowed_staged(const OrbitFragmentsShade &job) {
    if (job.flags & ORBIT_SHADE_FORCE_PER_LANE) return false;
    return job.tile_size_px % 8u == 0u; // orbit_fragments_shade's rule
}

hipError_t launch_fragments_shade_shadowed(const OrbitFragmentsShadeShadowed &job, uint32_t num_cus, uint32_t grid_cap, int32_t *status,
                                           hipStream_t s) {
    const OrbitFragmentsShade &b = job.shade;
    const uint32_t resident = (num_cus ? num_cus : 64u) * 8u;
    const uint32_t cap = grid_cap != 0u && grid_cap < resident ? grid_cap : resident; // orbit_ctx_set_visibility_grid
    const size_t pixels = (size_t)b.width * b.height; // width, height <= 32768: at most 2^30
    const bool fill = (b.flags & ORBIT_SHADE_CLEAR) != 0u;
    if (fill || b.stats || job.shadow_stats) {
        const size_t need = fill ? (4u * pixels + kThreads * 4u - 1u) / (kThreads * 4u) : 1u;
        hipLaunchKernelGGL(shadowed_clear_kernel, dim3((uint32_t)(need < cap ? need : cap)), dim3(kThreads), 0, s,
                           fill ? (uint32_t *)b.color : nullptr, fill ? b.lights_walked : nullptr, fill ? (uint32_t *)job.shadow_factor : nullptr,
                           fill ? job.cascade : nullptr, pixels, (uint32_t *)b.stats, (uint32_t *)job.shadow_stats);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint32_t tiles_x = (b.width + 7u) / 8u, tiles = tiles_x * ((b.height + 7u) / 8u); // at most 2^24
    const uint32_t need = (tiles + kWaves - 1u) / kWaves;
    if (fragments_shade_shadowed_staged(b))
        hipLaunchKernelGGL(shadowed_kernel<true>, dim3(need < cap ? need : cap), dim3(kThreads), 0, s, job, tiles_x, tiles, status);
    else
        hipLaunchKernelGGL(shadowed_kernel<false>, dim3(need < cap ? need : cap), dim3(kThreads), 0, s, job, tiles_x, tiles, status);
    return hipGetLastError();
}

} // namespace orbit
