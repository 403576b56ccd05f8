// fragments_shade_sky.hip — orbit_fragments_shade_sky (include/orbit_abi_ext.h K1-K10 on top of H1-H10 and L1-L9, DESIGN.md
// §4.31): orbit_fragments_shade_shadowed with the SKY lights served from the environment's three images and the uncovered
// pixels filled from the sky cube.  The arithmetic is shade_common.h's, shadow_common.h's, env_common.h's and
// sky_common.h's, shared with the host mirror, which is the pin.
//
// Two or three launches on the stream, no look-back, no spinning, nothing handed between workgroups:
//   clear  stats, shadow_stats and sky_stats = 0, and with ORBIT_SHADE_CLEAR color, lights_walked, shadow_factor (1.0f)
//          and cascade (0xFFFFFFFF)
//   shade  fragments_shade_shadowed.hip's launch: a wave takes an 8 x 8 pixel tile and a lane a pixel, the two forms of the
//          light walk chosen by the same flags under the same rule.  Built twice: without the environment it is the shadowed
//          unit's kernel, and a call that gives none pays nothing for K.  With it, K1's branch sits where
//          shadow_pixel_light is called: in the staged form the light is table[k], one row for the wave, so the branch is
//          taken by every lane of the slice or by none; the cube and table gathers are a lane's own (the offsets of a
//          cube's levels are wave-uniform and picked by a select chain: nothing is indexed by a lane's value).
//   box    K9, where sky is given and the mode is 0: the same tiles in the same trips under the same grid cap, the lanes
//          whose visibility word is 0.  A launch of its own: inside the shade launch it cost the lit path 24 VGPRs and
//          with them a wave per SIMD, with or without an environment.
//          The counters are wave-uniform sums: one atomic each per wave at the end.
#include "kernels.h"
#include "orbit_device.h"
#include "sky_common.h"

namespace orbit {
namespace {

using namespace raster;

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;

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

__global__ __launch_bounds__(kThreads) void sky_clear_kernel(uint32_t *color, uint32_t *lights_walked, uint32_t *shadow_factor, uint32_t *cascade,
                                                             const size_t pixels, uint32_t *stats, uint32_t *shadow_stats, uint32_t *sky_stats) {
    const size_t stride = (size_t)gridDim.x * kThreads, first = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (stats && first < kBaseWords) stats[first] = 0u;
    if (shadow_stats && first < kShadowEnd - kBaseWords) shadow_stats[first] = 0u;
    if (sky_stats && first < sizeof(OrbitSkyStats) / 4u) sky_stats[first] = 0u;
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

// a wave's sum of a lane value (each at most 2^9: the sum fits)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// The staged form of one tile: L1-L8 with H and K of the lane's covered pixel p = (x, y) through the wave's table -> the
// verdict, as sky_shade_pixel's.  Called by the whole wave; `covered` lanes lie in the target.  tx, ty: the tile's
// cluster column.
template <bool ENV>
__device__ __forceinline__ uint32_t sky_pixel_staged(const OrbitFragmentsShadeSky &js, ShadeLight *table, uint32_t lane,
                                                     bool covered, uint32_t tx, uint32_t ty, uint32_t x, uint32_t y, size_t p, uint32_t slice,
                                                     float *color, uint32_t &n, uint32_t &marks, ShadowPixel &sp, SkyPixel &sk) {
    const OrbitFragmentsShadeShadowed &j = js.shadowed;
    const OrbitFragmentsShade &b = j.shade;
    n = 0u, marks = 0u;
    for (int i = 0; i < 4; i++) color[i] = 0.0f;
    shadow_pixel_begin(1.0f, sp);
    sk.roughness = 0.0f, sk.ao = 1.0f, sk.evaluations = 0u, sk.bad = 0u;
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
            if (ENV && sky_env_given(js)) sky_pixel_begin(js, m.roughness_factor, p, sk); // (ao has no other reader)
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
                if (mine && !sp.stale) sky_pixel_light<ENV>(js, l, x, y, px, sp, sk);
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

// ENV: the environment is given (K1-K8 are built in; without it the kernel is the shadowed unit's, instruction for instruction
// but for sky_stats)
template <bool STAGED, bool ENV>
__global__ __launch_bounds__(kThreads) void sky_kernel(const OrbitFragmentsShadeSky js, const uint32_t tiles_x, const uint32_t tiles,
                                                       int32_t *status) {
    __shared__ ShadeLight table[STAGED ? kWaves : 1u][STAGED ? 64u : 1u];
    const OrbitFragmentsShadeShadowed &j = js.shadowed;
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
        SkyPixel sk = {0.0f, 1.0f, 0u, 0u};
        shadow_pixel_begin(1.0f, sp);
        if (STAGED) {
            verdict = sky_pixel_staged<ENV>(js, table[wave], lane, covered, x0 / b.tile_size_px, y0 / b.tile_size_px, x, y, p, slice, color, n, marks,
                                            sp, sk);
        } else if (covered) {
            verdict = sky_shade_pixel<ENV>(js, x, y, p, slice, color, n, marks, sp, sk); // (in_target: p lies inside every plane)
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
            count[kEvaluations] += wave_sum(written ? sp.evaluations : 0u); // at most 256 each
        }
        if (ENV) {
            const uint64_t sky_lit = __ballot(written && sk.evaluations != 0u);
            if (sky_lit != 0ull) { // (wave-uniform)
                count[kSkyLit] += (uint32_t)__popcll(sky_lit);
                count[kSkyEvaluations] += wave_sum(written ? sk.evaluations : 0u); // at most 256 each
                count[kBad] += wave_sum(written ? sk.bad : 0u);                    // at most 512 each
            }
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
        for (uint32_t i = kBaseWords; i < kShadowEnd; i++)
            if (count[i] != 0u) atomicAdd(&stats[i - kBaseWords], count[i]);
    }
    if (ENV && js.sky_stats) {
        OrbitSkyStats *stats = js.sky_stats;
        if (count[kSkyEvaluations] != 0u) atomicAdd(&stats->sky_evaluations, count[kSkyEvaluations]);
        if (count[kSkyLit] != 0u) atomicAdd(&stats->sky_lit_pixels, count[kSkyLit]);
        if (count[kBad] != 0u) atomicAdd((unsigned long long *)&stats->bad_directions, (unsigned long long)count[kBad]);
    }
}

// K9, the call's last launch where sky is given and the mode is 0: the same tiles in the same trips, the lanes whose
// visibility word is 0.  A pixel is written by this launch or by the one before it, never by both.
__global__ __launch_bounds__(kThreads) void sky_box_kernel(const OrbitFragmentsShadeSky js, const uint32_t tiles_x, const uint32_t tiles) {
    const OrbitFragmentsShade &b = js.shadowed.shade;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t stride = gridDim.x * kWaves;
    uint32_t boxed = 0u, bad = 0u; // wave-uniform
    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < tiles; tile += stride) { // (wave-uniform)
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

static bool fragments_shade_sky_staged(const OrbitFragmentsShade &job) {
    if (job.flags & ORBIT_SHADE_FORCE_PER_LANE) return false;
    return job.tile_size_px % 8u == 0u; // orbit_fragments_shade's rule
}

hipError_t launch_fragments_shade_sky(const OrbitFragmentsShadeSky &job, uint32_t num_cus, uint32_t grid_cap, int32_t *status, hipStream_t s) {
    const OrbitFragmentsShadeShadowed &j = job.shadowed;
    const OrbitFragmentsShade &b = j.shade;
    const uint32_t resident = (num_cus ? num_cus : 64u) * 8u;
    const uint32_t cap = grid_cap != 0u && grid_cap < resident ? grid_cap : resident; // orbit_ctx_set_visibility_grid
    const size_t pixels = (size_t)b.width * b.height; // width, height <= 32768: at most 2^30
    const bool fill = (b.flags & ORBIT_SHADE_CLEAR) != 0u;
    if (fill || b.stats || j.shadow_stats || job.sky_stats) {
        const size_t need = fill ? (4u * pixels + kThreads * 4u - 1u) / (kThreads * 4u) : 1u;
        hipLaunchKernelGGL(sky_clear_kernel, dim3((uint32_t)(need < cap ? need : cap)), dim3(kThreads), 0, s, fill ? (uint32_t *)b.color : nullptr,
                           fill ? b.lights_walked : nullptr, fill ? (uint32_t *)j.shadow_factor : nullptr, fill ? j.cascade : nullptr, pixels,
                           (uint32_t *)b.stats, (uint32_t *)j.shadow_stats, (uint32_t *)job.sky_stats);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint32_t tiles_x = (b.width + 7u) / 8u, tiles = tiles_x * ((b.height + 7u) / 8u); // at most 2^24
    const uint32_t need = (tiles + kWaves - 1u) / kWaves;
    const dim3 grid(need < cap ? need : cap);
    const bool staged = fragments_shade_sky_staged(b), env = sky_env_given(job);
    if (staged && env) hipLaunchKernelGGL((sky_kernel<true, true>), grid, dim3(kThreads), 0, s, job, tiles_x, tiles, status);
    else if (staged) hipLaunchKernelGGL((sky_kernel<true, false>), grid, dim3(kThreads), 0, s, job, tiles_x, tiles, status);
    else if (env) hipLaunchKernelGGL((sky_kernel<false, true>), grid, dim3(kThreads), 0, s, job, tiles_x, tiles, status);
    else hipLaunchKernelGGL((sky_kernel<false, false>), grid, dim3(kThreads), 0, s, job, tiles_x, tiles, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !sky_box_given(job)) return e;
    hipLaunchKernelGGL(sky_box_kernel, grid, dim3(kThreads), 0, s, job, tiles_x, tiles);
    return hipGetLastError();
}

} // namespace orbit
