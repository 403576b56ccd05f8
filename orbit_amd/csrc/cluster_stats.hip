// cluster_stats.hip — orbit_cluster_stats: the uncapped light counts of the cluster chain (include/orbit_abi_ext.h).
//
// The chain's own arithmetic (cluster_common.h), no output of it: one WAVE owns one screen tile and walks its samples as
// cluster_mark_kernel does (mark_sample, mark_values, mark_slice_bounds), keeping per z slice (lane = slice) the
// number of in-grid samples and the depth bounds in registers.  Lane s then builds cluster s's box with the chain's
// cluster_aabb from those bounds.  A workgroup is a 4 x 4 square of tiles; its lights are transformed as
// light_prepare_body does, a chunk at a time (one light per thread), filtered against the union of the workgroup's
// boxes into LDS, and each wave tests the survivors against its tile's boxes (lane = candidate), a ballot's popcount per
// active slice.  The union is sound because aabb_sphere_test is monotone in the box; a union holding a
// NaN does not filter.  Non-point lights are in every cluster and are counted without a test (light_culling.comp:116).
// Counts go to LDS as 64-bit sums, then one 64-bit atomic per non-zero counter and workgroup: order-independent.
#include "cluster_common.h"

namespace orbit {

namespace {

constexpr uint32_t kStatsSide = 4;                        // a workgroup's tiles: kStatsSide x kStatsSide
constexpr uint32_t kStatsWaves = kStatsSide * kStatsSide; // one wave per tile
constexpr uint32_t kStatsThreads = kStatsWaves * 64;      // = the lights of one chunk
constexpr uint32_t kClasses = 5;                          // 0, 1-16, 17-64, 65-256, > 256 lights

// OrbitClusterStats' words
enum : uint32_t {
    kSamples = 0, kOutside = 1, kActive = 2, kRefs = 3, kIndices = 4, kMaxLights = 5, kSampleRefs = 6,
    kClusterClass = 8, kSampleClass = 16, kWords = 21,
};
static_assert(offsetof(OrbitClusterStats, clusters_by_lights) == 8 * kClusterClass, "word of clusters_by_lights");
static_assert(offsetof(OrbitClusterStats, samples_by_lights) == 8 * kSampleClass, "word of samples_by_lights");
static_assert(kClusterClass + kClasses <= kSampleClass && kSampleClass + kClasses == kWords, "five classes each");
static_assert(offsetof(OrbitClusterStats, max_cluster_lights) == 8 * kMaxLights, "word of max_cluster_lights");

__device__ __forceinline__ uint32_t light_class(uint32_t count) {
    return count == 0u ? 0u : count <= 16u ? 1u : count <= 64u ? 2u : count <= ORBIT_MAX_LIGHTS_PER_CLUSTER ? 3u : 4u;
}

__global__ __launch_bounds__(kStatsThreads) void cluster_stats_kernel(const ClusterStatsParams p) {
    __shared__ float4 s_cand[kStatsThreads];      // view-space point lights behind the union filter
    __shared__ float s_wbox[kStatsWaves][8];      // per wave: a row as union_row_store leaves it (its tile's boxes), and in word 7 whether the tile has a cluster
    __shared__ uint32_t s_ncand[2], s_nonpoint[2]; // per chunk (by parity): candidates, non-point lights
    __shared__ unsigned long long s_cnt[kWords];
    const OrbitMarkActivePush &pc = p.pc;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t cx = pc.cluster_count[0], cy = pc.cluster_count[1], cz = pc.cluster_count[2];
    const uint32_t tiles = cx * cy;
    if (threadIdx.x < kWords) s_cnt[threadIdx.x] = blockIdx.x == 0u && threadIdx.x == kSamples ? p.samples
                                                   : blockIdx.x == 0u && threadIdx.x == kOutside ? p.uncovered : 0ull;
    if (threadIdx.x < 2u) s_ncand[threadIdx.x] = 0u, s_nonpoint[threadIdx.x] = 0u;

    // ---- the tile's samples (cluster_mark_kernel): lane s < cz ends with slice s's in-grid samples and bounds
    const uint32_t bx = max((cx + kStatsSide - 1u) / kStatsSide, 1u); // (an empty grid: one workgroup, no tile)
    const uint32_t tx = (blockIdx.x % bx) * kStatsSide + wave % kStatsSide, ty = (blockIdx.x / bx) * kStatsSide + wave / kStatsSide;
    const bool tile_ok = tx < cx && ty < cy; // (wave-uniform)
    const uint32_t tile = ty * cx + tx;
    uint32_t n_samples = 0, acc_min = 0, acc_max = 0, outside = 0;
    if (tile_ok) {
        const uint32_t items = pc.tile_size_px * pc.tile_size_px * pc.depth_buffer_sample_count;
        for (uint32_t base = 0; base < items; base += 64) {
            size_t index;
            const bool valid = mark_sample(pc, cx, cy, tile, base + lane, index);
            const float d = valid ? p.depth[index] : 0.0f;
            const MarkValues v = mark_values(pc, valid, d);
            const bool in_grid = valid && v.slice < cz;                     // mark_active.comp:31
            outside += (uint32_t)__popcll(__ballot(valid && !in_grid));
            const uint32_t todo = wave_reduce_or(in_grid ? v.bit : 0u);
            mark_slice_bounds(todo, v, lane, acc_min, acc_max, [&](uint32_t s, bool mine) {
                const uint32_t n = (uint32_t)__popcll(__ballot(mine));
                n_samples += lane == s ? n : 0u;
            });
        }
    }
    const bool active = n_samples != 0u; // (lane < cz only)
    const uint64_t active_mask = __ballot(active);

    // ---- lane s: cluster s's box (light_culling.comp:62-90), the wave's union of them, the workgroup's union
    Aabb3 box;
    box_empty(box.mn, box.mx);
    if (active) {
        OrbitClusterDepthBounds db;
        db.min_depth = acc_min;
        db.max_depth = acc_max;
        box = cluster_aabb(p.info, tile + lane * tiles, db);
    }
    {
        Aabb3 u = box;
        const bool wave_nan = lanes_union<64>(u.mn, u.mx);
        if (lane == 0) {
            union_row_store(s_wbox[wave], u.mn, u.mx, wave_nan);
            s_wbox[wave][7] = active_mask != 0ull ? 1.0f : 0.0f;
        }
    }
    __syncthreads();
    // (not union_rows: its sixteen rows a few at a time cost the regime scene 1 us of this call's 36 — DESIGN.md 4.17.  The
    // rows' NaN flags are the lanes': a row holds a NaN only if its flag is set.)
    BoxUnion un = union_empty();
    bool any_active = false;
    for (uint32_t w = 0; w < kStatsWaves; w++) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float lo = s_wbox[w][i], hi = s_wbox[w][3 + i];
            un.box.mn[i] = lo < un.box.mn[i] ? lo : un.box.mn[i];
            un.box.mx[i] = hi > un.box.mx[i] ? hi : un.box.mx[i];
        }
        un.any_nan = un.any_nan || s_wbox[w][6] != 0.0f;
        any_active = any_active || s_wbox[w][7] != 0.0f;
    }

    // ---- the lights, a chunk of kStatsThreads at a time (skipped by a workgroup without an active cluster)
    uint32_t count = 0; // lane s: cluster s's lights, uncapped
    const uint32_t nl = any_active ? p.info.global_light_count : 0u;
    for (uint32_t l0 = 0, par = 0; l0 < nl; l0 += kStatsThreads, par ^= 1u) {
        if (threadIdx.x == 0) s_ncand[par ^ 1u] = 0u, s_nonpoint[par ^ 1u] = 0u; // the next chunk's (read before the last barrier)
        const uint32_t i = l0 + threadIdx.x;
        bool point = false, cand = false;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < nl) {
            const OrbitLightData &l = p.lights[i];
            point = l.light_type == ORBIT_LIGHT_TYPE_POINT;
            v = light_to_view(p.info, l); // light_culling.comp:103, :111
            cand = point && light_passes(un, true, v);
        }
        const uint64_t np = __ballot(i < nl && !point), m = __ballot(cand);
        uint32_t at = 0;
        if (lane == 0) {
            if (np != 0ull) atomicAdd(&s_nonpoint[par], (uint32_t)__popcll(np));
            if (m != 0ull) at = atomicAdd(&s_ncand[par], (uint32_t)__popcll(m));
        }
        at = (uint32_t)__shfl((int)at, 0, 64);
        if (cand) s_cand[at + lane_prefix(m)] = v;
        __syncthreads();
        const uint32_t nc = s_ncand[par];
        if (active_mask != 0ull) { // wave-uniform
            for (uint32_t b0 = 0; b0 < nc; b0 += 64u) {
                const uint32_t k = b0 + lane;
                const float4 cl = s_cand[k < nc ? k : 0u];
                uint64_t todo = active_mask;
                while (todo) {
                    const uint32_t s = (uint32_t)__builtin_ctzll(todo);
                    todo &= todo - 1ull;
                    Aabb3 a;
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        a.mn[j] = __uint_as_float(__builtin_amdgcn_readlane((int)__float_as_uint(box.mn[j]), (int)s));
                        a.mx[j] = __uint_as_float(__builtin_amdgcn_readlane((int)__float_as_uint(box.mx[j]), (int)s));
                    }
                    const uint32_t hits = (uint32_t)__popcll(__ballot(k < nc && sphere_hits(a, cl))); // :108-119
                    count += lane == s ? hits : 0u;
                }
            }
            count += active ? s_nonpoint[par] : 0u; // :116-118
        }
        __syncthreads(); // s_cand and this chunk's words are rewritten two chunks on
    }

    // ---- the tile's counters, summed in LDS, then one atomic per counter and workgroup
    if (lane == 0 && outside != 0u) atomicAdd(&s_cnt[kOutside], (unsigned long long)outside);
    if (active) {
        const uint32_t capped = min(count, ORBIT_MAX_LIGHTS_PER_CLUSTER); // :135
        const uint32_t c = light_class(count);
        atomicAdd(&s_cnt[kActive], 1ull);
        atomicAdd(&s_cnt[kRefs], (unsigned long long)count);
        atomicAdd(&s_cnt[kIndices], (unsigned long long)capped);
        atomicMax(&s_cnt[kMaxLights], (unsigned long long)count);
        atomicAdd(&s_cnt[kSampleRefs], (unsigned long long)n_samples * capped);
        atomicAdd(&s_cnt[kClusterClass + c], 1ull);
        atomicAdd(&s_cnt[kSampleClass + c], (unsigned long long)n_samples);
    }
    __syncthreads();
    if (threadIdx.x < kWords) {
        const unsigned long long v = s_cnt[threadIdx.x];
        if (v != 0ull) {
            if (threadIdx.x == kMaxLights) atomicMax(p.stats + threadIdx.x, v);
            else atomicAdd(p.stats + threadIdx.x, v);
        }
    }
}

} // namespace

hipError_t launch_cluster_stats(const ClusterStatsParams &p, hipStream_t s) {
    hipError_t e = hipMemsetAsync(p.stats, 0, sizeof(OrbitClusterStats), s);
    if (e != hipSuccess) return e;
    const uint32_t bx = (p.pc.cluster_count[0] + kStatsSide - 1u) / kStatsSide;
    const uint32_t by = (p.pc.cluster_count[1] + kStatsSide - 1u) / kStatsSide;
    const uint32_t blocks = bx * by != 0u ? bx * by : 1u; // (block 0 writes `samples` for an empty grid too)
    hipLaunchKernelGGL(cluster_stats_kernel, dim3(blocks), dim3(kStatsThreads), 0, s, p);
    return hipGetLastError();
}

} // namespace orbit
