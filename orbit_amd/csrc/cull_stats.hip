// cull_stats.hip — orbit_cull_stats for gfx950: what orbit_entity_cull + orbit_meshlet_cull would do with every
// entity-draw and every meshlet, counted by the first test that rejected it (include/orbit_abi_ext.h OrbitCullStats).
//
// Nothing here restates a predicate.  The entity stage is entity_eval_one (entity_common.h) with its verdict kept; the
// meshlet stage runs the evaluation's own tile slab, row loads, geometry mask, alpha bits and should-draw rule
// (meshlet_common.h), and the pass-2 HiZ test of orbit_device.h on the survivors of planes + cone, with the sphere, radius
// and scale the candidate flush hands it.  The one thing the stats add is the split of the geometry mask: the plane test
// alone, once more on the same view-space sphere — a lane outside it is frustum-culled, a lane inside it that the mask
// rejects is cone-culled (the cone is the mask's only other test).
//
// Shape: a persistent grid of 256-thread workgroups strides over chunks of 256 entity-draws.  A chunk's entity-draws are
// classified one per thread; their records (ceil(meshlets / 32) each, worked out here, never read from a dispatch buffer)
// are prefix-summed in LDS, and the four waves take the chunk's wave tiles of 16 records in turn (a scene of few chunks
// gives each chunk gridDim.y workgroups: all of them classify its entity-draws, the first one counts them, and they
// share its tiles — the meshlet stage is then spread over the chip instead of queued behind a few waves): the model
// columns are multiplied into the tile slab once, the eight rows of 64 meshlets are loaded at once (two dwordx4 per lane
// and row),
// and every class of a row is a ballot whose popcount is added to a per-wave counter.  At the end the workgroup adds its
// four waves' counters in LDS and issues one 64-bit atomic add per non-zero counter.  Sums do not depend on the order:
// the result is deterministic.  Nothing but the counters is written.
#include "entity_common.h"
#include "meshlet_common.h"

namespace orbit {

namespace {

// counter words of OrbitCullStats (include/orbit_abi_ext.h) the kernel accumulates
enum : uint32_t {
    kStEntities = 0, kStEntSkipped, kStEntFrustum, kStEntOcclusion, kStEntEarly, kStEntDrawn, kStRecords,
    kStLod = 8,
    kStMeshlets = 16, kStMlSkipped, kStMlFrustum, kStMlCone, kStMlOcclusion, kStMlAlpha, kStMlEarly, kStMlDrawn,
    kStWords = 24
};
static_assert(kStLod + ORBIT_MAX_MESH_LODS <= kStMeshlets, "lod_drawn[8] @64");
static_assert(kStMlDrawn * 8 == 184 && kStWords * 8 == 192, "OrbitCullStats layout");

constexpr int kStatsWaves = kEntityBlock / 64;
constexpr uint32_t kStatsBlocksPerCu = 4;
constexpr uint32_t kStatsMaxSplit = 16; // workgroups that share one chunk's tiles (gridDim.y)

__device__ __forceinline__ uint32_t popc(uint64_t m) { return (uint32_t)__popcll(m); }

// One row of a wave tile (record 2 r + lane / 32, meshlet lane % 32): every active lane lands in exactly one class.
// (occlusion_pass == PASS; `prev` is the lane's last-frame visibility word as rows_load fetched it)
template <int PASS>
__device__ __forceinline__ void classify_row(const MeshletCullParams &p, const WaveTileLds &L, const PlaneLds &P,
                                             const AlphaLds *A, int lane, int r, const uint4 &a, const uint4 &b,
                                             uint32_t prev, uint32_t *c) {
    const uint32_t half = lane >> 5, ml = lane & 31, rid = 2 * r + half;
    const uint64_t act = ballot(ml < L.r[rid].rec.z); // :111
    if (act == 0ull) return;
    const bool meshlet_occ = p.ci.meshlet_visibility_buffer != ORBIT_NONE;
    const bool occ2 = PASS == 2 && meshlet_occ;
    const uint32_t abits = lane_alpha_bits<false>(p, L, A, rid, ml, b.w);
    const bool visible_in_buffer = !(PASS != 0 && meshlet_occ) || ((prev >> ml) & 1u) != 0u; // :129-134
    Sphere s;
    const uint64_t geo = eval_geometry_mask<-1>(p, L, P, rid, a, b, s, row_is_affine(L, r)); // :139-158
    const uint64_t inside = plane_test_lds(P, p.ci.cull_plane_count, s);                      // :139-146 alone
    const uint64_t skipped = (PASS == 1 && meshlet_occ) ? act & ~ballot(visible_in_buffer) : 0ull; // :137
    const uint64_t live = act & ~skipped;
    uint64_t vis = live & geo;
    uint64_t occluded = 0ull;
    if (occ2) { // :161-205, as cand_flush runs it: model-space radius and the record's scale
        bool ov = true;
        if (lane_of(vis)) {
            Sphere o = s;
            ov = occlusion_test(p.ci, o, __uint_as_float(a.w), L.r[rid].scale, p.pyr);
        }
        occluded = vis & ~ballot(ov);
        vis &= ~occluded;
    }
    const uint64_t drawn = vis & ballot(should_draw_of(true, abits, visible_in_buffer, occ2)); // :207-213
    // :210-213 overrides :207 for alpha modes outside noskip_alphamode: such a lane is left out only for being visible
    // last frame, whatever its alpha flag says
    const uint64_t early = occ2 ? vis & ~drawn & ~ballot((abits & 2u) != 0u) : 0ull;
    c[kStMeshlets] += popc(act);
    c[kStMlSkipped] += popc(skipped);
    c[kStMlFrustum] += popc(live & ~inside);
    c[kStMlCone] += popc(live & inside & ~geo);
    c[kStMlOcclusion] += popc(occluded);
    c[kStMlAlpha] += popc(vis & ~drawn & ~early);
    c[kStMlEarly] += popc(early);
    c[kStMlDrawn] += popc(drawn);
}

template <int PASS>
__global__ __launch_bounds__(kEntityBlock) void cull_stats_kernel(const CullStatsParams p) {
    __shared__ PlaneLds planes;
    __shared__ AlphaLds alpha_tab;
    __shared__ uint32_t smem[kStatsWaves + 1];
    __shared__ uint32_t s_off[kEntityBlock];
    __shared__ OrbitMeshletDispatch s_proto[kEntityBlock];
    __shared__ WaveTileLds tiles[kStatsWaves];
    __shared__ unsigned long long s_red[kStatsWaves][kStWords];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    planes_to_lds(p.m, planes);
    const AlphaLds *alpha = alpha_table_fill(p.m, alpha_tab) ? &alpha_tab : nullptr;
    __syncthreads();
    WaveTileLds &L = tiles[wave];

    // per-wave counts (wave-uniform; records: wave 0 adds the chunk totals)
    uint32_t c[kStWords];
#pragma unroll
    for (uint32_t i = 0; i < kStWords; i++) c[i] = 0u;
    unsigned long long records = 0ull;

    const uint32_t draw_count = *reinterpret_cast<const uint32_t *>(p.e.entity_draw_buffer);
    const uint32_t draw_end = min(draw_count, p.e.draw_limit); // as entity_cull's launches bound it (:106)
    const bool counts_entities = blockIdx.y == 0u;
    for (uint32_t eb = blockIdx.x; eb < p.e.ne_chunks; eb += gridDim.x) {
        const uint32_t g = p.e.draw_first + eb * kEntityBlock + threadIdx.x;
        const bool active = g < draw_end;
        bool visible;
        EntityVerdict v;
        const OrbitMeshletDispatch pr = entity_eval_one(p.e, g, active, visible, &v);
        const uint64_t drawn = ballot(v.cls == kEntDrawn);
        if (counts_entities) {
            c[kStEntities] += popc(ballot(active));
            c[kStEntSkipped] += popc(ballot(v.cls == kEntSkipped));
            c[kStEntFrustum] += popc(ballot(v.cls == kEntFrustum));
            c[kStEntOcclusion] += popc(ballot(v.cls == kEntOcclusion));
            c[kStEntEarly] += popc(ballot(v.cls == kEntEarly));
            c[kStEntDrawn] += popc(drawn);
        }
        if (counts_entities && drawn != 0ull) {
#pragma unroll
            for (uint32_t l = 0; l < ORBIT_MAX_MESH_LODS; l++) c[kStLod + l] += popc(drawn & ballot(v.lod == l));
        }

        // the chunk's records (:210-223 with S = 32), owner found by bisection as entity_expand_records does
        const uint32_t n = (pr.meshlet_count + 31u) >> 5;
        uint32_t total;
        s_off[threadIdx.x] = block_exclusive_scan<kStatsWaves>(n, smem, &total);
        s_proto[threadIdx.x] = pr;
        total = uniform(total);
        if (counts_entities && wave == 0) records += total;
        __syncthreads();
        const uint32_t ntiles = (total + kTileRecords - 1u) / kTileRecords;
        for (uint32_t t = blockIdx.y * kStatsWaves + (uint32_t)wave; t < ntiles; t += kStatsWaves * gridDim.y) {
            const uint32_t r = t * kTileRecords + (uint32_t)(lane >> 2);
            uint4 rec = make_uint4(0u, 0u, 0u, 0u); // meshlet_count 0: no record (zero page, no lane active)
            if (r < total) {
                uint32_t lo = 0u, hi = kEntityBlock;
#pragma unroll
                for (int step = 0; step < 8; step++) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_off[mid] <= r) lo = mid; else hi = mid;
                }
                const OrbitMeshletDispatch o = entity_record(s_proto[lo], r - s_off[lo], 5u);
                rec = make_uint4(o.entity_index, o.meshlet_offset, o.meshlet_count, o.visibility_offset);
            }
            const float4 mc = setup_load_mat(p.m, rec, lane);
            setup_write(p.m, L, rec, mc, lane);
            RowRegs<kTileRows> rows;
            rows_load<PASS, 0, kTileRows>(p.m, L, lane, rows);
#pragma unroll
            for (int k = 0; k < (int)kTileRows; k++)
                classify_row<PASS>(p.m, L, planes, alpha, lane, k, rows.a[k], rows.b[k], rows.prev[k], c);
        }
        __syncthreads(); // s_off / s_proto are the next chunk's
    }

    if (lane == 0) {
#pragma unroll
        for (uint32_t i = 0; i < kStWords; i++) s_red[wave][i] = c[i];
        s_red[wave][kStRecords] = records;
    }
    __syncthreads();
    if (threadIdx.x < kStWords) {
        unsigned long long sum = 0ull;
#pragma unroll
        for (int w = 0; w < kStatsWaves; w++) sum += s_red[w][threadIdx.x];
        if (sum != 0ull)
            __hip_atomic_fetch_add(p.stats + threadIdx.x, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

} // namespace

hipError_t launch_cull_stats(const CullStatsParams &p, uint32_t num_cus, hipStream_t s) {
#if !ORBIT_CONTRACT
    if (p.e.arith != 0u) return launch_cull_stats_contracted(p, num_cus, s); // OrbitCaps.arith_profile
#endif
    hipError_t e = hipMemsetAsync(p.stats, 0, sizeof(OrbitCullStats), s);
    if (e != hipSuccess || p.e.ne_chunks == 0u) return e;
    const uint32_t gx = max(min(p.e.ne_chunks, num_cus * kStatsBlocksPerCu), 1u);
    const dim3 grid(gx, max(min(num_cus * kStatsBlocksPerCu / gx, kStatsMaxSplit), 1u));
    switch (p.e.ci.occlusion_pass) {
    case 0: hipLaunchKernelGGL(cull_stats_kernel<0>, grid, dim3(kEntityBlock), 0, s, p); break;
    case 1: hipLaunchKernelGGL(cull_stats_kernel<1>, grid, dim3(kEntityBlock), 0, s, p); break;
    default: hipLaunchKernelGGL(cull_stats_kernel<2>, grid, dim3(kEntityBlock), 0, s, p); break;
    }
    return hipGetLastError();
}

} // namespace orbit
