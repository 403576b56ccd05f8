// cluster_common.h — the light-cluster arithmetic shared by the cluster chain (light_cluster.hip) and its statistics
// (cluster_stats.hip): the mark's sample addressing, values and per-slice bounds, the cluster volume of light_culling.comp,
// its light test and the union of boxes that the conservative filters test against.
// One definition, so that the statistics classify with the chain's own operations.
#pragma once
#include "kernels.h"
#include "scan.h"

namespace orbit {

namespace {

// sample `it` of tile `tile` (mark_active.comp:40): its address in the depth buffer, or none.  cx, cy: the grid's tiles.
__device__ __forceinline__ bool mark_sample(const OrbitMarkActivePush &pc, uint32_t cx, uint32_t cy, uint32_t tile, uint32_t it,
                                            size_t &index) {
    const uint32_t ts = pc.tile_size_px, sc = pc.depth_buffer_sample_count;
    const uint32_t W = pc.screen_size[0], H = pc.screen_size[1];
    const uint32_t items = ts * ts * sc;
    // (divisors the compiler cannot see through: their reciprocals are not hoisted into every wave's prologue)
    uint32_t dcx = cx, dsc = sc, dts = ts;
    asm volatile("" : "+s"(dcx), "+s"(dsc), "+s"(dts));
    const uint32_t tx = tile % dcx, ty = tile / dcx;
    const uint32_t pix = it / dsc, smp = it % dsc;
    const uint32_t px = tx * ts + pix % dts, py = ty * ts + pix / dts;
    index = ((size_t)py * W + px) * sc + smp;
    return tile < cx * cy && it < items && px < W && py < H;
}

// What the mark keeps of one depth sample (mark_active.comp:28-34): its z slice, the slice's bit of the tile's mask and
// the two words of its cluster's depth bounds, both taken as maxima.  A lane without a sample (!valid): no slice, no bit.
struct MarkValues {
    uint32_t slice, bit, bmin, bmax;
    bool valid;
};

__device__ __forceinline__ MarkValues mark_values(const OrbitMarkActivePush &pc, bool valid, float d) {
    MarkValues v = {0xFFFFFFFFu, 0u, 0u, 0u, valid};
    if (valid) {
        const float linear_z = pc.z_near / d;                       // :28
        // cluster_common.glsl:18-20 as compiled (mark_active.comp.spv): one fused operation — through the
        // hardware log2 where that provably gives the canonical slice (orbit_device.h depth_slice)
        v.slice = depth_slice(linear_z, pc.z_scale, pc.z_bias);
        v.bit = shl1(v.slice);                                      // :30
        const float inv = 1.0f - d;                                 // :33
        // the sign / payload of a NaN produced by arithmetic is implementation-defined: canonical quiet NaN
        v.bmin = inv != inv ? 0x7fc00000u : __float_as_uint(inv);
        v.bmax = __float_as_uint(d);                                // :34
    }
    return v;
}

// The bounds of the slices in `todo` (a wave-uniform mask of slices that some lane's sample lies in) over the wave's 64
// samples: lane s accumulates slice s's.  per_slice(s, mine) runs once per slice with all lanes active (the statistics
// count the slice's samples there).
template <class PerSlice>
__device__ __forceinline__ void mark_slice_bounds(uint32_t todo, const MarkValues &v, uint32_t lane, uint32_t &acc_min,
                                                  uint32_t &acc_max, PerSlice per_slice) {
    while (todo) {
        const uint32_t s = (uint32_t)__builtin_ctz(todo);
        todo &= todo - 1u;
        const bool mine = v.valid && v.slice == s;
        per_slice(s, mine);
        const uint32_t m1 = wave_reduce_max(mine ? v.bmin : 0u);
        const uint32_t m2 = wave_reduce_max(mine ? v.bmax : 0u);
        if (lane == s) {
            acc_min = max(acc_min, m1);
            acc_max = max(acc_max, m2);
        }
    }
}

// view-space light of light_culling.comp: world_to_view x position (:111) and sphere.w * sphere.w (:103)
__device__ __forceinline__ float4 light_to_view(const OrbitClusterCullInfo &info, const OrbitLightData &l) {
    const float *m = info.world_to_view_matrix;
    const float x = l.position[0], y = l.position[1], z = l.position[2];
    float4 v;
    v.x = ((m[0] * x + m[4] * y) + m[8] * z) + m[12] * 1.0f; // light_culling.comp:111
    v.y = ((m[1] * x + m[5] * y) + m[9] * z) + m[13] * 1.0f;
    v.z = ((m[2] * x + m[6] * y) + m[10] * z) + m[14] * 1.0f;
    v.w = l.outer_radius * l.outer_radius;                     // sphere.w * sphere.w, :103
    return v;
}

struct Aabb3 {
    float mn[3], mx[3];
};

// screen_to_view, light_culling.comp:34-48
__device__ __forceinline__ void screen_to_view(const OrbitClusterCullInfo &in, float sx, float sy, float out[3]) {
    const float tx = sx / (float)in.screen_size[0], ty = sy / (float)in.screen_size[1];
    const float c0 = tx * 2.0f - 1.0f, c1 = (1.0f - ty) * 2.0f - 1.0f, c2 = 1.0f, c3 = 1.0f;
    const float *m = in.screen_to_view_matrix;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = ((m[0 + r] * c0 + m[4 + r] * c1) + m[8 + r] * c2) + m[12 + r] * c3;
    out[0] = v[0] / v[3];
    out[1] = v[1] / v[3];
    out[2] = v[2] / v[3];
}

// line_intersection_to_z_plane with a = eye = 0, light_culling.comp:50-60
__device__ __forceinline__ void line_z(const float b[3], float zd, float out[3]) {
    const float ab0 = b[0] - 0.0f, ab1 = b[1] - 0.0f, ab2 = b[2] - 0.0f;
    const float dna = (0.0f * 0.0f + 0.0f * 0.0f) + -1.0f * 0.0f;
    const float dnab = (0.0f * ab0 + 0.0f * ab1) + -1.0f * ab2;
    const float t = (zd - dna) / dnab;
    out[0] = 0.0f + t * ab0;
    out[1] = 0.0f + t * ab1;
    out[2] = 0.0f + t * ab2;
}

// compute_cluster_volume, light_culling.comp:62-90, of the cluster with linear index `cluster_index`; its depth bounds are
// bounds_of() (called where the shader reads them, :72-73: the chain's code objects keep that order of their loads)
template <class BoundsOf>
__device__ __forceinline__ Aabb3 cluster_aabb_with(const OrbitClusterCullInfo &in, uint32_t cluster_index, BoundsOf bounds_of) {
    const uint32_t cx = in.cluster_count[0], cy = in.cluster_count[1];
    uint32_t idx = cluster_index;
    const uint32_t z = idx / (cx * cy);
    idx -= z * cx * cy;
    const uint32_t y = idx / cx;
    idx -= y * cx;
    const uint32_t x = idx;
    const float minx = (float)(x * in.tile_size_px), miny = (float)(y * in.tile_size_px);
    const float maxx = gmin(minx + (float)in.tile_size_px, (float)in.screen_size[0]);
    const float maxy = gmin(miny + (float)in.tile_size_px, (float)in.screen_size[1]);
    float minv[3], maxv[3];
    screen_to_view(in, minx, miny, minv);
    screen_to_view(in, maxx, maxy, maxv);
    const OrbitClusterDepthBounds db = bounds_of();
    const float min_depth = 1.0f - __uint_as_float(db.min_depth); // :72
    const float max_depth = __uint_as_float(db.max_depth);        // :73
    const float cnear = in.z_near / max_depth, cfar = in.z_near / min_depth;
    float q[4][3];
    line_z(minv, cnear, q[0]);
    line_z(minv, cfar, q[1]);
    line_z(maxv, cnear, q[2]);
    line_z(maxv, cfar, q[3]);
    Aabb3 a;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        a.mn[i] = gmin(gmin(q[0][i], q[1][i]), gmin(q[2][i], q[3][i]));
        a.mx[i] = gmax(gmax(q[0][i], q[1][i]), gmax(q[2][i], q[3][i]));
    }
    return a;
}

// ... with the bounds as a value
__device__ __forceinline__ Aabb3 cluster_aabb(const OrbitClusterCullInfo &in, uint32_t cluster_index,
                                              const OrbitClusterDepthBounds db) {
    return cluster_aabb_with(in, cluster_index, [&] { return db; });
}

// aabb_sphere_test, light_culling.comp:92-104 (l.w already holds r*r)
__device__ __forceinline__ bool sphere_hits(const Aabb3 &a, const float4 l) {
    // as compiled (light_culling.comp.spv): sqr_dist = fma(d, d, sqr_dist) per term
    float sq = 0.0f;
    if (l.x < a.mn[0]) sq = __builtin_fmaf(a.mn[0] - l.x, a.mn[0] - l.x, sq);
    if (l.x > a.mx[0]) sq = __builtin_fmaf(l.x - a.mx[0], l.x - a.mx[0], sq);
    if (l.y < a.mn[1]) sq = __builtin_fmaf(a.mn[1] - l.y, a.mn[1] - l.y, sq);
    if (l.y > a.mx[1]) sq = __builtin_fmaf(l.y - a.mx[1], l.y - a.mx[1], sq);
    if (l.z < a.mn[2]) sq = __builtin_fmaf(a.mn[2] - l.z, a.mn[2] - l.z, sq);
    if (l.z > a.mx[2]) sq = __builtin_fmaf(l.z - a.mx[2], l.z - a.mx[2], sq);
    return sq <= l.w;
}

// The union of cluster boxes that a conservative filter tests the lights against.  A union contains every member box,
// and aabb_sphere_test is monotone in the box (each clamp distance, each square and each partial sum can only shrink
// when the box grows, also in floating point), so no light that hits a member box is ever filtered out.  A union over
// boxes that contain a NaN does not filter at all (any_nan: light_passes), so what the selects below make of a NaN
// operand does not matter.
struct BoxUnion {
    Aabb3 box;
    bool any_nan;
};

// an absent cluster: the empty box, neutral in the union
__device__ __forceinline__ void box_empty(float lo[3], float hi[3]) {
    const float inf = __uint_as_float(0x7f800000u);
#pragma unroll
    for (int i = 0; i < 3; i++) lo[i] = inf, hi[i] = -inf;
}

__device__ __forceinline__ BoxUnion union_empty() {
    BoxUnion u;
    u.any_nan = false;
    box_empty(u.box.mn, u.box.mx);
    return u;
}

__device__ __forceinline__ void union_add(BoxUnion &u, const float lo[3], const float hi[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        u.any_nan = u.any_nan || lo[i] != lo[i] || hi[i] != hi[i];
        u.box.mn[i] = lo[i] < u.box.mn[i] ? lo[i] : u.box.mn[i];
        u.box.mx[i] = hi[i] > u.box.mx[i] ? hi[i] : u.box.mx[i];
    }
}

// Level 1: the union of the boxes of the wave's first LANES lanes (a power of two) by a butterfly, left in every one of
// them; returns whether any of those boxes holds a NaN.
template <int LANES>
__device__ __forceinline__ bool lanes_union(float lo[3], float hi[3]) {
    bool nan = false;
#pragma unroll
    for (int i = 0; i < 3; i++) nan = nan || lo[i] != lo[i] || hi[i] != hi[i];
    const bool any_nan = (__ballot(nan) & (LANES == 64 ? ~0ull : (1ull << (LANES & 63)) - 1ull)) != 0ull;
#pragma unroll
    for (int d = LANES / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float ol = __shfl_xor(lo[i], d, 64), oh = __shfl_xor(hi[i], d, 64);
            lo[i] = ol < lo[i] ? ol : lo[i];
            hi[i] = oh > hi[i] ? oh : hi[i];
        }
    }
    return any_nan;
}

// Level 2: a table in LDS with a row of 8 words per wave — its union's lo (0-2) and hi (3-5), its any-NaN flag (6); word
// 7 is the table owner's.  union_row_store is one lane's; union_rows, behind a barrier, is the union of the rows.
__device__ __forceinline__ void union_row_store(float row[8], const float lo[3], const float hi[3], bool any_nan) {
#pragma unroll
    for (int i = 0; i < 3; i++) row[i] = lo[i], row[3 + i] = hi[i];
    row[6] = any_nan ? 1.0f : 0.0f;
}

template <int ROWS>
__device__ __forceinline__ BoxUnion union_rows(const float (*rows)[8]) {
    BoxUnion un = union_empty();
#pragma unroll
    for (int w = 0; w < ROWS; w++) {
        union_add(un, &rows[w][0], &rows[w][3]);
        un.any_nan = un.any_nan || rows[w][6] != 0.0f;
    }
    return un;
}

// The filters' rule: a light that is no point light is in every cluster (light_culling.comp:116-118), a union that
// holds a NaN filters nothing, every other light is tested against the union's box.
__device__ __forceinline__ bool light_passes(const BoxUnion &un, bool point, const float4 l) {
    return !point || un.any_nan || sphere_hits(un.box, l);
}

} // namespace

} // namespace orbit
