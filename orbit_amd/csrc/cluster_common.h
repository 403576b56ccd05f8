// cluster_common.h — the light-cluster arithmetic shared by the cluster chain (light_cluster.hip) and its statistics
// (cluster_stats.hip): the mark's sample addressing, the cluster volume of light_culling.comp and its light test.
// One definition, so that the statistics classify with the chain's own operations.
#pragma once
#include "kernels.h"

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

} // namespace

} // namespace orbit
