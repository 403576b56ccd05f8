// scene_rows.h — what the two scene-update units (scene_update.hip: orbit_scene_update_entities; scene_full.hip:
// orbit_scene_update) share, so that the EntityData rows of both are the same instructions: the row arithmetic, the
// staging of a workgroup's slab of transforms through LDS, and the swizzle of the rows in LDS.
#pragma once
#include "kernels.h"

namespace orbit {
namespace {

constexpr uint32_t kUpdateThreads = 256;
constexpr uint32_t kTransformFloats = 10; // OrbitEntityTransform
constexpr uint32_t kRowVecs = 8;          // OrbitEntityData: 128 B = 8 x float4

// EntityData::entity_gpu_data of one transform: model (16 floats) and normal matrix (16 floats), column-major.
__device__ __forceinline__ void entity_rows(const float *t, float model[16], float normal[16]) {
    const float px = t[0], py = t[1], pz = t[2];
    const float qx = t[3], qy = t[4], qz = t[5], qw = t[6];
    const float sx = t[7], sy = t[8], sz = t[9];
    // mat4_from_quat (glam quat_to_axes)
    const float x2 = qx + qx, y2 = qy + qy, z2 = qz + qz;
    const float xx = qx * x2, xy = qx * y2, xz = qx * z2, yy = qy * y2, yz = qy * z2, zz = qz * z2;
    const float wx = qw * x2, wy = qw * y2, wz = qw * z2;
    // mat4_from_scale_rotation_translation: columns 0..2 scaled, translation in column 3, identity's zeros in row 3
    float m[16];
    m[0] = (1.0f - (yy + zz)) * sx, m[1] = (xy + wz) * sx, m[2] = (xz - wy) * sx, m[3] = 0.0f;
    m[4] = (xy - wz) * sy, m[5] = (1.0f - (xx + zz)) * sy, m[6] = (yz + wx) * sy, m[7] = 0.0f;
    m[8] = (xz + wy) * sz, m[9] = (yz - wx) * sz, m[10] = (1.0f - (xx + yy)) * sz, m[11] = 0.0f;
    m[12] = px, m[13] = py, m[14] = pz, m[15] = 1.0f;
    // Mat4::inverse, cofactor form: the cofactors the upper 3x3 of the transpose and the determinant need
    float inv[16];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] +
             m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] -
             m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] +
             m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] -
              m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] -
             m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] +
             m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] -
             m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] +
             m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] -
             m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] +
              m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    const float det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    const float rdet = 1.0f / det;
    for (int k = 0; k < 16; k++) model[k] = m[k];
    // normal column c, row r = inverse()[column r, row c] (transpose); identity outside the upper 3x3
    normal[0] = inv[0] * rdet, normal[1] = inv[4] * rdet, normal[2] = inv[8] * rdet, normal[3] = 0.0f;
    normal[4] = inv[1] * rdet, normal[5] = inv[5] * rdet, normal[6] = inv[9] * rdet, normal[7] = 0.0f;
    normal[8] = inv[2] * rdet, normal[9] = inv[6] * rdet, normal[10] = inv[10] * rdet, normal[11] = 0.0f;
    normal[12] = 0.0f, normal[13] = 0.0f, normal[14] = 0.0f, normal[15] = 1.0f;
}

// The workgroup's slab of `n` <= 256 transforms from `src` into LDS (`lds`: at least 640 float4).  kAligned16: `src` is
// 16-B aligned.  Every load of the slab is issued before the first LDS write waits for one; the caller's barrier follows.
template <bool kAligned16>
__device__ __forceinline__ void load_transform_slab(const float *__restrict__ src, uint32_t n, float4 *lds) {
    const uint32_t tid = threadIdx.x;
    float *slab = (float *)lds;
    if (kAligned16) {
        const uint32_t vecs = n * kTransformFloats / 4; // whole float4 of the slab (<= 640); an odd n leaves 2 floats
        const float4 *src4 = (const float4 *)src;
        const uint32_t q0 = tid, q1 = tid + kUpdateThreads, q2 = tid + 2 * kUpdateThreads;
        float4 v0 = {}, v1 = {}, v2 = {};
        float tail = 0.0f;
        if (q0 < vecs) v0 = src4[q0];
        if (q1 < vecs) v1 = src4[q1];
        if (q2 < vecs) v2 = src4[q2];
        if ((n & 1u) && tid < 2u) tail = src[vecs * 4u + tid];
        if (q0 < vecs) lds[q0] = v0;
        if (q1 < vecs) lds[q1] = v1;
        if (q2 < vecs) lds[q2] = v2;
        if ((n & 1u) && tid < 2u) slab[vecs * 4u + tid] = tail;
    } else {
        float v[kTransformFloats];
#pragma unroll
        for (uint32_t k = 0; k < kTransformFloats; k++) {
            v[k] = 0.0f;
            if (tid + k * kUpdateThreads < n * kTransformFloats) v[k] = src[tid + k * kUpdateThreads];
        }
#pragma unroll
        for (uint32_t k = 0; k < kTransformFloats; k++)
            if (tid + k * kUpdateThreads < n * kTransformFloats) slab[tid + k * kUpdateThreads] = v[k];
    }
}

// This lane's transform out of the slab (behind the barrier that follows load_transform_slab).
__device__ __forceinline__ void read_own_transform(const float4 *lds, float t[kTransformFloats]) {
    const float2 *own = (const float2 *)((const float *)lds + threadIdx.x * kTransformFloats); // 8-B aligned: ds_read_b64, no bank conflict
    for (uint32_t k = 0; k < kTransformFloats / 2; k++) {
        const float2 v = own[k];
        t[2 * k] = v.x, t[2 * k + 1] = v.y;
    }
}

// Row `r` of the workgroup's rows in LDS keeps its 16-B slot k at k ^ (r & 7): eight lanes that write slot k of eight
// consecutive rows, and eight that read the eight slots of one row, hit different banks.
__device__ __forceinline__ void put_row(float4 *lds, uint32_t r, const float row[32]) {
    for (uint32_t k = 0; k < kRowVecs; k++)
        lds[r * kRowVecs + (k ^ (r & 7u))] = make_float4(row[4 * k], row[4 * k + 1], row[4 * k + 2], row[4 * k + 3]);
}
__device__ __forceinline__ float4 get_row_slot(const float4 *lds, uint32_t r, uint32_t slot) {
    return lds[r * kRowVecs + (slot ^ (r & 7u))];
}

} // namespace
} // namespace orbit
