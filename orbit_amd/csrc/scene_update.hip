// scene_update.hip — orbit_scene_update_entities (include/orbit_abi_ext.h): the EntityData rows of
// SceneData::update_scene (src/scene.rs:75-82, 404-492) computed on the device from the entities' 40-B transforms.
//
// The pin is the host mirror, bit for bit: math::mat4_from_quat and mat4_from_scale_rotation_translation
// (orbit_host.cpp), Mat4::inverse in its scalar cofactor form, transpose, and identity outside the normal matrix's upper
// 3x3 (scene.cpp EntityData::entity_gpu_data).  Every expression below is the host's, written in the same association;
// terms that vanish for an affine matrix (m[3], m[7], m[11] = 0, m[15] = 1) are kept, because dropping them changes
// signed zeros and 0 * inf.  The translation unit is built with -ffp-contract=off -fno-fast-math and correctly rounded
// division (Makefile), and hipcc keeps f32 denormals: the same IEEE binary32 operations as the host's SSE code.
//
// Shape: bandwidth-bound, one lane per entity, 256 lanes per workgroup.  The workgroup's contiguous slab of transforms
// (256 x 40 B = 10 KiB) is staged through LDS with dwordx4 loads (a 40-B stride gives a lane no aligned 16-B load of its
// own); each lane then computes its 128-B row and puts it back into LDS, and the rows leave in full 128-B lines — eight
// lanes per row, one dwordx4 each, so one store instruction of a wave writes eight whole lines (1 KiB contiguous in the
// dense form).  The sparse form reads a lane's instance index beside its transform and guards the row's store.
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

// kAligned16: `transforms` is 16-B aligned (every workgroup's slab then is: 256 x 40 B = 640 x 16 B).
// kSparse: row i goes to entity_data[indices[i]] (guarded by `capacity`), else to entity_data[i].
template <bool kAligned16, bool kSparse>
__global__ __launch_bounds__(kUpdateThreads) void scene_update_kernel(const float *__restrict__ transforms,
                                                                      const uint32_t *__restrict__ indices,
                                                                      uint32_t count, float4 *__restrict__ out,
                                                                      uint32_t capacity, int32_t *status) {
    // 32 KiB: first the workgroup's slab of transforms (10 KiB), then its 256 rows (slot k of row r at k ^ (r & 7))
    __shared__ float4 lds[kUpdateThreads * kRowVecs];
    const uint32_t tid = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * kUpdateThreads;
    const uint32_t n = count - first < kUpdateThreads ? (uint32_t)(count - first) : kUpdateThreads;
    const float *src = transforms + first * kTransformFloats;
    float *slab = (float *)lds;
    uint32_t dst = (uint32_t)(first + tid); // the row this lane computes goes to entity_data[dst]
    if (kSparse) dst = tid < n ? indices[first + tid] : 0xFFFFFFFFu;
    // every load of the slab is issued before the first LDS write waits for one
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
    if (kSparse && tid < n && dst >= capacity) latch_status(status, ORBIT_E_RANGE);
    __syncthreads();
    float t[kTransformFloats];
    const float2 *own = (const float2 *)(slab + tid * kTransformFloats); // 8-B aligned: ds_read_b64, no bank conflict
    for (uint32_t k = 0; k < kTransformFloats / 2; k++) {
        const float2 v = own[k];
        t[2 * k] = v.x, t[2 * k + 1] = v.y;
    }
    __syncthreads(); // the slab is overwritten by the rows below
    float row[32];
    entity_rows(t, row, row + 16);
    for (uint32_t k = 0; k < kRowVecs; k++)
        lds[tid * kRowVecs + (k ^ (tid & 7u))] = make_float4(row[4 * k], row[4 * k + 1], row[4 * k + 2], row[4 * k + 3]);
    __syncthreads();
    // a wave stores its own 64 rows: store j, lane l -> row 8j + l/8 of the wave, 16-B slot l % 8
    const uint32_t lane = tid & 63u, wave_row0 = tid & ~63u, slot = lane & 7u;
    for (uint32_t j = 0; j < kRowVecs; j++) {
        const uint32_t local = j * 8u + lane / 8u;
        const uint32_t r = wave_row0 + local;
        const uint32_t d = kSparse ? (uint32_t)__shfl(dst, (int)local) : dst - tid + r;
        const float4 v = lds[r * kRowVecs + (slot ^ (r & 7u))];
        if (r < n && (!kSparse || d < capacity)) out[(uint64_t)d * kRowVecs + slot] = v;
    }
}

template <bool kSparse>
void launch_variant(bool aligned16, dim3 grid, const float *transforms, const uint32_t *indices, uint32_t count,
                    float4 *out, uint32_t capacity, int32_t *status, hipStream_t s) {
    if (aligned16)
        hipLaunchKernelGGL((scene_update_kernel<true, kSparse>), grid, dim3(kUpdateThreads), 0, s, transforms, indices,
                           count, out, capacity, status);
    else
        hipLaunchKernelGGL((scene_update_kernel<false, kSparse>), grid, dim3(kUpdateThreads), 0, s, transforms, indices,
                           count, out, capacity, status);
}

} // namespace

hipError_t launch_scene_update_entities(const OrbitEntityTransform *transforms, const uint32_t *instance_indices,
                                        uint32_t count, OrbitEntityData *entity_data, uint32_t entity_capacity,
                                        int32_t *status, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const dim3 grid((uint32_t)(((uint64_t)count + kUpdateThreads - 1) / kUpdateThreads));
    const bool aligned16 = ((uintptr_t)transforms & 15u) == 0;
    const float *t = (const float *)transforms;
    float4 *out = (float4 *)entity_data;
    if (instance_indices)
        launch_variant<true>(aligned16, grid, t, instance_indices, count, out, entity_capacity, status, s);
    else
        launch_variant<false>(aligned16, grid, t, nullptr, count, out, entity_capacity, status, s);
    return hipGetLastError();
}

} // namespace orbit
