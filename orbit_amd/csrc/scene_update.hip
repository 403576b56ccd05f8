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
#include "scene_rows.h"

namespace orbit {
namespace {

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
    uint32_t dst = (uint32_t)(first + tid); // the row this lane computes goes to entity_data[dst]
    if (kSparse) dst = tid < n ? indices[first + tid] : 0xFFFFFFFFu;
    load_transform_slab<kAligned16>(src, n, lds);
    if (kSparse && tid < n && dst >= capacity) latch_status(status, ORBIT_E_RANGE);
    __syncthreads();
    float t[kTransformFloats];
    read_own_transform(lds, t);
    __syncthreads(); // the slab is overwritten by the rows below
    float row[32];
    entity_rows(t, row, row + 16);
    put_row(lds, tid, row);
    __syncthreads();
    // a wave stores its own 64 rows: store j, lane l -> row 8j + l/8 of the wave, 16-B slot l % 8
    const uint32_t lane = tid & 63u, wave_row0 = tid & ~63u, slot = lane & 7u;
    for (uint32_t j = 0; j < kRowVecs; j++) {
        const uint32_t local = j * 8u + lane / 8u;
        const uint32_t r = wave_row0 + local;
        const uint32_t d = kSparse ? (uint32_t)__shfl(dst, (int)local) : dst - tid + r;
        const float4 v = get_row_slot(lds, r, slot);
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
