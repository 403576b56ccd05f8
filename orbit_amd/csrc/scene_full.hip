// scene_full.hip — orbit_scene_update (include/orbit_abi_ext.h): all of SceneData::update_scene
// (src/scene.rs:404-492) on the device — the EntityData rows, the EntityDrawBuffer, the LightData[] array with its shadow
// indices, the shadow commands' orientations and the entity -> instance / light maps — from one 48-B descriptor and one
// 40-B transform per entity, both in ENTITY order.
//
// The pin is the host mirror (orbit_scene.cpp SceneData::update), byte for byte.  The work is three ordered stream
// compactions over the entity array (has a mesh, has a light, is a directional light that casts shadows); order comes
// from prefix sums, never from atomics.  The EntityData arithmetic is scene_rows.h's, shared with
// orbit_scene_update_entities; the light rows restate EntityData::light_gpu_data in the host's association (the zero
// products of quat_mul_vec3 are kept: they carry signed zeros and 0 * inf).  Built like scene_update.hip:
// -ffp-contract=off, correctly rounded divide and sqrt, f32 denormals kept.
//
// Two launches, no hand-over between workgroups of one launch:
//   scene_count_kernel   one lane per entity reads the descriptor's first 16 B (mesh_index, light_kind, light_flags),
//                        ballots the three predicates and leaves the workgroup's three totals in the context's scratch
//   scene_build_kernel   one lane per entity, 256 per workgroup.  A workgroup's bases are the sums of the totals of the
//                        workgroups before it (the second scan level: every workgroup reduces its own prefix of the
//                        totals array — 3 words per 256 entities, L2-resident — so no workgroup waits for another);
//                        lane ranks are popcounts of the ballots below the lane plus the totals of the waves before.
//                        The mesh-bearing lanes' rows are compacted in LDS and leave as whole 128-B lines, the draws
//                        (12 B) and light rows (64 B) are compacted the same way and leave as contiguous dwords; the
//                        last workgroup, which knows the grand totals, writes the count word and *counts and latches
//                        ORBIT_E_CAPACITY.
#include "scan.h"
#include "scene_rows.h"

namespace orbit {
namespace {

constexpr uint32_t kNone = ORBIT_SCENE_NONE;
constexpr uint32_t kEntityWords = 12; // OrbitSceneEntity
constexpr uint32_t kDrawWords = 3;    // OrbitEntityDraw
constexpr uint32_t kLightWords = 16;  // OrbitLightData
constexpr uint32_t kWaves = kUpdateThreads / 64;

static_assert(sizeof(OrbitSceneEntity) == kEntityWords * 4 && sizeof(OrbitLightData) == kLightWords * 4 &&
                  sizeof(OrbitEntityDraw) == kDrawWords * 4,
              "layouts");

__device__ __forceinline__ bool has_mesh(uint32_t mesh_index) { return mesh_index != kNone; }
__device__ __forceinline__ bool has_light(uint32_t kind) { return kind <= 2u; }
__device__ __forceinline__ bool casts_shadow(uint32_t kind, uint32_t flags) { return kind == 1u && (flags & 1u); }

// The three totals of every workgroup of 256 entities: block_sums[3 b + {0, 1, 2}] = {meshes, lights, shadow casters}.
template <bool kAligned16>
__global__ __launch_bounds__(kUpdateThreads) void scene_count_kernel(const uint32_t *__restrict__ entities,
                                                                     uint32_t count, uint32_t *__restrict__ block_sums) {
    __shared__ uint32_t wave_tot[kWaves][3];
    const uint32_t tid = threadIdx.x;
    const uint64_t e = (uint64_t)blockIdx.x * kUpdateThreads + tid;
    uint32_t mesh = kNone, kind = kNone, flags = 0u;
    if (e < count) {
        if (kAligned16) {
            const uint4 d = ((const uint4 *)entities)[e * 3u];
            mesh = d.x, kind = d.z, flags = d.w;
        } else {
            const uint32_t *d = entities + e * kEntityWords;
            mesh = d[0], kind = d[2], flags = d[3];
        }
    }
    const uint64_t bm = __ballot(has_mesh(mesh)), bl = __ballot(has_light(kind)), bs = __ballot(casts_shadow(kind, flags));
    if ((tid & 63u) == 0u) {
        wave_tot[tid >> 6][0] = (uint32_t)__popcll(bm);
        wave_tot[tid >> 6][1] = (uint32_t)__popcll(bl);
        wave_tot[tid >> 6][2] = (uint32_t)__popcll(bs);
    }
    __syncthreads();
    if (tid < 3u) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kWaves; w++) sum += wave_tot[w][tid];
        block_sums[blockIdx.x * 3u + tid] = sum;
    }
}

struct SceneBuildParams {
    const uint32_t *entities;
    const float *transforms;
    float4 *entity_data;
    uint32_t *draw_buffer; // word 0 = count, draw r at words 1 + 3 r
    uint32_t *light_data;
    uint32_t *shadow_orientations, *instance_of_entity, *light_of_entity, *counts; // optional
    const uint32_t *block_sums;
    int32_t *status;
    uint32_t entity_count, instance_capacity, light_capacity, shadow_capacity;
    float luminance_cutoff;
    uint32_t shadow_index_base;
};

// EntityData::light_gpu_data (orbit_scene.cpp) of a light-bearing entity: `d` its descriptor, `t` its transform.
__device__ __forceinline__ void light_row(const uint32_t d[kEntityWords], const float t[kTransformFloats], float cutoff,
                                          uint32_t shadow_data_index, uint32_t out[kLightWords]) {
    const uint32_t kind = d[2];
    for (uint32_t k = 0; k < kLightWords; k++) out[k] = 0u;
    out[0] = kind;
    out[1] = shadow_data_index;
    out[4] = d[4], out[5] = d[5], out[6] = d[6], out[7] = d[7]; // color, intensity
    if (kind == 0u) {
        out[2] = d[9], out[3] = d[10];
    } else if (kind == 1u) {
        // glam Quat::mul_vec3 of v = (0, 0, -1): v * (w^2 - b.b) + b * (2 v.b) + (b x v) * (2 w), then negated
        const float vx = 0.0f, vy = 0.0f, vz = -1.0f;
        const float bx = t[3], by = t[4], bz = t[5], w = t[6];
        const float b2 = bx * bx + by * by + bz * bz;
        const float vb = (vx * bx + vy * by + vz * bz) * 2.0f;
        const float cx = by * vz - vy * bz, cy = bz * vx - vz * bx, cz = bx * vy - by * vx;
        const float s = w * w - b2, w2 = w * 2.0f;
        const float fx = vx * s + bx * vb + cx * w2, fy = vy * s + by * vb + cy * w2, fz = vz * s + bz * vb + cz * w2;
        out[12] = __float_as_uint(-fx), out[13] = __float_as_uint(-fy), out[14] = __float_as_uint(-fz);
        out[11] = d[8];
    } else {
        out[8] = __float_as_uint(t[0]), out[9] = __float_as_uint(t[1]), out[10] = __float_as_uint(t[2]);
        out[11] = d[8];
        out[15] = __float_as_uint(__builtin_sqrtf(__uint_as_float(d[7]) / cutoff)); // Light::outer_radius
    }
}

template <bool kAligned16>
__global__ __launch_bounds__(kUpdateThreads) void scene_build_kernel(const SceneBuildParams p) {
    // 32 KiB: first the workgroup's slab of transforms (10 KiB), then the rows of its mesh-bearing entities, compacted
    __shared__ float4 lds[kUpdateThreads * kRowVecs];
    __shared__ uint32_t lds_draws[kUpdateThreads * kDrawWords];
    __shared__ uint32_t lds_lights[kUpdateThreads * kLightWords];
    __shared__ uint32_t wave_tot[kWaves][3], wave_base[kWaves][3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * kUpdateThreads;
    const uint32_t n = p.entity_count - first < kUpdateThreads ? (uint32_t)(p.entity_count - first) : kUpdateThreads;
    // every load is issued before anything waits for one: the slab, this lane's descriptor, the totals in front
    uint32_t d[kEntityWords];
    for (uint32_t k = 0; k < kEntityWords; k++) d[k] = 0u;
    d[0] = kNone, d[2] = kNone;
    if (tid < n) {
        if (kAligned16) {
            const uint4 *src = (const uint4 *)p.entities + (first + tid) * 3u;
            const uint4 a = src[0], b = src[1], c = src[2];
            d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w, d[4] = b.x, d[5] = b.y, d[6] = b.z, d[7] = b.w;
            d[8] = c.x, d[9] = c.y, d[10] = c.z, d[11] = c.w;
        } else {
            const uint32_t *src = p.entities + (first + tid) * kEntityWords;
            for (uint32_t k = 0; k < kEntityWords; k++) d[k] = src[k];
        }
    }
    uint32_t before[3] = {0u, 0u, 0u}; // this lane's share of the totals of the workgroups in front
    for (uint32_t b = tid; b < blockIdx.x; b += kUpdateThreads)
        for (uint32_t k = 0; k < 3u; k++) before[k] += p.block_sums[b * 3u + k];
    load_transform_slab<kAligned16>(p.transforms + first * kTransformFloats, n, lds);

    const bool mesh = has_mesh(d[0]), light = has_light(d[2]), shadow = casts_shadow(d[2], d[3]);
    if (!light && d[2] != kNone) latch_status(p.status, ORBIT_E_RANGE); // a kind the host cannot produce: no light
    const uint64_t bm = __ballot(mesh), bl = __ballot(light), bs = __ballot(shadow);
    for (uint32_t k = 0; k < 3u; k++) before[k] = wave_reduce_add(before[k]);
    if (lane == 0u) {
        wave_tot[wave][0] = (uint32_t)__popcll(bm), wave_tot[wave][1] = (uint32_t)__popcll(bl);
        wave_tot[wave][2] = (uint32_t)__popcll(bs);
        for (uint32_t k = 0; k < 3u; k++) wave_base[wave][k] = before[k];
    }
    __syncthreads();
    float t[kTransformFloats];
    read_own_transform(lds, t);
    // base[k]: rank of the workgroup's first; local[k]: rank of this lane inside the workgroup; total[k]: the workgroup's
    uint32_t base[3], local[3], total[3];
    local[0] = lane_prefix(bm), local[1] = lane_prefix(bl), local[2] = lane_prefix(bs);
    for (uint32_t k = 0; k < 3u; k++) {
        base[k] = 0u, total[k] = 0u;
        for (uint32_t w = 0; w < kWaves; w++) {
            const uint32_t c = wave_tot[w][k];
            base[k] += wave_base[w][k];
            if (w < wave) local[k] += c;
            total[k] += c;
        }
    }
    __syncthreads(); // the slab is overwritten by the rows below

    const uint64_t e = first + tid;
    if (mesh) {
        float row[32];
        entity_rows(t, row, row + 16);
        put_row(lds, local[0], row);
        lds_draws[local[0] * kDrawWords] = base[0] + local[0];
        lds_draws[local[0] * kDrawWords + 1u] = d[0];
        lds_draws[local[0] * kDrawWords + 2u] = d[1];
    }
    if (light) {
        uint32_t row[kLightWords];
        light_row(d, t, p.luminance_cutoff, shadow ? p.shadow_index_base + base[2] + local[2] : kNone, row);
        for (uint32_t k = 0; k < kLightWords; k++) lds_lights[local[1] * kLightWords + k] = row[k];
    }
    if (shadow && p.shadow_orientations && base[2] + local[2] < p.shadow_capacity) {
        uint32_t *o = p.shadow_orientations + (uint64_t)(base[2] + local[2]) * 4u;
        for (uint32_t k = 0; k < 4u; k++) o[k] = __float_as_uint(t[3 + k]);
    }
    if (tid < n) {
        if (p.instance_of_entity) p.instance_of_entity[e] = mesh ? base[0] + local[0] : kNone;
        if (p.light_of_entity) p.light_of_entity[e] = light ? base[1] + local[1] : kNone;
    }
    __syncthreads();

    // rows base[0] .. base[0] + total[0] - 1, eight lanes per 128-B row: a wave's store writes eight whole lines
    const uint32_t rows_fit = base[0] < p.instance_capacity ? min(total[0], p.instance_capacity - base[0]) : 0u;
    for (uint32_t i = tid; i < rows_fit * kRowVecs; i += kUpdateThreads)
        p.entity_data[(uint64_t)base[0] * kRowVecs + i] = get_row_slot(lds, i / kRowVecs, i % kRowVecs);
    for (uint32_t i = tid; i < rows_fit * kDrawWords; i += kUpdateThreads)
        p.draw_buffer[1u + (uint64_t)base[0] * kDrawWords + i] = lds_draws[i];
    const uint32_t lights_fit = base[1] < p.light_capacity ? min(total[1], p.light_capacity - base[1]) : 0u;
    for (uint32_t i = tid; i < lights_fit * kLightWords; i += kUpdateThreads)
        p.light_data[(uint64_t)base[1] * kLightWords + i] = lds_lights[i];

    if (blockIdx.x == gridDim.x - 1u && tid == 0u) { // the last workgroup's bases + totals are the grand totals
        const uint32_t draws = base[0] + total[0], lights = base[1] + total[1], shadows = base[2] + total[2];
        if (p.draw_buffer) p.draw_buffer[0] = min(draws, p.instance_capacity);
        if (p.counts) p.counts[0] = draws, p.counts[1] = lights, p.counts[2] = shadows, p.counts[3] = p.entity_count;
        if (draws > p.instance_capacity || lights > p.light_capacity ||
            (p.shadow_orientations && shadows > p.shadow_capacity))
            latch_status(p.status, ORBIT_E_CAPACITY);
    }
}

} // namespace

hipError_t launch_scene_update(const OrbitSceneUpdate &u, uint32_t *block_sums, int32_t *status, hipStream_t s) {
    const uint32_t blocks = (uint32_t)(((uint64_t)u.entity_count + kUpdateThreads - 1) / kUpdateThreads);
    const bool aligned16 = (((uintptr_t)u.transforms | (uintptr_t)u.entities) & 15u) == 0;
    SceneBuildParams p;
    p.entities = (const uint32_t *)u.entities;
    p.transforms = (const float *)u.transforms;
    p.entity_data = (float4 *)u.entity_data;
    p.draw_buffer = (uint32_t *)u.entity_draw_buffer;
    p.light_data = (uint32_t *)u.light_data;
    p.shadow_orientations = (uint32_t *)u.shadow_orientations;
    p.instance_of_entity = u.instance_of_entity;
    p.light_of_entity = u.light_of_entity;
    p.counts = (uint32_t *)u.counts;
    p.block_sums = block_sums;
    p.status = status;
    p.entity_count = u.entity_count, p.instance_capacity = u.instance_capacity;
    p.light_capacity = u.light_capacity, p.shadow_capacity = u.shadow_capacity;
    p.luminance_cutoff = u.luminance_cutoff;
    p.shadow_index_base = u.shadow_index_base;
    if (blocks) {
        if (((uintptr_t)u.entities & 15u) == 0) // the count reads the descriptors only
            hipLaunchKernelGGL(scene_count_kernel<true>, dim3(blocks), dim3(kUpdateThreads), 0, s, p.entities,
                               u.entity_count, block_sums);
        else
            hipLaunchKernelGGL(scene_count_kernel<false>, dim3(blocks), dim3(kUpdateThreads), 0, s, p.entities,
                               u.entity_count, block_sums);
    }
    // no entities: one workgroup with nothing in front of it writes the zero count word and counts
    const dim3 grid(blocks ? blocks : 1u);
    if (aligned16)
        hipLaunchKernelGGL(scene_build_kernel<true>, grid, dim3(kUpdateThreads), 0, s, p);
    else
        hipLaunchKernelGGL(scene_build_kernel<false>, grid, dim3(kUpdateThreads), 0, s, p);
    return hipGetLastError();
}

} // namespace orbit
