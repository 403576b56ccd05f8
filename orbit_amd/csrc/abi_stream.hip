// abi_stream.hip — the C ABI's meshlet streams (include/orbit_abi.h): derived arrays of a Meshlet buffer that the
// culls of the contexts they are bound to read, the mesh side table, and the per-context cull counters.
#include "abi_internal.h"

namespace {

// meshes the side table holds when none was asked for more: 32 MB (the reference's MAX_MESH_COUNT is 10 000)
constexpr uint32_t kMeshSideMinCapacity = 1u << 20;

// Enqueues the read-back of the stream's class flag behind the launch that may have set it.  On a stream that is being
// captured into a graph nothing runs now and an event query would invalidate the capture: the outcome stays unknown
// (the culls keep reading material indices) until a derivation runs on a live stream.
hipError_t read_back_class_flag(OrbitMeshletStream *ms, hipStream_t s) {
    ms->other_pending = true;
    ms->other_recorded = false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return hipSuccess;
    hipError_t e = hipMemcpyAsync(ms->h_other, ms->d_other, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(ms->other_event, s);
    if (e == hipSuccess) ms->other_recorded = true;
    return e;
}

// The preconditions of `who` on a stream of the caller's: the stream given (and `buffer`, for the calls that take a
// Meshlet buffer: then a missing one is "NULL argument"), and on the context's device.
int32_t check_stream(OrbitCtx *ctx, const OrbitMeshletStream *ms, const char *who, bool takes_buffer = false, const void *buffer = nullptr) {
    if (takes_buffer ? !ms || !buffer : !ms)
        return fail(ctx, ORBIT_E_MISSING, takes_buffer ? "%s: NULL argument" : "%s: stream is NULL", who);
    if (ms->device != ctx->device) return fail(ctx, ORBIT_E_INVALID, "%s: stream lives on device %d", who, ms->device);
    return ORBIT_OK;
}

} // namespace

extern "C" {

int32_t orbit_meshlet_stream_create(OrbitCtx *ctx, uint64_t first_meshlet, uint64_t capacity,
                                    OrbitMeshletStream **out_stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!out_stream) return fail(ctx, ORBIT_E_MISSING, "meshlet_stream_create: out_stream is NULL");
    *out_stream = nullptr;
    // 32-bit meshlet indices; the kernels address the arrays through buffer resources (32-bit byte offsets: 16 B per
    // meshlet stay below 2 GiB, so the "no access" offset of meshlet_cull.hip lies outside every array)
    if (capacity == 0 || capacity > (1ull << 27) || first_meshlet + capacity > 0xFFFFFFFFull)
        return fail(ctx, ORBIT_E_INVALID, "meshlet_stream_create: range [%llu, +%llu) (at most 2^27 meshlets per stream)",
                    (unsigned long long)first_meshlet, (unsigned long long)capacity);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    OrbitMeshletStream *ms = new (std::nothrow) OrbitMeshletStream();
    if (!ms) return fail(ctx, ORBIT_E_HIP, "out of host memory");
    ms->device = ctx->device;
    ms->first = first_meshlet;
    ms->capacity = capacity;
    // one bit per meshlet in words aligned to global index 0, plus the word behind a record that ends the range
    const size_t bit_words = (size_t)(((first_meshlet + capacity + 31u) >> 5) - (first_meshlet >> 5)) + 2u;
    struct {
        void **p;
        size_t bytes;
        int fill;
    } arrays[] = {{(void **)&ms->sphere, capacity * sizeof(uint4), 0},
                  {(void **)&ms->cone, capacity * sizeof(uint32_t), 0},
                  {(void **)&ms->mat, capacity * sizeof(uint16_t) + 256u, 0},
                  {(void **)&ms->cmd, capacity * 12u, 0},
                  {(void **)&ms->cnt, capacity * sizeof(uint16_t) + 256u, 0},
                  {(void **)&ms->link, bit_words * sizeof(uint32_t), 0},
                  {(void **)&ms->base32, bit_words * sizeof(uint2), 0},
                  {(void **)&ms->blk, bit_words * sizeof(BlockBound), 0}, // not valid until derived
                  {(void **)&ms->cls0, bit_words * sizeof(uint32_t), 0xFF},  // class 3: look the material up
                  {(void **)&ms->cls1, bit_words * sizeof(uint32_t), 0xFF}};
    // Zero-filled: a meshlet inside the derived range that no update has reached (a gap between two uploads) is a
    // defined, empty meshlet — never uninitialised memory.
    for (auto &a : arrays) {
        if (e == hipSuccess) e = hipMalloc(a.p, a.bytes);
        if (e == hipSuccess) e = hipMemset(*a.p, a.fill, a.bytes); // (waited for below)
    }
    if (e == hipSuccess) e = hipMalloc((void **)&ms->d_other, 256);
    if (e == hipSuccess) e = memset_now(ms->d_other, 0, 256); // ... and every fill above: updates launch on the caller's streams
    if (e == hipSuccess) e = hipHostMalloc((void **)&ms->h_other, sizeof(uint32_t), hipHostMallocDefault);
    if (e == hipSuccess) *ms->h_other = 0u;
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ms->other_event, hipEventDisableTiming);
    if (e != hipSuccess) {
        orbit_meshlet_stream_destroy(ms);
        return hip_fail(ctx, e, "meshlet_stream_create: hipMalloc (37.65 B per meshlet)");
    }
    *out_stream = ms;
    return ORBIT_OK;
}

int32_t orbit_meshlet_stream_update(OrbitCtx *ctx, OrbitMeshletStream *ms, const void *meshlet_buffer, uint64_t first,
                                    uint64_t count, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (const int32_t rc = check_stream(ctx, ms, "meshlet_stream_update", true, meshlet_buffer)) return rc;
    if (first < ms->first || count > ms->capacity || first - ms->first > ms->capacity - count)
        return fail(ctx, ORBIT_E_CAPACITY, "meshlet_stream_update: [%llu, +%llu) outside the stream's [%llu, +%llu)",
                    (unsigned long long)first, (unsigned long long)count, (unsigned long long)ms->first,
                    (unsigned long long)ms->capacity);
    std::lock_guard<std::mutex> slock(ms->mu);
    // What was derived from another buffer says nothing about this one: the readable range starts over.  (The arrays
    // keep the other buffer's values outside [first, first + count); they are outside the new range too.)
    const bool same = ms->source == meshlet_buffer && ms->valid_hi > ms->valid_lo;
    const uint64_t lo = same ? (first < ms->valid_lo ? first : ms->valid_lo) : first;
    const uint64_t hi = same ? (first + count > ms->valid_hi ? first + count : ms->valid_hi) : first + count;
    // the link bit in front of / behind the range looks at the neighbour's derived copy: only inside the same buffer's range
    MeshletStreamView v = stream_arrays(ms, same ? ms->valid_lo : first, same ? ms->valid_hi : first + count);
    if (v.first > first) v.count += v.first - (uint32_t)first, v.first = (uint32_t)first;
    if ((uint64_t)v.first + v.count < first + count) v.count = (uint32_t)(first + count - v.first);
    hipError_t e = launch_meshlet_stream_build((const OrbitMeshlet *)meshlet_buffer, first, count, v,
                                               (const OrbitMaterialData *)ms->materials, ms->material_count, ms->d_other,
                                               ms->first, ms->first + ms->capacity, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch meshlet_stream_build");
    // the bounds of every block the update touched, from the sphere array as it now stands (all of each block that
    // the arrays hold, not only the updated part)
    if (count != 0) {
        const MeshletStreamView all = stream_arrays(ms, ms->first, ms->first + ms->capacity);
        e = launch_block_bounds_build(all.sphere, const_cast<BlockBound *>(stream_block_bounds(ms)), first >> 5,
                                      ((first + count - 1u) >> 5) - (first >> 5) + 1u, ms->first, ms->first + ms->capacity,
                                      (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "launch block_bounds_build");
    }
    if (ms->materials != nullptr && count != 0) { // the range's classes were derived: did a class 3 appear?
        e = read_back_class_flag(ms, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "meshlet_stream_update: class flag read-back");
    }
    if (count != 0) { // the stream mirrors the buffer only once the launch is enqueued
        ms->source = meshlet_buffer;
        ms->valid_lo = lo;
        ms->valid_hi = hi;
    }
    return ORBIT_OK;
}

int32_t orbit_meshlet_stream_set_materials(OrbitCtx *ctx, OrbitMeshletStream *ms, const void *material_buffer,
                                           uint32_t material_count, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::unique_lock<std::mutex> lock(ctx->mu);
    if (const int32_t rc = check_stream(ctx, ms, "meshlet_stream_set_materials")) return rc;
    if (material_buffer && material_count == 0)
        return fail(ctx, ORBIT_E_INVALID, "meshlet_stream_set_materials: material_count is 0");
    std::unique_lock<std::mutex> slock(ms->mu);
    // every meshlet the arrays hold, derived or not (the indices of never-derived ones are zero)
    ms->other_pending = true; // no cull trusts the classes until the flag of THIS derivation has come back
    ms->other_recorded = false;
    hipError_t e = hipMemsetAsync(ms->d_other, 0, sizeof(uint32_t), (hipStream_t)stream);
    if (e == hipSuccess)
        e = launch_meshlet_stream_classes(stream_arrays(ms, ms->first, ms->first + ms->capacity),
                                          (const OrbitMaterialData *)material_buffer, material_buffer ? material_count : 0u,
                                          ms->d_other, (hipStream_t)stream);
    if (e == hipSuccess) e = read_back_class_flag(ms, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch meshlet_stream_classes");
    ms->materials = material_buffer;
    ms->material_count = material_buffer ? material_count : 0u;
    // Resolved before the call returns (an upload-time call; nothing to wait for while `stream` is only being
    // captured): the first cull after set_materials takes the class kernel or the index kernel because of what the
    // stream holds, never because of when the flag's copy happened to land.  The wait itself is made WITHOUT the two
    // locks — it lasts as long as everything already queued on `stream`, and other threads' enqueues on this context
    // (or on any context the stream is bound to) have nothing to do with it; nothing is written behind it: the next
    // cull's event query finds the event complete and clears `other_pending` itself (stream_view_for).
    const bool wait = ms->other_recorded;
    hipEvent_t ev = ms->other_event;
    slock.unlock();
    lock.unlock();
    if (wait) {
        e = hipEventSynchronize(ev);
        if (e != hipSuccess) {
            lock.lock();
            return hip_fail(ctx, e, "hipEventSynchronize(alpha-class flag)");
        }
    }
    return ORBIT_OK;
}

int32_t orbit_meshlet_stream_update_meshes(OrbitCtx *ctx, OrbitMeshletStream *ms, const void *mesh_info_buffer,
                                           uint32_t first_mesh, uint32_t count, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (const int32_t rc = check_stream(ctx, ms, "meshlet_stream_update_meshes")) return rc;
    std::lock_guard<std::mutex> slock(ms->mu);
    if (!mesh_info_buffer) { // forget: entity culls read the MeshInfos again
        ms->mesh_source = nullptr;
        ms->mesh_hi = 0u;
        return ORBIT_OK;
    }
    if ((uint64_t)first_mesh + count > 0xFFFFFFFFull) return fail(ctx, ORBIT_E_INVALID, "meshlet_stream_update_meshes: range");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    if (ms->mesh_side == nullptr) { // the first update allocates (an upload-time call, like orbit_meshlet_stream_create)
        const uint32_t cap = first_mesh + count > kMeshSideMinCapacity ? first_mesh + count : kMeshSideMinCapacity;
        e = hipMalloc((void **)&ms->mesh_side, (size_t)cap * sizeof(MeshSide));
        if (e == hipSuccess) e = memset_now(ms->mesh_side, 0, (size_t)cap * sizeof(MeshSide));
        if (e != hipSuccess) {
            (void)hipFree(ms->mesh_side);
            ms->mesh_side = nullptr;
            return hip_fail(ctx, e, "meshlet_stream_update_meshes: hipMalloc (32 B per mesh)");
        }
        ms->mesh_capacity = cap;
    }
    if (first_mesh + count > ms->mesh_capacity)
        return fail(ctx, ORBIT_E_CAPACITY, "meshlet_stream_update_meshes: meshes [%u, +%u) beyond the table's %u", first_mesh,
                    count, ms->mesh_capacity);
    if (ms->mesh_source != mesh_info_buffer && ms->mesh_hi != 0u) { // another buffer: what was derived says nothing about it
        e = hipMemsetAsync(ms->mesh_side, 0, (size_t)ms->mesh_hi * sizeof(MeshSide), (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "meshlet_stream_update_meshes: hipMemsetAsync");
        ms->mesh_hi = 0u;
    }
    e = launch_mesh_side_build((const OrbitMeshInfo *)mesh_info_buffer, first_mesh, count, ms->mesh_side, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch mesh_side_build");
    if (count != 0u) {
        ms->mesh_source = mesh_info_buffer;
        if (first_mesh + count > ms->mesh_hi) ms->mesh_hi = first_mesh + count;
    }
    return ORBIT_OK;
}

uint64_t orbit_ctx_mesh_side_culls(const OrbitCtx *ctx) {
    if (!ctx || !ctx->meshlet_stream) return 0;
    std::lock_guard<std::mutex> lock(ctx->meshlet_stream->mu);
    return ctx->meshlet_stream->mesh_side_culls;
}

int32_t orbit_meshlet_stream_validate(OrbitCtx *ctx, OrbitMeshletStream *ms, const void *meshlet_buffer,
                                      const void *material_buffer, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (const int32_t rc = check_stream(ctx, ms, "meshlet_stream_validate", true, meshlet_buffer)) return rc;
    {   // the mesh side table against the mesh_info buffer it was derived from (if any)
        std::lock_guard<std::mutex> slock(ms->mu);
        if (ms->mesh_side != nullptr && ms->mesh_source != nullptr && ms->mesh_hi != 0u) {
            const hipError_t me = launch_mesh_side_validate((const OrbitMeshInfo *)ms->mesh_source, 0u, ms->mesh_hi, ms->mesh_side,
                                                            ctx->status, (hipStream_t)stream);
            if (me != hipSuccess) return hip_fail(ctx, me, "launch mesh_side_validate");
        }
    }
    MeshletStreamView v = stream_view_for(ms, meshlet_buffer, nullptr);
    if (!v.sphere) return ORBIT_OK; // mirrors another buffer (or nothing): no cull of this one reads it
    // the classes are checked against the buffer they were derived from, whether or not a cull would read them yet
    const bool classes = material_buffer != nullptr && ms->materials == material_buffer;
    if (classes) {
        const MeshletStreamView all = stream_arrays(ms, ms->first, ms->first + ms->capacity);
        v.cls0 = all.cls0, v.cls1 = all.cls1;
    }
    const hipError_t e = launch_meshlet_stream_validate((const OrbitMeshlet *)meshlet_buffer, v,
                                                        classes ? (const OrbitMaterialData *)material_buffer : nullptr,
                                                        ms->material_count, ctx->status, (hipStream_t)stream,
                                                        stream_block_bounds(ms));
    if (e != hipSuccess) return hip_fail(ctx, e, "launch meshlet_stream_validate");
    return ORBIT_OK;
}

int32_t orbit_meshlet_stream_block_bounds(OrbitCtx *ctx, OrbitMeshletStream *ms, uint64_t first_block, uint64_t count,
                                          void *out, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (const int32_t rc = check_stream(ctx, ms, "meshlet_stream_block_bounds", true, out)) return rc;
    const uint64_t b0 = ms->first >> 5, b1 = (ms->first + ms->capacity + 31u) >> 5;
    if (first_block < b0 || count > b1 - b0 || first_block - b0 > b1 - b0 - count)
        return fail(ctx, ORBIT_E_CAPACITY, "meshlet_stream_block_bounds: blocks [%llu, +%llu) outside the stream's [%llu, %llu)",
                    (unsigned long long)first_block, (unsigned long long)count, (unsigned long long)b0, (unsigned long long)b1);
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpy(out, ms->blk + (first_block - b0), count * sizeof(BlockBound), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(ctx, e, "meshlet_stream_block_bounds: read-back");
    return ORBIT_OK;
}

int32_t orbit_meshlet_stream_read_arrays(OrbitCtx *ctx, OrbitMeshletStream *ms, uint64_t first, uint64_t count,
                                         const OrbitMeshletStreamArrays *out, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (const int32_t rc = check_stream(ctx, ms, "meshlet_stream_read_arrays", true, out)) return rc;
    if (!out->sphere || !out->cone || !out->mat || !out->cmd || !out->cnt || !out->link || !out->cls0 || !out->cls1 ||
        !out->base32)
        return fail(ctx, ORBIT_E_MISSING, "meshlet_stream_read_arrays: NULL array");
    if (first < ms->first || count > ms->capacity || first - ms->first > ms->capacity - count)
        return fail(ctx, ORBIT_E_CAPACITY, "meshlet_stream_read_arrays: [%llu, +%llu) outside the stream's [%llu, +%llu)",
                    (unsigned long long)first, (unsigned long long)count, (unsigned long long)ms->first,
                    (unsigned long long)ms->capacity);
    // the words that hold [first, first + count), as the allocation counts them: word 0 = meshlets (ms->first & ~31) .. +31
    const size_t at = (size_t)(first - ms->first), w0 = (size_t)((first >> 5) - (ms->first >> 5));
    const size_t words = count != 0 ? (size_t)(((first + count - 1u) >> 5) - (first >> 5)) + 1u : 0u;
    const struct {
        void *dst;
        const void *src;
        size_t bytes;
    } copies[] = {{out->sphere, ms->sphere + at, count * sizeof(uint4)},
                  {out->cone, ms->cone + at, count * sizeof(uint32_t)},
                  {out->mat, ms->mat + at, count * sizeof(uint16_t)},
                  {out->cmd, ms->cmd + 3u * at, count * 12u},
                  {out->cnt, ms->cnt + at, count * sizeof(uint16_t)},
                  {out->link, ms->link + w0, words * sizeof(uint32_t)},
                  {out->cls0, ms->cls0 + w0, words * sizeof(uint32_t)},
                  {out->cls1, ms->cls1 + w0, words * sizeof(uint32_t)},
                  {out->base32, ms->base32 + w0, words * sizeof(uint2)}};
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    for (const auto &c : copies)
        if (e == hipSuccess && c.bytes != 0) e = hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(ctx, e, "meshlet_stream_read_arrays: read-back");
    return ORBIT_OK;
}

int32_t orbit_meshlet_stream_destroy(OrbitMeshletStream *ms) {
    if (!ms) return ORBIT_OK;
    if (ms->bindings.load() > 0)
        return fail(nullptr, ORBIT_E_INVALID, "meshlet_stream_destroy: the stream is still bound to %d context(s)",
                    ms->bindings.load());
    (void)hipFree(ms->sphere);
    (void)hipFree(ms->cone);
    (void)hipFree(ms->mat);
    (void)hipFree(ms->cmd);
    (void)hipFree(ms->cnt);
    (void)hipFree(ms->link);
    (void)hipFree(ms->base32);
    (void)hipFree(ms->blk);
    (void)hipFree(ms->cls0);
    (void)hipFree(ms->cls1);
    (void)hipFree(ms->d_other);
    (void)hipFree(ms->mesh_side);
    if (ms->h_other) (void)hipHostFree(ms->h_other);
    if (ms->other_event) (void)hipEventDestroy(ms->other_event);
    delete ms;
    return ORBIT_OK;
}

int32_t orbit_ctx_bind_meshlet_stream(OrbitCtx *ctx, OrbitMeshletStream *ms) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (const int32_t rc = ms ? check_stream(ctx, ms, "bind_meshlet_stream") : ORBIT_OK) return rc;
    if (ms) ms->bindings.fetch_add(1);
    if (ctx->meshlet_stream) ctx->meshlet_stream->bindings.fetch_sub(1);
    ctx->meshlet_stream = ms;
    return ORBIT_OK;
}

uint64_t orbit_ctx_fused_culls(const OrbitCtx *ctx) { return ctx ? ctx->fused_culls : 0; }
uint64_t orbit_ctx_meshlet_stream_culls(const OrbitCtx *ctx) { return ctx ? ctx->stream_culls : 0; }
uint64_t orbit_ctx_meshlet_class_culls(const OrbitCtx *ctx) { return ctx ? ctx->class_culls : 0; }
uint64_t orbit_ctx_shard_culls(const OrbitCtx *ctx) { return ctx ? ctx->shard_culls : 0; }
uint64_t orbit_ctx_block_culls(const OrbitCtx *ctx) { return ctx ? ctx->block_culls : 0; }

int32_t orbit_ctx_set_block_cull(OrbitCtx *ctx, uint32_t enable) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->block_cull = enable != 0u;
    return ORBIT_OK;
}

} // extern "C"
