// abi_dist.hip — the C ABI's multi-GPU entry points (include/orbit_abi.h): shard ranges, the list gather through RCCL
// (resolved with dlsym), the exchange without a host round trip (HIP IPC), and the segment compaction.
#include <dlfcn.h>
#include <rccl/rccl.h> // types and prototypes only: the symbols are resolved with dlsym (orbit_gather_visible)

#include "abi_internal.h"

namespace {

// RCCL entry points, resolved from the copy already loaded in the process (the one the caller's
// communicator belongs to); liborbit_cull.so itself does not link RCCL.
struct Rccl {
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    bool ok = false;
};

const Rccl &rccl() {
    static const Rccl table = [] {
        Rccl t;
        void *h = nullptr;
        for (const char *name : {"librccl.so.1", "librccl.so"}) {
            h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
            if (h) break;
        }
        if (!h)
            for (const char *name : {"librccl.so.1", "librccl.so"}) {
                h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
                if (h) break;
            }
        if (!h) return t;
        t.all_gather = (decltype(t.all_gather))dlsym(h, "ncclAllGather");
        t.send = (decltype(t.send))dlsym(h, "ncclSend");
        t.recv = (decltype(t.recv))dlsym(h, "ncclRecv");
        t.group_start = (decltype(t.group_start))dlsym(h, "ncclGroupStart");
        t.group_end = (decltype(t.group_end))dlsym(h, "ncclGroupEnd");
        t.error_string = (decltype(t.error_string))dlsym(h, "ncclGetErrorString");
        t.ok = t.all_gather && t.send && t.recv && t.group_start && t.group_end && t.error_string;
        return t;
    }();
    return table;
}

constexpr uint32_t kMaxGatherWorld = 64; // counts scratch: one 256-B carve

// Rank-ordered all-gather of {u32 count @0 | header_bytes | items of `stride` bytes} buffers.
int32_t gather_lists(OrbitCtx *ctx, void *nccl_comm, uint32_t rank, uint32_t world, const void *local_draw_buffer,
                     void *out_draw_buffer, uint32_t out_capacity, void *stream, size_t header_bytes, size_t stride) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!nccl_comm || !local_draw_buffer || !out_draw_buffer)
        return fail(ctx, ORBIT_E_MISSING, "gather_visible: NULL argument");
    if (world == 0 || world > kMaxGatherWorld || rank >= world)
        return fail(ctx, ORBIT_E_INVALID, "gather_visible: rank %u of world %u (max %u)", rank, world, kMaxGatherWorld);
    const Rccl &nc = rccl();
    if (!nc.ok) return fail(ctx, ORBIT_E_COMM, "gather_visible: librccl is not loadable in this process");
    ncclComm_t comm = (ncclComm_t)nccl_comm;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
#define ORBIT_NCCL(call, what)                                                                  \
    do {                                                                                        \
        const ncclResult_t r_ = (call);                                                         \
        if (r_ != ncclSuccess) return fail(ctx, ORBIT_E_COMM, "%s: %s", what, nc.error_string(r_)); \
    } while (0)
    // 1. counts of all ranks (4 B each), device -> host: the message sizes
    ORBIT_NCCL(nc.all_gather(local_draw_buffer, ctx->g_counts, 1, ncclUint32, comm, s), "ncclAllGather(counts)");
    uint32_t counts[kMaxGatherWorld];
    e = hipMemcpyAsync(counts, ctx->g_counts, world * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipMemcpyAsync(counts)");
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize(counts)");
    uint64_t prefix[kMaxGatherWorld + 1];
    prefix[0] = 0;
    for (uint32_t r = 0; r < world; r++) prefix[r + 1] = prefix[r] + counts[r];
    if (prefix[world] > out_capacity)
        return fail(ctx, ORBIT_E_CAPACITY, "gather_visible: %llu commands > out_capacity %u",
                    (unsigned long long)prefix[world], out_capacity);
    // 2. header = total; 3. every list straight into out + prefix[rank]
    uint8_t *out = (uint8_t *)out_draw_buffer;
    const uint8_t *mine = (const uint8_t *)local_draw_buffer + header_bytes;
    e = launch_write_word((uint32_t *)out, (uint32_t)prefix[world], s);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch write_word");
    if (counts[rank] > 0) {
        e = hipMemcpyAsync(out + header_bytes + stride * prefix[rank], mine, stride * counts[rank],
                           hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipMemcpyAsync(own list)");
    }
    if (world > 1) {
        ORBIT_NCCL(nc.group_start(), "ncclGroupStart");
        // an error inside the group must still close it (an open group would swallow the communicator's next calls)
        ncclResult_t bad = ncclSuccess;
        const char *bad_what = "";
        for (uint32_t peer = 0; peer < world && bad == ncclSuccess; peer++) {
            if (peer == rank) continue;
            if (counts[rank] > 0) {
                bad = nc.send(mine, stride * counts[rank], ncclUint8, (int)peer, comm, s);
                bad_what = "ncclSend";
            }
            if (bad == ncclSuccess && counts[peer] > 0) {
                bad = nc.recv(out + header_bytes + stride * prefix[peer], stride * counts[peer], ncclUint8, (int)peer,
                              comm, s);
                bad_what = "ncclRecv";
            }
        }
        const ncclResult_t ended = nc.group_end();
        if (bad != ncclSuccess) return fail(ctx, ORBIT_E_COMM, "%s: %s", bad_what, nc.error_string(bad));
        ORBIT_NCCL(ended, "ncclGroupEnd");
    }
#undef ORBIT_NCCL
    return ORBIT_OK;
}

int32_t compact_segments_locked(OrbitCtx *ctx, const void *segments, uint32_t world, uint32_t segment_capacity,
                                       void *out_list, uint32_t out_capacity, uint32_t header_bytes, uint32_t stride,
                                       void *stream) {
    if (!segments || !out_list) return fail(ctx, ORBIT_E_MISSING, "compact_segments: NULL argument");
    if (world == 0 || world > kMaxGatherWorld)
        return fail(ctx, ORBIT_E_INVALID, "compact_segments: world %u (max %u)", world, kMaxGatherWorld);
    if (header_bytes < 4 || header_bytes % 4u || stride == 0 || stride % 4u)
        return fail(ctx, ORBIT_E_INVALID, "compact_segments: header %u / stride %u must be multiples of 4", header_bytes,
                    stride);
    const hipError_t e = launch_compact_segments((const uint8_t *)segments, world, segment_capacity, (uint8_t *)out_list,
                                                 out_capacity, header_bytes, stride, ctx->num_cus, ctx->status,
                                                 (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch compact_segments");
    return ORBIT_OK;
}

} // namespace

extern "C" {

void orbit_shard_range(uint32_t n, uint32_t rank, uint32_t world, uint32_t *begin, uint32_t *end) {
    // contiguous ranges cut at multiples of 32 so entity-bitset words are rank-private
    if (world == 0) world = 1;
    const uint64_t words = ((uint64_t)n + 31u) / 32u;
    uint64_t b = words * rank / world * 32u, e = words * (rank + 1ull) / world * 32u;
    if (b > n) b = n;
    if (e > n) e = n;
    if (begin) *begin = (uint32_t)b;
    if (end) *end = (uint32_t)e;
}


// ------------------------------------------------------------------- exchange without a host round trip
int32_t orbit_p2p_alloc(OrbitCtx *ctx, uint64_t bytes, void **out_ptr, uint8_t out_handle[ORBIT_P2P_HANDLE_BYTES]) {
    static_assert(sizeof(hipIpcMemHandle_t) == ORBIT_P2P_HANDLE_BYTES, "handle size");
    if (!ctx || !out_ptr || !out_handle || bytes == 0) return fail(ctx, ORBIT_E_INVALID, "p2p_alloc: bad argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    *out_ptr = nullptr;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    // Fine-grained device memory: what a peer GPU stores into it over xGMI — the list segments, and the counts and
    // completion words this device's waiting kernel polls while it runs — must be visible to this device without a
    // kernel boundary in between.  Ordinary (coarse-grained) device memory is only coherent between devices at kernel
    // boundaries: the device's L2 may keep serving a polled control word it cached before the peer's store arrived.
    void *ptr = nullptr;
    e = hipExtMallocWithFlags(&ptr, bytes, hipDeviceMallocFinegrained);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipExtMallocWithFlags(p2p buffer, fine-grained)");
    e = memset_now(ptr, 0, bytes);
    if (e == hipSuccess) e = hipIpcGetMemHandle(reinterpret_cast<hipIpcMemHandle_t *>(out_handle), ptr);
    if (e != hipSuccess) {
        (void)hipFree(ptr);
        return hip_fail(ctx, e, "hipIpcGetMemHandle (is HSA_ENABLE_IPC_MODE_LEGACY=0 set?)");
    }
    *out_ptr = ptr;
    return ORBIT_OK;
}

int32_t orbit_p2p_free(OrbitCtx *ctx, void *ptr) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ptr) return ORBIT_OK;
    const hipError_t e = hipFree(ptr);
    return e == hipSuccess ? ORBIT_OK : hip_fail(ctx, e, "hipFree(p2p buffer)");
}

int32_t orbit_p2p_open(OrbitCtx *ctx, const uint8_t handle[ORBIT_P2P_HANDLE_BYTES], void **out_peer_ptr) {
    if (!ctx || !handle || !out_peer_ptr) return fail(ctx, ORBIT_E_INVALID, "p2p_open: bad argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    *out_peer_ptr = nullptr;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    void *ptr = nullptr;
    e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipIpcOpenMemHandle");
    *out_peer_ptr = ptr;
    return ORBIT_OK;
}

int32_t orbit_p2p_close(OrbitCtx *ctx, void *peer_ptr) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!peer_ptr) return ORBIT_OK;
    const hipError_t e = hipIpcCloseMemHandle(peer_ptr);
    return e == hipSuccess ? ORBIT_OK : hip_fail(ctx, e, "hipIpcCloseMemHandle");
}

int32_t orbit_exchange_list(OrbitCtx *ctx, const void *local_list, uint32_t rank, uint32_t world,
                            void *const *out_buffers, void *const *ctrl_buffers, uint32_t out_capacity,
                            uint32_t header_bytes, uint32_t stride, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!local_list || !out_buffers || !ctrl_buffers) return fail(ctx, ORBIT_E_MISSING, "exchange_list: NULL argument");
    if (world == 0 || world > ORBIT_P2P_MAX_WORLD || rank >= world)
        return fail(ctx, ORBIT_E_INVALID, "exchange_list: rank %u of world %u (max %u)", rank, world,
                    (unsigned)ORBIT_P2P_MAX_WORLD);
    if (header_bytes < 4 || header_bytes % 4u || stride == 0 || stride % 4u)
        return fail(ctx, ORBIT_E_INVALID, "exchange_list: header %u / stride %u must be multiples of 4", header_bytes,
                    stride);
    ExchangeListParams p{};
    p.local_list = (const uint8_t *)local_list;
    for (uint32_t r = 0; r < world; r++) {
        if (!out_buffers[r] || !ctrl_buffers[r]) return fail(ctx, ORBIT_E_MISSING, "exchange_list: buffer %u is NULL", r);
        p.out[r] = (uint8_t *)out_buffers[r];
        p.ctrl[r] = (uint8_t *)ctrl_buffers[r];
    }
    p.rank = rank;
    p.world = world;
    p.out_capacity = out_capacity;
    p.header_bytes = header_bytes;
    p.stride = stride;
    p.status = ctx->status;
    const hipError_t e = launch_exchange_list(p, ctx->num_cus, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch exchange_list");
    return ORBIT_OK;
}

int32_t orbit_compact_segments(OrbitCtx *ctx, const void *segments, uint32_t world, uint32_t segment_capacity,
                               void *out_list, uint32_t out_capacity, uint32_t header_bytes, uint32_t stride,
                               void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    return compact_segments_locked(ctx, segments, world, segment_capacity, out_list, out_capacity, header_bytes, stride,
                                   stream);
}

int32_t orbit_allgather_list(OrbitCtx *ctx, void *nccl_comm, uint32_t rank, uint32_t world, const void *local_list,
                             uint32_t segment_capacity, void *segments, void *out_list, uint32_t out_capacity,
                             uint32_t header_bytes, uint32_t stride, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!nccl_comm || !local_list || !segments || !out_list)
        return fail(ctx, ORBIT_E_MISSING, "allgather_list: NULL argument");
    if (world == 0 || world > kMaxGatherWorld || rank >= world)
        return fail(ctx, ORBIT_E_INVALID, "allgather_list: rank %u of world %u (max %u)", rank, world, kMaxGatherWorld);
    if (header_bytes < 4 || header_bytes % 4u || stride == 0 || stride % 4u)
        return fail(ctx, ORBIT_E_INVALID, "allgather_list: header %u / stride %u must be multiples of 4", header_bytes,
                    stride);
    const Rccl &nc = rccl();
    if (!nc.ok) return fail(ctx, ORBIT_E_COMM, "allgather_list: librccl is not loadable in this process");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    // ONE collective of a fixed size: every rank's whole segment {count | header | segment_capacity items}.  Nothing is
    // read back, nothing waits: the counts stay on the device, where the compaction reads them.
    const size_t seg_bytes = (size_t)header_bytes + (size_t)stride * segment_capacity;
    const ncclResult_t r = nc.all_gather(local_list, segments, seg_bytes, ncclUint8, (ncclComm_t)nccl_comm, (hipStream_t)stream);
    if (r != ncclSuccess) return fail(ctx, ORBIT_E_COMM, "ncclAllGather(list segments): %s", nc.error_string(r));
    return compact_segments_locked(ctx, segments, world, segment_capacity, out_list, out_capacity, header_bytes, stride,
                                   stream);
}

int32_t orbit_gather_visible(OrbitCtx *ctx, void *nccl_comm, uint32_t rank, uint32_t world,
                             const void *local_draw_buffer, void *out_draw_buffer, uint32_t out_capacity,
                             void *stream) {
    return gather_lists(ctx, nccl_comm, rank, world, local_draw_buffer, out_draw_buffer, out_capacity, stream,
                        ORBIT_DRAW_HEADER, sizeof(OrbitMeshletDrawCommand));
}

} // extern "C"
