// abi_ctx.hip — the C ABI (include/orbit_abi.h), its context: version, caps, errors, create / destroy / status, the
// measurement hook and the triage-only debug entry points.  The other abi_*.hip units hold the entry points by area.
//
// Argument validation mirrors the reference's host-side failure modes
// (assert!/unwrap in src/passes/draw_gen.rs:123-133,247,334,390) as status
// codes; nothing unwinds across the boundary.  There is no host fallback: a
// missing device or an unloadable code object is ORBIT_E_NO_DEVICE.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "abi_internal.h"

thread_local char g_err[512] = "no error";

int32_t fail(OrbitCtx *ctx, int32_t code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    snprintf(g_err, sizeof(g_err), "%s", buf);
    if (ctx) snprintf(ctx->err, sizeof(ctx->err), "%s", buf);
    return code;
}

namespace {

// Carves the scratch arena at 256-B alignment: ctx's scratch pointers are `base` plus their offset, and the arena's size
// is returned.  Run once on base 0 to size the arena and once on the arena itself.
size_t layout_arena(OrbitCtx *ctx, uintptr_t base, uint64_t md32) {
    const OrbitCaps &caps = ctx->caps;
    const size_t ent = align_up((size_t)caps.max_entities, 256);
    const size_t mtiles = ((size_t)md32 + kTileRecords - 1) / kTileRecords + 1;
    const size_t cchunks = ((size_t)caps.max_clusters / 1024 + 64) * 32;
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const uintptr_t p = base + off;
        off = align_up(off + bytes, 256);
        return p;
    };
    ctx->status = (int32_t *)carve(256);
    ctx->debug_cycles = (unsigned long long *)carve(256 + 16 * 8192); // phase sums + per-wave {begin, end} wall-clock stamps (triage builds)
    ctx->zero_page = (void *)carve(256);
    ctx->g_counts = (uint32_t *)carve(256);
    ctx->m_tickets = (uint32_t *)carve((kTicketPools + kEmitTicketPools) * kTicketStride * 4);
    ctx->m_list_sync = (uint32_t *)carve(kListSyncWords * 4);
    ctx->f_done = (uint32_t *)carve((size_t)kShardDoneWords * kShardDoneStride * 4);
    ctx->f_sync = (uint32_t *)carve(kFusedSyncWords * 4);
    ctx->f_ent_flags = (uint32_t *)carve((ent / 256 + 2) * 4);
    ctx->d_tickets = (uint32_t *)carve((size_t)kMaxPyramidBatch * kDepthTicketWords * 4);
    ctx->e_proto = (OrbitMeshletDispatch *)carve(ent * sizeof(OrbitMeshletDispatch));
    ctx->e_block_sums = (uint32_t *)carve((ent / 256 + 1) * 4);
    ctx->e_total = (uint32_t *)carve(256);
    ctx->m_tile_counts = (uint32_t *)carve(mtiles * 4);
    ctx->m_tile_base = (uint32_t *)carve(mtiles * 4);
    ctx->m_total = (uint32_t *)carve(256);
    ctx->f_tile_flags = (uint32_t *)carve(((size_t)md32 / 4 + 2) * 4); // one flag per tile of 4 records (cull_fused.hip)
    // dispatch_size 64 / 128 only (carving nothing moves nothing: `off` stays 256-B aligned)
    ctx->m_split = ctx->rec_shift > 5u ? (uint8_t *)carve(ORBIT_DISPATCH_HEADER + 16 * (size_t)md32) : nullptr;
    ctx->x_block_pop = (uint32_t *)carve((size_t)kExpandBlocks * 4);
    ctx->m_tile_masks = (uint32_t *)carve(mtiles * 64);
    ctx->m_tile_payload = (Payload *)carve(mtiles * 128 * sizeof(Payload));
    ctx->m_chunk_sums = (uint32_t *)carve((mtiles / kScanChunk + 2) * 4);
    ctx->c_chunk = (uint32_t *)carve((2 * cchunks + 64) * 4);
    ctx->c_chunk_words = cchunks;
    ctx->a_view_lights = (float4 *)carve((size_t)caps.max_lights * 16 + 1024);
    ctx->a_light_flags = (uint32_t *)carve(((size_t)caps.max_lights / 32 + 64) * 4);
    ctx->a_counts = (uint32_t *)carve(((size_t)caps.max_clusters + kAssignPad) * 4);
    // assign: block_sums holds the sums of the chunks' counts (a line each); block_base the list of heavy blocks
    ctx->a_block_sums = (uint32_t *)carve((((size_t)caps.max_clusters / kScanChunk + 2) * kChunkSumStride + 64) * 4);
    ctx->a_block_base = (uint32_t *)carve(((size_t)caps.max_clusters + kAssignPad) * 4);
    ctx->a_total = (uint32_t *)carve(256);
    // light assignment: cached cluster AABBs, and per group of 256 active clusters the coarse candidate lists
    const size_t agroups = (size_t)caps.max_clusters / 256 + 1;
    const size_t aseg = (((size_t)caps.max_lights + 15) / 16 + 63) / 64 * 64;
    ctx->a_aabb = (float *)carve(((size_t)caps.max_clusters + kAssignPad) * 6 * 4);
    ctx->a_coarse = (uint32_t *)carve(agroups * 16 * aseg * 4);
    ctx->a_coarse_lights = (float4 *)carve(agroups * 16 * aseg * 16);
    ctx->a_coarse_counts = (uint32_t *)carve(agroups * 16 * 4);
    ctx->a_group_box = (float *)carve(agroups * 32);
    ctx->a_group_order = (uint32_t *)carve((agroups + 1) * 4);
    ctx->a_coarse_seg = (uint32_t)aseg;
    ctx->a_hit_cache = (uint32_t *)carve(((size_t)caps.max_clusters + kAssignPad) * kHitCache * 4);
    ctx->s_block_sums = (uint32_t *)carve((ent / 256 + 1) * 3 * 4); // last: nothing in front of it moves
    ctx->b_mesh_slices = (float *)carve((size_t)kMeshBoundsSlots * 8 * 4); // (behind it, for the same reason)
    return off;
}

} // namespace

extern "C" {

uint32_t orbit_abi_version(void) { return ORBIT_ABI_VERSION; }

void orbit_default_caps(OrbitCaps *caps) {
    if (!caps) return;
    memset(caps, 0, sizeof(*caps));
    caps->max_entities = 100000;    // src/scene.rs:303
    caps->max_dispatches = 1000000; // src/passes/draw_gen.rs:16
    caps->max_draws = 1000000;      // src/passes/draw_gen.rs:15
    caps->max_lights = 2000;        // src/scene.rs:304
    caps->max_clusters = 240 * 135 * 32; // 1920x1080, 8 px tiles, 32 slices (cluster.rs:23-33)
    caps->dispatch_size = ORBIT_MESHLET_DISPATCH_SIZE;
}

const char *orbit_last_error(const OrbitCtx *ctx) { return ctx ? ctx->err : g_err; }

int32_t orbit_ctx_create(int32_t device_id, const OrbitCaps *caps_in, OrbitCtx **out_ctx) {
    if (!out_ctx) return fail(nullptr, ORBIT_E_INVALID, "out_ctx is NULL");
    *out_ctx = nullptr;
    OrbitCaps caps;
    if (caps_in) caps = *caps_in;
    else orbit_default_caps(&caps);
    if (caps.dispatch_size != 32u && caps.dispatch_size != 64u && caps.dispatch_size != 128u)
        return fail(nullptr, ORBIT_E_INVALID, "dispatch_size %u: 32, 64 or 128 (src/graphics/device.rs:369-372)",
                    caps.dispatch_size);
    const uint32_t rec_shift = caps.dispatch_size == 32u ? 5u : caps.dispatch_size == 64u ? 6u : 7u;
    // the meshlet stage works on records of 32 whatever the caller's records hold: its scratch is sized for those
    const uint64_t md32 = (uint64_t)caps.max_dispatches << (rec_shift - 5u);
    if (md32 > max_dispatch_capacity())
        return fail(nullptr, ORBIT_E_CAPACITY, "caps.max_dispatches %u x dispatch_size %u / 32 > %u (chunk-base table of the emit launch)",
                    caps.max_dispatches, caps.dispatch_size, max_dispatch_capacity());
    if (caps.arith_profile > ORBIT_ARITH_CONTRACTED)
        return fail(nullptr, ORBIT_E_INVALID, "arith_profile %u (0 canonical, 1 contracted)", caps.arith_profile);
    if (caps.max_dispatches > max_dispatch_capacity())
        return fail(nullptr, ORBIT_E_CAPACITY, "caps.max_dispatches %u > %u (chunk-base table of the emit launch)",
                    caps.max_dispatches, max_dispatch_capacity());
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev)
        return fail(nullptr, ORBIT_E_NO_DEVICE, "no usable HIP device %d (count %d): %s; there is no CPU fallback",
                    device_id, ndev, e == hipSuccess ? "ok" : hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, ORBIT_E_NO_DEVICE, "device %d is %s; this library carries gfx950 code objects only",
                    device_id, prop.gcnArchName);
    e = hipSetDevice(device_id);
    if (e != hipSuccess) return hip_fail(nullptr, e, "hipSetDevice");
    if (caps.cull_path > 2u)
        return fail(nullptr, ORBIT_E_INVALID, "caps.cull_path %u (0 auto, 1 launch chain, 2 one-launch cull)", caps.cull_path);
    if (caps.max_views > ORBIT_MAX_CULL_VIEWS)
        return fail(nullptr, ORBIT_E_CAPACITY, "caps.max_views %u > %u", caps.max_views, (unsigned)ORBIT_MAX_CULL_VIEWS);

    OrbitCtx *ctx = new (std::nothrow) OrbitCtx();
    if (!ctx) return fail(nullptr, ORBIT_E_HIP, "out of host memory");
    ctx->device = device_id;
    ctx->num_cus = (uint32_t)prop.multiProcessorCount;
    for (uint32_t v = 0; v < kRasterVariants; v++)
        with_raster_variant((RasterVariant)v, [&](auto variant) {
            ctx->raster_blocks[v] = ctx->num_cus * raster_depth_blocks_per_cu<variant.value>();
            ctx->visibility_blocks[v] = ctx->num_cus * raster_visibility_blocks_per_cu<variant.value>();
        });
    ctx->caps = caps;
    ctx->rec_shift = rec_shift;

    // one arena for all scan scratch
    ctx->arena_bytes = layout_arena(ctx, 0, md32);
    // (Where the arena lands physically was suspected of the Meshlet-buffer evaluation's two speeds, 311 against 333-343 us
    // by process at BASELINE config 5.  Round 6 allocated four candidate arenas here and timed a probe of that
    // evaluation's write pattern against each: the probe does not tell them apart — 14.3-14.9 us on all — and engines on
    // probed and unprobed arenas ran the same 328-353 us; five engines alive on one buffer 348-352: the spread is between
    // boxes and processes, not between arenas of a process.  Removed; profiles/r06_notes.md.)
    e = hipMalloc((void **)&ctx->arena, ctx->arena_bytes);
    if (e != hipSuccess) {
        delete ctx;
        return hip_fail(nullptr, e, "hipMalloc(scratch arena)");
    }
    e = memset_now(ctx->arena, 0, ctx->arena_bytes);
    if (e != hipSuccess) {
        (void)hipFree(ctx->arena);
        delete ctx;
        return hip_fail(nullptr, e, "hipMemset(scratch arena)");
    }
    (void)layout_arena(ctx, (uintptr_t)ctx->arena, md32);
#ifdef ORBIT_TRIAGE // perf-triage builds (tools/mkvariant_any.sh); the product library reads no other environment variable
    const char *dbg = getenv("ORBIT_SP_DEBUG");
    ctx->debug_flags = dbg ? (uint32_t)atoi(dbg) : 0u;
#endif
    // ORBIT_BLOCK_CULL=0: pass 0 keeps the per-meshlet evaluation (orbit_ctx_set_block_cull) — so that one library can
    // be timed both ways by a program that knows nothing of the switch
    const char *bc = getenv("ORBIT_BLOCK_CULL");
    ctx->block_cull = !(bc && bc[0] == '0' && bc[1] == '\0');
    snprintf(ctx->err, sizeof(ctx->err), "no error");
    // scan scratch of views 1.. of orbit_cull_views, when the caller announced them
    const OrbitCaps child_caps = view_child_caps(caps);
    for (uint32_t v = 1; v < caps.max_views; v++) {
        OrbitCtx *child = nullptr;
        const int32_t rc = orbit_ctx_create(device_id, &child_caps, &child);
        if (rc != ORBIT_OK) {
            (void)orbit_ctx_destroy(ctx);
            return rc;
        }
        ctx->view_ctx.push_back(child);
    }
    *out_ctx = ctx;
    return ORBIT_OK;
}

int32_t orbit_ctx_destroy(OrbitCtx *ctx) {
    if (!ctx) return ORBIT_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (hipEvent_t ev : ctx->prof_events) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : ctx->side_event)
        if (ev) (void)hipEventDestroy(ev);
    for (hipStream_t st : ctx->side_stream)
        if (st) (void)hipStreamDestroy(st);
    for (OrbitCtx *child : ctx->view_ctx) (void)orbit_ctx_destroy(child);
    if (ctx->meshlet_stream) ctx->meshlet_stream->bindings.fetch_sub(1);
    if (ctx->arena) (void)hipFree(ctx->arena);
    delete ctx;
    return ORBIT_OK;
}

int32_t orbit_ctx_set_block_cull_grid(OrbitCtx *ctx, uint32_t max_workgroups) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->block_cull_grid = max_workgroups;
    return ORBIT_OK;
}

int32_t orbit_ctx_set_raster_grid(OrbitCtx *ctx, uint32_t max_workgroups) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->raster_grid = max_workgroups;
    return ORBIT_OK;
}

int32_t orbit_ctx_set_fused_grid(OrbitCtx *ctx, uint32_t max_workgroups) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->fused_grid = max_workgroups;
    return ORBIT_OK;
}

int32_t orbit_ctx_set_visibility_grid(OrbitCtx *ctx, uint32_t max_workgroups) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->visibility_grid = max_workgroups;
    return ORBIT_OK;
}

int32_t orbit_ctx_status(OrbitCtx *ctx, void *stream, int32_t sync) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s = (hipStream_t)stream;
    if (sync) {
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize");
    }
    int32_t v = 0;
    hipError_t e = hipMemcpy(&v, ctx->status, 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipMemcpy(status)");
    for (OrbitCtx *child : ctx->view_ctx) { // latches of the views that ran on the children's scratch
        int32_t cv = 0;
        e = hipMemcpy(&cv, child->status, 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipMemcpy(status)");
        if (cv != 0) {
            (void)memset_now(child->status, 0, 4);
            if (v == 0) v = cv;
        }
    }
    if (v != 0) {
        e = memset_now(ctx->status, 0, 4);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipMemset(status)");
        return fail(ctx, v, v == ORBIT_E_CAPACITY ? "an append overflowed a caller buffer (entries dropped)"
                            : v == ORBIT_E_RANGE  ? "a meshlet outside the bound meshlet stream was culled or expanded, "
                                                    "or a scene update named an instance index past entity_capacity, "
                                                    "or a raster call was handed a draw command that points out of range"
                            : v == ORBIT_E_STALE  ? "the bound meshlet stream no longer mirrors its meshlet buffer (update missing)"
                                                  : "device-latched error %d", v);
    }
    return ORBIT_OK;
}

// ------------------------------------------------------------- measurement hooks
int32_t orbit_ctx_profile(OrbitCtx *ctx, int32_t enable) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->profiling = enable > 0 ? (uint32_t)enable : 0u;
    ctx->prof_used = 0;
    ctx->prof_calls = 0;
    return ORBIT_OK;
}

// The hook's event pairs are created on first use (hipEventCreate + an event's first record: tens of microseconds of
// host time each) — a caller that times a region creates them BEFORE it: `pairs` pairs exist afterwards, each recorded
// once on `stream`.
int32_t orbit_ctx_profile_reserve(OrbitCtx *ctx, uint32_t pairs, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (pairs > 65536u) return fail(ctx, ORBIT_E_CAPACITY, "profile_reserve: %u pairs", pairs);
    while (ctx->prof_events.size() < 2u * (size_t)pairs) {
        hipEvent_t ev;
        hipError_t e = hipEventCreate(&ev);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipEventCreate");
        ctx->prof_events.push_back(ev);
        e = hipEventRecord(ev, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipEventRecord");
    }
    return ORBIT_OK;
}

int32_t orbit_ctx_profile_read(OrbitCtx *ctx, float *avg_ms, uint32_t *launches) {
    if (!ctx || !avg_ms || !launches) return fail(ctx, ORBIT_E_INVALID, "profile_read: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    double sum = 0.0;
    uint32_t n = 0;
    for (size_t i = 0; i + 1 < ctx->prof_used; i += 2) {
        hipError_t e = hipEventSynchronize(ctx->prof_events[i + 1]);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipEventSynchronize");
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, ctx->prof_events[i], ctx->prof_events[i + 1]);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipEventElapsedTime");
        sum += ms;
        n++;
    }
    *avg_ms = n ? (float)(sum / n) : 0.f;
    *launches = n;
    ctx->prof_used = 0;
    return ORBIT_OK;
}

// perf triage only (not part of the public ABI): per-wave {begin, end} wall_clock64 stamps of the last phase-stamped
// meshlet_eval launch (ORBIT_SP_DEBUG=8), 100 MHz ticks; out holds 2 * 8192 values
int32_t orbit_debug_read_wave_stamps(OrbitCtx *ctx, unsigned long long *out) {
    if (!ctx || !out) return ORBIT_E_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return ORBIT_E_HIP;
    if (hipMemcpy(out, ctx->debug_cycles + 32, 16 * 8192, hipMemcpyDeviceToHost) != hipSuccess) return ORBIT_E_HIP;
    return ORBIT_OK;
}

// triage only (not part of the public ABI): the progress marks of a -DORBIT_FUSED_DEBUG build of cull_fused.hip, copied
// on a stream of their own so that they can be read while a launch is still running; out holds 8192 values
int32_t orbit_debug_read_fused_marks(OrbitCtx *ctx, unsigned long long *out) {
    if (!ctx || !out) return ORBIT_E_INVALID;
    hipStream_t s;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return ORBIT_E_HIP;
    hipError_t e = hipMemcpyAsync(out, ctx->debug_cycles + 64, 8192 * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    return e == hipSuccess ? ORBIT_OK : ORBIT_E_HIP;
}

// tests only (not part of the public ABI): how many polls a workgroup of the chain emit waits for a chunk's sum before
// it scans the chunk itself (meshlet_emit.hip emit_scan_wait; default 256).  0 makes every waiting workgroup do so at
// once — the path that otherwise only runs when the launch's first workgroups are not being dispatched.
int32_t orbit_debug_set_scan_patience(OrbitCtx *ctx, uint32_t polls) {
    if (!ctx) return ORBIT_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->scan_patience = polls;
    return ORBIT_OK;
}

// tests only (not part of the public ABI): cluster_mark's z slice through the hardware log2 with its guard band
// (orbit_device.h depth_slice) against the canonical software form, for every float bit pattern in [lo_bits, hi_bits]:
// out = {mismatches, samples decided by the canonical path, bits of the largest |v_log_f32 - log2c| seen}
int32_t orbit_debug_log2_guard(OrbitCtx *ctx, uint32_t lo_bits, uint32_t hi_bits, float z_scale, float z_bias,
                               unsigned long long out[3]) {
    if (!ctx || !out || hi_bits < lo_bits) return ORBIT_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    unsigned long long *d = ctx->debug_cycles + 8;
    if (hipMemset(d, 0, 24) != hipSuccess) return ORBIT_E_HIP;
    if (launch_log2_guard_check(lo_bits, hi_bits, z_scale, z_bias, d, nullptr) != hipSuccess) return ORBIT_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return ORBIT_E_HIP;
    if (hipMemcpy(out, d, 24, hipMemcpyDeviceToHost) != hipSuccess) return ORBIT_E_HIP;
    if (hipMemset(d, 0, 24) != hipSuccess) return ORBIT_E_HIP;
    return ORBIT_OK;
}

// perf triage only (not part of the public ABI): reads and clears the per-phase cycle sums
int32_t orbit_debug_read_cycles(OrbitCtx *ctx, unsigned long long out[8]) {
    if (!ctx || !out) return ORBIT_E_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return ORBIT_E_HIP;
    if (hipMemcpy(out, ctx->debug_cycles, 64, hipMemcpyDeviceToHost) != hipSuccess) return ORBIT_E_HIP;
    if (hipMemset(ctx->debug_cycles, 0, 64) != hipSuccess) return ORBIT_E_HIP;
    return ORBIT_OK;
}

// perf triage only (not part of the public ABI): the seven wall-clock stamps a -DORBIT_TRIAGE_STAMPS build of
// depth_reduce.hip leaves in the unused words of pyramid 0's arrival counters (tools/depth_stamps.py)
int32_t orbit_debug_read_depth_stamps(OrbitCtx *ctx, unsigned long long out[7]) {
    if (!ctx || !out) return ORBIT_E_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return ORBIT_E_HIP;
    if (hipMemcpy(out, ctx->d_tickets + 2, 56, hipMemcpyDeviceToHost) != hipSuccess) return ORBIT_E_HIP;
    return ORBIT_OK;
}

// perf triage only (not part of the public ABI; all zeros unless the library was built with -DORBIT_TRIAGE): reads and
// clears the executed sphere-box test counts of the cluster assignment — coarse tests, coarse passes, count launch
// {filter, cluster} tests, write launch {filter, cluster} tests, write-launch blocks served from the hit cache, the
// largest candidate list of a group
// (the count launch's per-block {begin, end} wall-clock stamps land where orbit_debug_read_wave_stamps reads)
int32_t orbit_debug_read_cluster_tests(OrbitCtx *ctx, unsigned long long out[8]) {
    if (!ctx || !out) return ORBIT_E_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return ORBIT_E_HIP;
    if (hipMemcpy(out, ctx->debug_cycles + 16, 64, hipMemcpyDeviceToHost) != hipSuccess) return ORBIT_E_HIP;
    if (hipMemset(ctx->debug_cycles + 16, 0, 64) != hipSuccess) return ORBIT_E_HIP;
    return ORBIT_OK;
}

} // extern "C"
