// abi_frame.hip — the C ABI's frame passes (include/orbit_abi.h): depth pyramids, the light-cluster chain and its
// statistics, and orbit_frame_late, which runs the late culls, the cascades and the cluster chain side by side.
#include <algorithm>

#include "abi_internal.h"

extern "C" {

static uint32_t next_pow2(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

static void fill_pyramid_desc(uint32_t w0, uint32_t h0, OrbitDepthPyramidDesc *d) {
    memset(d, 0, sizeof(*d));
    d->width = w0;
    d->height = h0;
    d->mip_levels = mip_levels_from_size(w0 > h0 ? w0 : h0);
    uint32_t off = 0;
    for (uint32_t k = 0; k < d->mip_levels && k < ORBIT_MAX_PYRAMID_MIPS; k++) {
        d->mip_offset[k] = off;
        d->mip_width[k] = (w0 >> k) ? (w0 >> k) : 1; // image.rs:533
        d->mip_height[k] = (h0 >> k) ? (h0 >> k) : 1;
        off += d->mip_width[k] * d->mip_height[k];
    }
    d->total_texels = off;
}

// ----------------------------------------------------------------- depth_reduce
int32_t orbit_depth_pyramid_desc(uint32_t sw, uint32_t sh, OrbitDepthPyramidDesc *desc) {
    if (!desc || sw == 0 || sh == 0) return fail(nullptr, ORBIT_E_INVALID, "depth_pyramid_desc: bad argument");
    uint32_t w0 = next_pow2(sw) / 2, h0 = next_pow2(sh) / 2; // draw_gen.rs:458
    if (w0 == 0) w0 = 1;
    if (h0 == 0) h0 = 1;
    fill_pyramid_desc(w0, h0, desc);
    return ORBIT_OK;
}

int32_t orbit_depth_pyramid_desc_from_mip0(uint32_t w0, uint32_t h0, OrbitDepthPyramidDesc *desc) {
    if (!desc || w0 == 0 || h0 == 0) return fail(nullptr, ORBIT_E_INVALID, "depth_pyramid_desc: bad argument");
    fill_pyramid_desc(w0, h0, desc);
    return ORBIT_OK;
}

// Validates a batch of pyramids and fills the launch's parameter block (ctx->mu held; nothing is enqueued).
static int32_t prepare_depth_reduce(OrbitCtx *ctx, const OrbitDepthReduceItem *items, uint32_t count, DepthReduceBatch &b) {
    if (!items || count == 0) return fail(ctx, ORBIT_E_MISSING, "depth_reduce: no items");
    if (count > ORBIT_MAX_PYRAMID_BATCH)
        return fail(ctx, ORBIT_E_CAPACITY, "depth_reduce: %u pyramids in one batch (max %u)", count,
                    (unsigned)ORBIT_MAX_PYRAMID_BATCH);
    static_assert(ORBIT_MAX_PYRAMID_BATCH == kMaxPyramidBatch, "batch size");
    b = DepthReduceBatch{};
    b.count = count;
    b.tickets = ctx->d_tickets;
    for (uint32_t i = 0; i < count; i++) {
        const OrbitDepthReduceItem &it = items[i];
        if (!it.depth || (!it.pyramid) == (!it.levels))
            return fail(ctx, ORBIT_E_MISSING, "depth_reduce item %u: depth, and exactly one of pyramid / levels", i);
        OrbitDepthPyramidDesc d;
        const int32_t rc = orbit_depth_pyramid_desc(it.screen_width, it.screen_height, &d);
        if (rc) return rc;
        DepthReduceParams &p = b.p[i];
        p.depth = it.depth;
        p.depth_pitch = it.depth_row_pitch ? it.depth_row_pitch : it.screen_width;
        if (p.depth_pitch < it.screen_width)
            return fail(ctx, ORBIT_E_INVALID, "depth_reduce item %u: row pitch %u < width %u", i, p.depth_pitch,
                        it.screen_width);
        p.screen_w = it.screen_width;
        p.screen_h = it.screen_height;
        p.w0 = d.width;
        p.h0 = d.height;
        p.mips = d.mip_levels;
        for (uint32_t k = 0; k < d.mip_levels; k++) {
            if (it.pyramid) {
                p.level[k] = it.pyramid + d.mip_offset[k];
                p.pitch[k] = d.mip_width[k];
            } else {
                if (!it.levels[k].texels || it.levels[k].row_pitch < d.mip_width[k])
                    return fail(ctx, ORBIT_E_INVALID, "depth_reduce item %u: level %u is NULL or its pitch %u < %u", i, k,
                                it.levels[k].row_pitch, d.mip_width[k]);
                p.level[k] = it.levels[k].texels;
                p.pitch[k] = it.levels[k].row_pitch;
            }
        }
    }
    return ORBIT_OK;
}

int32_t orbit_depth_reduce_multi(OrbitCtx *ctx, const OrbitDepthReduceItem *items, uint32_t count, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DepthReduceBatch b;
    const int32_t rc = prepare_depth_reduce(ctx, items, count, b);
    if (rc != ORBIT_OK) return rc;
    const hipError_t e = launch_depth_reduce(b, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch depth_reduce");
    return ORBIT_OK;
}

int32_t orbit_depth_reduce(OrbitCtx *ctx, const float *depth, uint32_t sw, uint32_t sh, float *pyramid,
                           void *stream) {
    OrbitDepthReduceItem it{};
    it.depth = depth;
    it.screen_width = sw;
    it.screen_height = sh;
    it.pyramid = pyramid;
    if (ctx && (!depth || !pyramid)) {
        std::lock_guard<std::mutex> lock(ctx->mu);
        return fail(ctx, ORBIT_E_MISSING, "depth_reduce: NULL buffer");
    }
    return orbit_depth_reduce_multi(ctx, &it, 1, stream);
}

// ---------------------------------------------------------------- light_cluster
// The three stages behind their entry points (ctx->mu held).  `count_chunks`: the mark launch also takes the
// compaction's chunk counts (orbit_compute_clusters; the words are zero: cleared at creation and by every assignment
// that follows a counting mark); `counted`: the compaction finds them there; `clear_counts`: the assignment's first
// launch clears them again.
static int32_t cluster_mark_check(OrbitCtx *ctx, const OrbitMarkActivePush *push, const float *depth,
                                  const uint32_t *tile_depth_slice_mask, const OrbitClusterDepthBounds *depth_bounds) {
    if (!push || !depth || !tile_depth_slice_mask || !depth_bounds)
        return fail(ctx, ORBIT_E_MISSING, "cluster_mark: NULL argument");
    if (push->cluster_count[2] > 32 || push->tile_size_px == 0 || push->depth_buffer_sample_count == 0)
        return fail(ctx, ORBIT_E_INVALID, "cluster_mark: z slices %u (> 32), tile %u or samples %u invalid",
                    push->cluster_count[2], push->tile_size_px, push->depth_buffer_sample_count);
    return ORBIT_OK;
}

static int32_t cluster_mark_locked(OrbitCtx *ctx, const OrbitMarkActivePush *push, const float *depth,
                                   uint32_t *tile_depth_slice_mask, OrbitClusterDepthBounds *depth_bounds, bool count_chunks,
                                   void *stream) {
    if (const int32_t rc = cluster_mark_check(ctx, push, depth, tile_depth_slice_mask, depth_bounds)) return rc;
    ClusterMarkParams p;
    p.pc = *push;
    p.depth = depth;
    p.masks = tile_depth_slice_mask;
    p.bounds = depth_bounds;
    p.chunk_counts = count_chunks ? ctx->c_chunk + ctx->c_chunk_words : nullptr;
    hipError_t e = launch_cluster_mark(p, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch cluster_mark");
    return ORBIT_OK;
}

static int32_t cluster_compact_check(OrbitCtx *ctx, const uint32_t cluster_count[3], const uint32_t *masks,
                                     void *unique_cluster_buffer) {
    if (!cluster_count || !masks || !unique_cluster_buffer)
        return fail(ctx, ORBIT_E_MISSING, "cluster_compact: NULL argument");
    const uint64_t total = (uint64_t)cluster_count[0] * cluster_count[1] * cluster_count[2];
    if (cluster_count[2] > 32 || total > ctx->caps.max_clusters)
        return fail(ctx, ORBIT_E_CAPACITY, "cluster grid %ux%ux%u exceeds caps.max_clusters %u or 32 slices",
                    cluster_count[0], cluster_count[1], cluster_count[2], ctx->caps.max_clusters);
    return ORBIT_OK;
}

static int32_t cluster_compact_locked(OrbitCtx *ctx, const uint32_t cluster_count[3], const uint32_t *masks,
                                      void *unique_cluster_buffer, uint32_t index_capacity, bool counted, void *stream) {
    const int32_t rc = cluster_compact_check(ctx, cluster_count, masks, unique_cluster_buffer);
    if (rc != ORBIT_OK) return rc;
    ClusterCompactParams p;
    memcpy(p.cc, cluster_count, 12);
    p.masks = masks;
    p.unique = (uint8_t *)unique_cluster_buffer;
    p.index_capacity = index_capacity;
    p.chunk_counts = counted ? ctx->c_chunk + ctx->c_chunk_words : ctx->c_chunk;
    p.status = ctx->status;
    p.counted = counted;
    hipError_t e = launch_cluster_compact(p, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch cluster_compact");
    return ORBIT_OK;
}

static int32_t cluster_assign_check(OrbitCtx *ctx, const OrbitClusterCullInfo *info, const void *unique_cluster_buffer,
                                    const OrbitClusterDepthBounds *depth_bounds, const OrbitLightData *lights,
                                    void *light_index_buffer, uint32_t *cluster_offset_image) {
    if (!info || !unique_cluster_buffer || !depth_bounds || !light_index_buffer || !cluster_offset_image)
        return fail(ctx, ORBIT_E_MISSING, "cluster_assign: NULL argument");
    if (info->global_light_count > 0 && !lights) return fail(ctx, ORBIT_E_MISSING, "cluster_assign: lights is NULL");
    if (info->global_light_count > ctx->caps.max_lights)
        return fail(ctx, ORBIT_E_CAPACITY, "light count %u > caps.max_lights %u", info->global_light_count,
                    ctx->caps.max_lights);
    const uint64_t total = (uint64_t)info->cluster_count[0] * info->cluster_count[1] * info->cluster_count[2];
    if (total > ctx->caps.max_clusters)
        return fail(ctx, ORBIT_E_CAPACITY, "cluster grid exceeds caps.max_clusters %u", ctx->caps.max_clusters);
    return ORBIT_OK;
}

static int32_t cluster_assign_locked(OrbitCtx *ctx, const OrbitClusterCullInfo *info, const void *unique_cluster_buffer,
                                     const OrbitClusterDepthBounds *depth_bounds, const OrbitLightData *lights,
                                     void *light_index_buffer, uint32_t light_index_capacity, uint32_t *cluster_offset_image,
                                     uint32_t clear_counts, void *stream) {
    const int32_t rc = cluster_assign_check(ctx, info, unique_cluster_buffer, depth_bounds, lights, light_index_buffer,
                                            cluster_offset_image);
    if (rc != ORBIT_OK) return rc;
    const uint64_t total = (uint64_t)info->cluster_count[0] * info->cluster_count[1] * info->cluster_count[2];
    ClusterAssignParams p;
    p.info = *info;
    p.unique = (const uint8_t *)unique_cluster_buffer;
    p.bounds = depth_bounds;
    p.lights = lights;
    p.light_index_buffer = (uint8_t *)light_index_buffer;
    p.light_index_capacity = light_index_capacity;
    p.offset_image = cluster_offset_image;
    p.max_clusters = (uint32_t)total;
    p.view_lights = ctx->a_view_lights;
    p.light_flags = ctx->a_light_flags;
    p.counts = ctx->a_counts;
    p.aabb = ctx->a_aabb;
    p.coarse = ctx->a_coarse;
    p.coarse_lights = ctx->a_coarse_lights;
    p.hit_cache = ctx->a_hit_cache;
    p.coarse_counts = ctx->a_coarse_counts;
    p.group_box = ctx->a_group_box;
    p.group_order = ctx->a_group_order;
    p.coarse_seg = ctx->a_coarse_seg;
    p.block_sums = ctx->a_block_sums;
    p.block_base = ctx->a_block_base;
    p.total = ctx->a_total;
    p.zero_words = clear_counts ? ctx->c_chunk + ctx->c_chunk_words : nullptr;
    p.zero_count = clear_counts;
    p.status = ctx->status;
    p.debug_tests = ctx->debug_cycles + 16;
    hipError_t e = launch_cluster_assign(p, ctx->num_cus, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch cluster_assign");
    return ORBIT_OK;
}

int32_t orbit_cluster_mark(OrbitCtx *ctx, const OrbitMarkActivePush *push, const float *depth,
                           uint32_t *tile_depth_slice_mask, OrbitClusterDepthBounds *depth_bounds, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    return cluster_mark_locked(ctx, push, depth, tile_depth_slice_mask, depth_bounds, false, stream);
}

int32_t orbit_cluster_compact(OrbitCtx *ctx, const uint32_t cluster_count[3], const uint32_t *masks,
                              void *unique_cluster_buffer, uint32_t index_capacity, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    return cluster_compact_locked(ctx, cluster_count, masks, unique_cluster_buffer, index_capacity, false, stream);
}

int32_t orbit_cluster_assign(OrbitCtx *ctx, const OrbitClusterCullInfo *info, const void *unique_cluster_buffer,
                             const OrbitClusterDepthBounds *depth_bounds, const OrbitLightData *lights,
                             void *light_index_buffer, uint32_t light_index_capacity, uint32_t *cluster_offset_image,
                             void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    return cluster_assign_locked(ctx, info, unique_cluster_buffer, depth_bounds, lights, light_index_buffer,
                                 light_index_capacity, cluster_offset_image, 0u, stream);
}

// Everything orbit_compute_clusters would refuse, refused before its first launch (ctx->mu held): the mark launch leaves
// the compaction's chunk counts behind, and only the assignment's first launch clears them again.
static int32_t compute_clusters_check(OrbitCtx *ctx, const OrbitClusterFrame &c) {
    if (!c.push || !c.info) return fail(ctx, ORBIT_E_MISSING, "compute_clusters: NULL parameter block");
    for (int i = 0; i < 3; i++)
        if (c.push->cluster_count[i] != c.info->cluster_count[i])
            return fail(ctx, ORBIT_E_INVALID, "compute_clusters: cluster_count[%d] differs between push (%u) and info (%u)",
                        i, c.push->cluster_count[i], c.info->cluster_count[i]);
    int32_t rc = cluster_mark_check(ctx, c.push, c.depth, c.tile_depth_slice_mask, c.depth_bounds);
    if (rc == ORBIT_OK) rc = cluster_compact_check(ctx, c.push->cluster_count, c.tile_depth_slice_mask, c.unique_cluster_buffer);
    if (rc == ORBIT_OK)
        rc = cluster_assign_check(ctx, c.info, c.unique_cluster_buffer, c.depth_bounds, c.lights, c.light_index_buffer,
                                  c.cluster_offset_image);
    return rc;
}

static int32_t compute_clusters_launch(OrbitCtx *ctx, const OrbitClusterFrame &c, void *stream) {
    // stream order is the only dependency between the stages (cluster.rs:380-395)
    int32_t rc = cluster_mark_locked(ctx, c.push, c.depth, c.tile_depth_slice_mask, c.depth_bounds, true, stream);
    if (rc != ORBIT_OK) return rc; // (refused before its launch: nothing was counted)
    const uint32_t tiles = c.push->cluster_count[0] * c.push->cluster_count[1];
    const uint32_t count_words = c.push->cluster_count[2] * ((tiles + 1023u) / 1024u);
    rc = cluster_compact_locked(ctx, c.push->cluster_count, c.tile_depth_slice_mask, c.unique_cluster_buffer,
                                c.index_capacity, true, stream);
    if (rc == ORBIT_OK)
        rc = cluster_assign_locked(ctx, c.info, c.unique_cluster_buffer, c.depth_bounds, c.lights, c.light_index_buffer,
                                   c.light_index_capacity, c.cluster_offset_image, count_words, stream);
    if (rc != ORBIT_OK) // a launch failed behind the counting mark: the words must not stay
        (void)hipMemsetAsync(ctx->c_chunk + ctx->c_chunk_words, 0, (size_t)count_words * 4u, (hipStream_t)stream);
    return rc;
}

int32_t orbit_compute_clusters(OrbitCtx *ctx, const OrbitMarkActivePush *push, const OrbitClusterCullInfo *info,
                               const float *depth, const OrbitLightData *lights, uint32_t *tile_depth_slice_mask,
                               OrbitClusterDepthBounds *depth_bounds, void *unique_cluster_buffer,
                               uint32_t index_capacity, void *light_index_buffer, uint32_t light_index_capacity,
                               uint32_t *cluster_offset_image, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const OrbitClusterFrame c{push, info, depth, lights, tile_depth_slice_mask, depth_bounds, unique_cluster_buffer,
                              light_index_buffer, cluster_offset_image, index_capacity, light_index_capacity};
    const int32_t rc = compute_clusters_check(ctx, c);
    return rc != ORBIT_OK ? rc : compute_clusters_launch(ctx, c, stream);
}

// The late half of a frame — everything the renderer records between "the depth buffer exists" and the forward pass
// (src/app.rs:1151-1212: the late cull of render_depth_prepass, render_shadows' cascade culls, compute_clusters) — as ONE
// call whose independent chains run side by side: {pyramids -> pass-2 culls} on the caller's stream, {cascade culls} and
// {compute_clusters} on two streams of the context, forked behind what the caller had enqueued and joined before the call
// returns control of the stream (events only: capturable).  Each chain is a handful of dependent latency-bound launches on
// a device that is 95 % idle during any one of them; serially they cost their sum, side by side the longest.
int32_t orbit_frame_late(OrbitCtx *ctx, const OrbitFrameLate *f, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!f) return fail(ctx, ORBIT_E_MISSING, "frame_late: NULL descriptor");
    if (f->late_view_count + f->cascade_view_count > ORBIT_MAX_CULL_VIEWS)
        return fail(ctx, ORBIT_E_CAPACITY, "frame_late: %u views (max %u)", f->late_view_count + f->cascade_view_count,
                    (unsigned)ORBIT_MAX_CULL_VIEWS);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    // everything is validated (and every scratch set exists) before anything is enqueued or forked
    DepthReduceBatch pyr;
    PreparedCullViews late, casc;
    int32_t rc = ORBIT_OK;
    if (f->pyramid_count) rc = prepare_depth_reduce(ctx, f->pyramids, f->pyramid_count, pyr);
    if (rc == ORBIT_OK && f->late_view_count) rc = prepare_cull_views(ctx, f->late_views, f->late_view_count, 0u, late);
    if (rc == ORBIT_OK && f->cascade_view_count)
        rc = prepare_cull_views(ctx, f->cascade_views, f->cascade_view_count, f->late_view_count, casc);
    const OrbitClusterFrame *c = f->clusters;
    if (rc == ORBIT_OK && c)
        rc = compute_clusters_check(ctx, *c);
    if (rc != ORBIT_OK) return rc;
    const bool chain_a = f->pyramid_count || f->late_view_count, chain_b = f->cascade_view_count != 0, chain_c = c != nullptr;
    // the side streams and the four events: created by the first call that forks (never while anything is enqueued)
    if ((chain_b || chain_c) && !ctx->side_stream[0]) {
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipStreamCreateWithFlags(&ctx->side_stream[i], hipStreamNonBlocking);
        for (int i = 0; i < 3 && e == hipSuccess; i++) e = hipEventCreateWithFlags(&ctx->side_event[i], hipEventDisableTiming);
        if (e != hipSuccess) return hip_fail(ctx, e, "frame_late: side streams");
    }
    hipStream_t s = (hipStream_t)stream;
    // The LONGEST chain stays on the caller's stream: a forked chain starts a fork's latency late (the side stream waits
    // for an event of `s`: a cross-queue dependency, ~5 us) and its join is a wait in `s` — both are hidden only behind
    // work `s` itself still has.  Measured on configs 3 + 4 as a replayed graph: the cluster chain (59 us alone) forked
    // beside {pyramid, late cull} on `s` took 76 us; on `s` with the others forked, what the chain itself takes.  Weight =
    // dependent launches of the chain.
    const uint32_t w_a = (f->pyramid_count ? 1u : 0u) + (f->late_view_count ? (late.fused ? 1u : 5u) : 0u);
    const uint32_t w_b = chain_b ? (casc.fused ? 1u : 5u) : 0u, w_c = chain_c ? 6u : 0u;
    hipStream_t sa = s, sb = s, sc = s;
    {
        const uint32_t heaviest = (w_c >= w_a && w_c >= w_b) ? 2u : (w_a >= w_b ? 0u : 1u);
        int side = 0;
        if (chain_a && heaviest != 0u) sa = ctx->side_stream[side++];
        if (chain_b && heaviest != 1u) sb = ctx->side_stream[side++];
        if (chain_c && heaviest != 2u) sc = ctx->side_stream[side++];
    }
    const bool fork_a = chain_a && sa != s, fork_b = chain_b && sb != s, fork_c = chain_c && sc != s;
    if (fork_a || fork_b || fork_c) {
        e = hipEventRecord(ctx->side_event[0], s);
        if (e == hipSuccess && fork_a) e = hipStreamWaitEvent(sa, ctx->side_event[0], 0);
        if (e == hipSuccess && fork_b) e = hipStreamWaitEvent(sb, ctx->side_event[0], 0);
        if (e == hipSuccess && fork_c) e = hipStreamWaitEvent(sc, ctx->side_event[0], 0);
        if (e != hipSuccess) return hip_fail(ctx, e, "frame_late: fork");
    }
    // Enqueue order.  Eagerly the call is bound by the HOST (fourteen launches and seven event operations are ~45 us of
    // enqueueing for chains of 36 and 60 us): the forked chains go first — they run while the host still enqueues the
    // long one — 80.8 us for configs 3 + 4 against 89.0 the other way round and 89.6 serially.  While the stream is being
    // CAPTURED the order only decides which branch the graph runs on the launch stream, and that should be the long one:
    // replayed, 81.6 us against 93.3 (profiles/r06_notes.md, all four arrangements).
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &capture) == hipSuccess && capture != hipStreamCaptureStatusNone;
    auto run_a = [&]() -> int32_t {
        if (f->pyramid_count) {
            const hipError_t le = launch_depth_reduce(pyr, sa);
            if (le != hipSuccess) return hip_fail(ctx, le, "launch depth_reduce");
        }
        return f->late_view_count ? launch_prepared_cull_views(ctx, late, sa) : ORBIT_OK;
    };
    auto run_b = [&]() -> int32_t { return launch_prepared_cull_views(ctx, casc, sb); };
    auto run_c = [&]() -> int32_t { return compute_clusters_launch(ctx, *c, sc); };
    for (int pass = 0; pass < 2 && rc == ORBIT_OK; pass++) {
        const bool forked_now = capturing ? pass == 1 : pass == 0; // eager: forked chains first; captured: the one on `s` first
        if (rc == ORBIT_OK && chain_a && fork_a == forked_now) rc = run_a();
        if (rc == ORBIT_OK && chain_b && fork_b == forked_now) rc = run_b();
        if (rc == ORBIT_OK && chain_c && fork_c == forked_now) rc = run_c();
    }
    // join — also behind a launch error: a forked stream must come back (a capture would otherwise be left unjoined)
    int ev = 1;
    for (hipStream_t side : {fork_a ? sa : nullptr, fork_b ? sb : nullptr, fork_c ? sc : nullptr}) {
        if (!side) continue;
        e = hipEventRecord(ctx->side_event[ev], side);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, ctx->side_event[ev], 0);
        if (e != hipSuccess && rc == ORBIT_OK) rc = hip_fail(ctx, e, "frame_late: join");
        ev++;
    }
    return rc;
}

// ----------------------------------------------------------- cluster statistics
// The uncapped counts of orbit_compute_clusters for these inputs (cluster_stats.hip).  Refused by the chain's own check
// with the same codes: the buffers only the chain writes are not arguments here, and `stats` stands in for them (it is
// checked first).  No allocation, no context scratch, no host sync: capturable on the first call, and safe beside a
// chain on another stream.
int32_t orbit_cluster_stats(OrbitCtx *ctx, const OrbitMarkActivePush *push, const OrbitClusterCullInfo *info,
                            const float *depth, const OrbitLightData *lights, OrbitClusterStats *stats, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!stats || ((uintptr_t)stats & 7u)) return fail(ctx, ORBIT_E_INVALID, "cluster_stats: stats is NULL or not 8-B aligned");
    void *out = stats;
    const int32_t rc = compute_clusters_check(ctx, {push, info, depth, lights, (uint32_t *)out, (OrbitClusterDepthBounds *)out,
                                                    out, out, (uint32_t *)out, 0u, 0u});
    if (rc != ORBIT_OK) return rc;
    ClusterStatsParams p;
    p.pc = *push;
    p.info = *info;
    p.depth = depth;
    p.lights = lights;
    p.stats = reinterpret_cast<unsigned long long *>(stats);
    const uint64_t W = push->screen_size[0], H = push->screen_size[1], sc = push->depth_buffer_sample_count;
    const uint64_t ts = push->tile_size_px;
    const uint64_t covered_w = std::min<uint64_t>(W, ts * push->cluster_count[0]);
    const uint64_t covered_h = std::min<uint64_t>(H, ts * push->cluster_count[1]);
    p.samples = W * H * sc;
    p.uncovered = p.samples - covered_w * covered_h * sc;
    const hipError_t e = launch_cluster_stats(p, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch cluster_stats");
    return ORBIT_OK;
}

} // extern "C"
