// abi_cull.hip — the C ABI's culls (include/orbit_abi.h): entity and meshlet culls, the task and record-list forms,
// orbit_cull_views, the shard cull, the record list's expansion, orbit_cull_stats, orbit_scene_update_entities and
// orbit_scene_update.
#include "abi_internal.h"

namespace {

int32_t check_cull_info(OrbitCtx *ctx, const OrbitGpuCullInfo *ci) {
    if (!ci) return fail(ctx, ORBIT_E_INVALID, "cull_info is NULL");
    if (ci->cull_plane_count > ORBIT_MAX_CULL_PLANES) // assert!, draw_gen.rs:247,334,390
        return fail(ctx, ORBIT_E_PLANES, "cull_plane_count %u > %d", ci->cull_plane_count, ORBIT_MAX_CULL_PLANES);
    if (ci->projection_type > 1) return fail(ctx, ORBIT_E_INVALID, "projection_type %u", ci->projection_type);
    if (ci->occlusion_pass > 2) return fail(ctx, ORBIT_E_INVALID, "occlusion_pass %u", ci->occlusion_pass);
    return ORBIT_OK;
}

// The mesh side table an entity cull of `mesh_info_buffer` may read: only the one derived from that very buffer.
// (count: the call is a cull — orbit_cull_stats reads the table without being one)
MeshSideView mesh_side_for(OrbitMeshletStream *ms, const void *mesh_info_buffer, bool count = true) {
    if (!ms) return MeshSideView{nullptr, 0u};
    std::lock_guard<std::mutex> lock(ms->mu);
    if (ms->mesh_side == nullptr || ms->mesh_source != mesh_info_buffer || ms->mesh_hi == 0u) return MeshSideView{nullptr, 0u};
    if (count) ms->mesh_side_culls++;
    return MeshSideView{ms->mesh_side, ms->mesh_hi};
}

PyramidView make_pyramid_view(const float *texels, const uint32_t size[2],
                              const OrbitDepthPyramidLevel *levels = nullptr) {
    PyramidView v;
    v.texels = texels;
    v.levels = levels;
    v.w0 = size[0];
    v.h0 = size[1];
    v.mips = (size[0] | size[1]) ? mip_levels_from_size(size[0] > size[1] ? size[0] : size[1]) : 0;
    return v;
}

// ------------------------------------------------------------------ entity_cull
// Validates one entity cull and fills its parameter block; `scratch` owns the scan scratch the launch will use
// (`ctx` itself, or one of its view children), errors are reported on `ctx`.  Caller holds ctx->mu.
int32_t entity_cull_params(OrbitCtx *ctx, OrbitCtx *scratch, const OrbitGpuCullInfo *ci, const OrbitEntityCullBufs *b,
                           uint32_t draw_first, uint32_t entity_draw_count, bool exact_range, EntityCullParams &p,
                           bool is_cull = true) {
    int32_t rc = check_cull_info(ctx, ci);
    if (rc) return rc;
    if (ctx->rec_shift > 5u && ci->occlusion_pass != 0)
        return fail(ctx, ORBIT_E_INVALID,
                    "occlusion_pass %u with dispatch_size %u: the reference's visibility words are consistent for 32 only — an "
                    "entity gets ceil(meshlets / 32) words (src/scene.rs:427) while entity_cull.comp:222 advances a record's "
                    "word offset by meshlet_count / S; other dispatch sizes serve occlusion pass 0",
                    ci->occlusion_pass, ctx->caps.dispatch_size);
    if (!b) return fail(ctx, ORBIT_E_INVALID, "bufs is NULL");
    if (!b->entity_draw_buffer || !b->mesh_info_buffer || !b->meshlet_dispatch_buffer || !b->entity_buffer)
        return fail(ctx, ORBIT_E_MISSING, "entity_cull: a required buffer is NULL");
    if (ci->occlusion_pass != 0 && !b->visibility_buffer)
        return fail(ctx, ORBIT_E_MISSING, "occlusion_pass %u needs visibility_buffer", ci->occlusion_pass);
    if (ci->occlusion_pass == 2 &&
        ((!b->depth_pyramid && !b->depth_pyramid_levels) || !b->depth_pyramid_size[0] || !b->depth_pyramid_size[1]))
        return fail(ctx, ORBIT_E_MISSING, "occlusion_pass 2 needs depth_pyramid");
    if (draw_first % 32u) return fail(ctx, ORBIT_E_INVALID, "draw_first %u is not a multiple of 32", draw_first);
    if (entity_draw_count > ctx->caps.max_entities)
        return fail(ctx, ORBIT_E_CAPACITY, "entity_draw_count %u > caps.max_entities %u", entity_draw_count,
                    ctx->caps.max_entities);
    p.ci = *ci;
    p.entity_draw_buffer = (const uint8_t *)b->entity_draw_buffer;
    p.mesh_infos = (const OrbitMeshInfo *)b->mesh_info_buffer;
    p.mesh_side = mesh_side_for(ctx->meshlet_stream, b->mesh_info_buffer, is_cull);
    p.dispatch_buffer = (uint8_t *)b->meshlet_dispatch_buffer;
    p.entities = (const OrbitEntityData *)b->entity_buffer;
    p.visibility = b->visibility_buffer;
    p.pyr = make_pyramid_view(b->depth_pyramid, b->depth_pyramid_size, b->depth_pyramid_levels);
    p.draw_first = draw_first;
    // whole-buffer call: the reference's grid of ceil(n/256) x 256 invocations (draw_gen.rs:377);
    // range call: exactly [draw_first, draw_first + n) so that shards never overlap
    const uint64_t limit = exact_range ? (uint64_t)draw_first + entity_draw_count
                                       : ((uint64_t)entity_draw_count + 255u) / 256u * 256u;
    p.draw_limit = limit > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)limit;
    p.dispatch_capacity = b->dispatch_capacity;
    p.ne_chunks = (entity_draw_count + 255u) / 256u;
    p.rec_shift = ctx->rec_shift;
    p.arith = ctx->caps.arith_profile;
    p.proto = scratch->e_proto;
    p.block_sums = scratch->e_block_sums;
    p.sync = scratch->f_sync;
    p.ent_flags = scratch->f_ent_flags;
    p.total = scratch->e_total;
    p.status = scratch->status;
    return ORBIT_OK;
}

// debug (caps.validate_streams): is the mesh side table this entity cull reads still a mirror of its MeshInfos?
int32_t validate_mesh_side(OrbitCtx *ctx, const EntityCullParams &p, hipStream_t s) {
    if (!p.mesh_side.table || !ctx->caps.validate_streams) return ORBIT_OK;
    const hipError_t e = launch_mesh_side_validate(p.mesh_infos, 0u, p.mesh_side.count, p.mesh_side.table, ctx->status, s);
    return e == hipSuccess ? ORBIT_OK : hip_fail(ctx, e, "launch mesh_side_validate");
}

// ----------------------------------------------------------------- meshlet_cull
// What a meshlet cull writes: the commands (bufs->draw_commands_buffer, bufs->draw_capacity), one OrbitMeshTaskRecord
// per survivor into `buffer` (the mesh-shading path), or the record list into `buffer` of `capacity` (the sharded
// engine) — and then, with `also_commands`, the same evaluation's commands as well.
struct MeshletCullOut {
    enum Kind { kCommands, kTaskRecords, kRecordList } kind = kCommands;
    void *buffer = nullptr;
    uint32_t capacity = 0;
    const char *also_commands = nullptr; // kRecordList: the commands too — the entry point's name, for its error
};

// Validation + parameter block of one meshlet cull (see entity_cull_params).  Caller holds ctx->mu.
int32_t meshlet_cull_params(OrbitCtx *ctx, OrbitCtx *scratch, const OrbitGpuCullInfo *ci, const OrbitMeshletCullBufs *b,
                            const MeshletCullOut &out, MeshletCullParams &p) {
    const bool task = out.kind == MeshletCullOut::kTaskRecords, list = out.kind == MeshletCullOut::kRecordList;
    int32_t rc = check_cull_info(ctx, ci);
    if (rc) return rc;
    if (!b) return fail(ctx, ORBIT_E_INVALID, "bufs is NULL");
    if (!b->meshlet_dispatch_buffer || !b->meshlet_buffer || !b->entity_buffer || !b->material_buffer ||
        (task || list ? out.buffer : b->draw_commands_buffer) == nullptr)
        return fail(ctx, ORBIT_E_MISSING, "meshlet_cull: a required buffer is NULL");
    if (ctx->rec_shift > 5u) { // dispatch_size 64 / 128: pass 0 into a MeshletDrawCommandBuffer, nothing else
        if (ci->occlusion_pass != 0)
            return fail(ctx, ORBIT_E_INVALID,
                        "occlusion_pass %u with dispatch_size %u: the reference's visibility words are consistent for 32 only "
                        "(src/scene.rs:427 against meshlet_cull.comp:129-134, 233-254); other dispatch sizes serve pass 0",
                        ci->occlusion_pass, ctx->caps.dispatch_size);
        if (task)
            return fail(ctx, ORBIT_E_INVALID,
                        "the mesh-shading path with dispatch_size %u: MeshTaskPayload.meshlet_indices has 32 entries whatever "
                        "the dispatch size (shaders/include/types.glsl:196-200) — a record with more survivors writes past it",
                        ctx->caps.dispatch_size);
        if (list)
            return fail(ctx, ORBIT_E_INVALID, "the sharded engine's record list is defined for dispatch_size 32 (one 32-bit "
                                              "ballot per record); this context has %u", ctx->caps.dispatch_size);
    }
    const bool meshlet_occ = ci->meshlet_visibility_buffer != ORBIT_NONE;
    if (meshlet_occ && ci->occlusion_pass != 0 && !b->meshlet_visibility_buffer)
        return fail(ctx, ORBIT_E_MISSING, "cull_info declares a meshlet visibility buffer but the pointer is NULL");
    if (meshlet_occ && ci->occlusion_pass == 2 &&
        ((!b->depth_pyramid && !b->depth_pyramid_levels) || !b->depth_pyramid_size[0] || !b->depth_pyramid_size[1]))
        return fail(ctx, ORBIT_E_MISSING, "occlusion_pass 2 needs depth_pyramid");
    if (b->dispatch_capacity > ctx->caps.max_dispatches)
        return fail(ctx, ORBIT_E_CAPACITY, "dispatch_capacity %u > caps.max_dispatches %u", b->dispatch_capacity,
                    ctx->caps.max_dispatches);
    if (out.also_commands && !b->draw_commands_buffer) // the record list AND the same evaluation's commands
        return fail(ctx, ORBIT_E_MISSING, "%s: draw_commands_buffer is NULL", out.also_commands);
    p.ci = *ci;
    p.dispatch_buffer = (const uint8_t *)b->meshlet_dispatch_buffer;
    p.meshlets = (const OrbitMeshlet *)b->meshlet_buffer;
    p.ms = stream_view_for(ctx->meshlet_stream, b->meshlet_buffer, b->material_buffer);
    p.draw_buffer = (uint8_t *)(list ? out.buffer : b->draw_commands_buffer);
    p.entities = (const OrbitEntityData *)b->entity_buffer;
    p.materials = (const OrbitMaterialData *)b->material_buffer;
    p.meshlet_visibility = b->meshlet_visibility_buffer;
    p.pyr = make_pyramid_view(b->depth_pyramid, b->depth_pyramid_size, b->depth_pyramid_levels);
    p.dispatch_capacity = b->dispatch_capacity;
    if (ctx->rec_shift > 5u) { // the launches read the records of 32 that split_params_for's launch derives
        p.dispatch_buffer = scratch->m_split;
        p.dispatch_capacity = b->dispatch_capacity << (ctx->rec_shift - 5u);
    }
    p.draw_capacity = list ? out.capacity : b->draw_capacity;
    p.visible_list = list ? 2u : 0u;
    p.arith = ctx->caps.arith_profile;
    p.material_count = b->material_count;
    {   // the symmetric five-plane frustum, recognised bit for bit (kernels.h MeshletCullParams::std_planes)
        auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
        auto zero = [&](float f) { return (bits(f) & 0x7FFFFFFFu) == 0u; };
        auto fin = [&](float f) { return (bits(f) & 0x7F800000u) != 0x7F800000u; };
        const float(*pl)[4] = ci->cull_planes;
        bool ok = ci->cull_plane_count == 5;
        ok = ok && zero(pl[0][1]) && zero(pl[0][3]) && zero(pl[1][1]) && zero(pl[1][3]) &&
             bits(pl[1][0]) == (bits(pl[0][0]) ^ 0x80000000u) && bits(pl[1][2]) == bits(pl[0][2]);
        ok = ok && zero(pl[2][0]) && zero(pl[2][3]) && zero(pl[3][0]) && zero(pl[3][3]) &&
             bits(pl[3][1]) == (bits(pl[2][1]) ^ 0x80000000u) && bits(pl[3][2]) == bits(pl[2][2]);
        ok = ok && zero(pl[4][0]) && zero(pl[4][1]);
        const float v[6] = {pl[0][0], pl[0][2], pl[2][1], pl[2][2], pl[4][2], pl[4][3]};
        for (float f : v) ok = ok && fin(f);
        p.std_planes = ok ? 1u : 0u;
        for (int k = 0; k < 6; k++) p.stdp[k] = ok ? v[k] : 0.0f;
    }
    p.task_records = task ? (OrbitMeshTaskRecord *)out.buffer : nullptr;
    p.also_commands = out.also_commands ? (uint8_t *)b->draw_commands_buffer : nullptr;
    p.also_commands_capacity = out.also_commands ? b->draw_capacity : 0u;
    p.tile_counts = scratch->m_tile_counts;
    p.tile_masks = scratch->m_tile_masks;
    p.tile_payload = scratch->m_tile_payload;
    p.tile_base = scratch->m_tile_base;
    p.chunk_sums = scratch->m_chunk_sums;
    p.total = scratch->m_total;
    p.tickets = scratch->m_tickets;
    p.list_sync = scratch->m_list_sync;
    p.debug_flags = scratch->debug_flags;
    p.debug_cycles = scratch->debug_cycles;
    p.scan_patience = ctx->scan_patience;
    p.zero_page = scratch->zero_page;
    p.status = scratch->status;
    return ORBIT_OK;
}

// dispatch_size 64 / 128: the launch that turns the caller's S-sized records into the records of 32 the meshlet stage
// reads (entity_cull.hip split_records_body), on `scratch`'s buffer.
SplitRecordsParams split_params_for(const OrbitCtx *ctx, const OrbitCtx *scratch, const OrbitMeshletCullBufs *b) {
    SplitRecordsParams sp;
    sp.src = (const uint8_t *)b->meshlet_dispatch_buffer;
    sp.dst = scratch->m_split;
    sp.src_capacity = b->dispatch_capacity;
    sp.rec_shift = ctx->rec_shift;
    return sp;
}

// The event pair around a timed meshlet cull's evaluation (orbit_ctx_profile: every n-th is timed), nulls otherwise.
int32_t profile_pair(OrbitCtx *ctx, hipEvent_t &ev0, hipEvent_t &ev1) {
    ev0 = ev1 = nullptr;
    if (!ctx->profiling || (ctx->prof_calls++ % ctx->profiling) != 0) return ORBIT_OK;
    if (ctx->prof_used + 2 > ctx->prof_events.size()) {
        for (int i = 0; i < 2; i++) {
            hipEvent_t ev;
            if (hipEventCreate(&ev) != hipSuccess) return fail(ctx, ORBIT_E_HIP, "hipEventCreate");
            ctx->prof_events.push_back(ev);
        }
    }
    ev0 = ctx->prof_events[ctx->prof_used];
    ev1 = ctx->prof_events[ctx->prof_used + 1];
    ctx->prof_used += 2;
    return ORBIT_OK;
}

// debug (caps.validate_streams): is the bound stream this meshlet cull reads still a mirror of its Meshlet buffer?
int32_t validate_stream(OrbitCtx *ctx, const MeshletCullParams &p, hipStream_t s) {
    if (!p.ms.sphere || !ctx->caps.validate_streams) return ORBIT_OK;
    const hipError_t e = launch_meshlet_stream_validate(p.meshlets, p.ms, p.ms.cls0 ? p.materials : nullptr,
                                                        ctx->meshlet_stream->material_count, ctx->status, s,
                                                        stream_block_bounds(ctx->meshlet_stream));
    return e == hipSuccess ? ORBIT_OK : hip_fail(ctx, e, "launch meshlet_stream_validate");
}

// orbit_ctx_meshlet_stream_culls / _class_culls: a cull that read the bound stream (pass 1 evaluates nothing)
void count_stream_cull(OrbitCtx *ctx, const MeshletCullParams &p) {
    if (p.ms.sphere && p.ci.occlusion_pass != 1) {
        ctx->stream_culls++;
        if (p.ms.cls0) ctx->class_culls++;
    }
}

int32_t entity_cull_impl(OrbitCtx *ctx, const OrbitGpuCullInfo *ci, const OrbitEntityCullBufs *b, uint32_t draw_first,
                         uint32_t entity_draw_count, bool exact_range, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    EntityCullParams p;
    int32_t rc = entity_cull_params(ctx, ctx, ci, b, draw_first, entity_draw_count, exact_range, p);
    if (rc == ORBIT_OK) rc = validate_mesh_side(ctx, p, (hipStream_t)stream);
    if (rc) return rc;
    const hipError_t e = launch_entity_cull(p, entity_draw_count, ctx->num_cus, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch entity_cull");
    return ORBIT_OK;
}

int32_t meshlet_cull_impl(OrbitCtx *ctx, const OrbitGpuCullInfo *ci, const OrbitMeshletCullBufs *b,
                          const MeshletCullOut &out, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipStream_t s = (hipStream_t)stream;
    MeshletCullParams p;
    hipEvent_t ev0, ev1;
    int32_t rc = meshlet_cull_params(ctx, ctx, ci, b, out, p);
    if (rc == ORBIT_OK) rc = profile_pair(ctx, ev0, ev1);
    if (rc == ORBIT_OK && ci->occlusion_pass != 1) rc = validate_stream(ctx, p, s);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    if (ctx->rec_shift > 5u) e = launch_split_records(split_params_for(ctx, ctx, b), s);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch split_records");
    // Pass 0 of a perspective view in canonical arithmetic, from streams with alpha classes, into commands: decided per
    // block of 32 wherever the block's bound makes the verdict certain (meshlet_eval_blocks.hip) — same outputs
    const bool blocks = ctx->block_cull && out.kind == MeshletCullOut::kCommands && p.ms.sphere != nullptr &&
                        p.ms.cls0 != nullptr && ci->occlusion_pass == 0u && ci->projection_type == 0u && p.arith == 0u;
    e = launch_meshlet_cull(p, ctx->num_cus, s, ev0, ev1, blocks ? stream_block_bounds(ctx->meshlet_stream) : nullptr,
                            ctx->block_cull_grid);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch meshlet_cull");
    count_stream_cull(ctx, p);
    if (blocks) ctx->block_culls++;
    return ORBIT_OK;
}

// ------------------------------------------------------------------- cull_views
// The one-launch parameter block of a view (cull_fused.hip) or a shard (the shard launch) from its two stages' blocks,
// on `scratch`'s one-launch scratch; `chunks` = ceil(entity_draw_count / 256).
FusedCullParams fused_params(const EntityCullParams &ep, const MeshletCullParams &mp, const OrbitCtx *scratch,
                             uint32_t chunks) {
    FusedCullParams f{};
    f.m = mp;
    f.entity_draw_buffer = ep.entity_draw_buffer;
    f.mesh_infos = ep.mesh_infos;
    f.mesh_side = ep.mesh_side;
    f.visibility = ep.visibility;
    f.e_pyr = ep.pyr;
    f.draw_first = ep.draw_first;
    f.draw_limit = ep.draw_limit;
    f.e_dispatch_capacity = ep.dispatch_capacity;
    f.ne_chunks = chunks;
    f.e_total = ep.total;
    f.sync = scratch->f_sync;
    f.ent_flags = scratch->f_ent_flags;
    f.tile_flags = scratch->f_tile_flags;
    return f;
}

OrbitCtx *scratch_of(OrbitCtx *ctx, uint32_t k) { return k == 0 ? ctx : ctx->view_ctx[k - 1]; }

} // namespace

int32_t prepare_cull_views(OrbitCtx *ctx, const OrbitCullView *views, uint32_t count, uint32_t scratch_base,
                           PreparedCullViews &pc) {
    if (!views || count == 0) return fail(ctx, ORBIT_E_MISSING, "cull_views: no views");
    if (count > ORBIT_MAX_CULL_VIEWS || scratch_base + count > ORBIT_MAX_CULL_VIEWS)
        return fail(ctx, ORBIT_E_CAPACITY, "cull_views: %u views (max %u)", scratch_base + count, (unsigned)ORBIT_MAX_CULL_VIEWS);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    // scan scratch per view (views 1.. on child contexts), created once
    while (ctx->view_ctx.size() + 1 < scratch_base + count) {
        OrbitCtx *child = nullptr;
        const OrbitCaps child_caps = view_child_caps(ctx->caps);
        const int32_t rc = orbit_ctx_create(ctx->device, &child_caps, &child);
        if (rc != ORBIT_OK) return fail(ctx, rc, "cull_views: scratch for view %zu: %s", ctx->view_ctx.size() + 1, g_err);
        ctx->view_ctx.push_back(child);
    }
    // every view's parameter block, validated before anything is enqueued; the blocks travel by value in the
    // kernels' argument segments (a few KB)
    pc.count = count;
    for (uint32_t i = 0; i < count; i++) {
        const OrbitCullView &v = views[i];
        OrbitCtx *scratch = scratch_of(ctx, scratch_base + i);
        int32_t rc = entity_cull_params(ctx, scratch, v.cull_info, &v.entity, 0u, v.entity_draw_count, false, pc.ev.v[i]);
        if (rc == ORBIT_OK && !v.skip_meshlet_stage) {
            rc = meshlet_cull_params(ctx, scratch, v.cull_info, &v.meshlet, MeshletCullOut{}, pc.mv.v[pc.n_mesh]);
            if (rc == ORBIT_OK && ctx->rec_shift > 5u) pc.sv.v[pc.n_mesh] = split_params_for(ctx, scratch, &v.meshlet);
            if (rc == ORBIT_OK && v.meshlet.meshlet_dispatch_buffer != v.entity.meshlet_dispatch_buffer)
                rc = fail(ctx, ORBIT_E_INVALID, "view %u: the meshlet stage must read the entity stage's dispatch buffer", i);
            pc.n_mesh++;
        }
        if (rc != ORBIT_OK) return rc;
        pc.max_draws = v.entity_draw_count > pc.max_draws ? v.entity_draw_count : pc.max_draws;
    }
    // Views of the reference's own size (src/scene.rs:303, assets/mod.rs:202) are bound by launch latency, not by
    // bytes: all of them together as ONE launch per (pass, projection) (cull_fused.hip) — same outputs.  It evaluates
    // the 32-B Meshlet buffer whatever stream is bound (the survivors' command words are then in the row registers).
    // (a context that validates its stream on every cull keeps the chain: the one launch never reads the stream, and
    // the validation and ORBIT_E_RANGE are what such a context exists for)
    // (and a context of another dispatch size: the one launch hands 32-meshlet records over inside itself)
    bool fused = ctx->caps.cull_path != 1u && pc.n_mesh == count && ctx->rec_shift == 5u &&
                 !(ctx->caps.validate_streams != 0u && ctx->meshlet_stream != nullptr);
    for (uint32_t i = 0; i < count && fused; i++)
        fused = views[i].entity_draw_count != 0u &&
                (ctx->caps.cull_path == 2u || views[i].entity_draw_count <= kFusedMaxEntityDraws);
    pc.fused = fused;
    if (fused) {
        for (uint32_t i = 0; i < count; i++) {
            pc.fv.v[i] = fused_params(pc.ev.v[i], pc.mv.v[i], scratch_of(ctx, scratch_base + i),
                                      (views[i].entity_draw_count + 255u) / 256u);
            pc.fv.v[i].m.ms = MeshletStreamView{};
            pc.draws[i] = views[i].entity_draw_count;
        }
    }
    return ORBIT_OK;
}

int32_t launch_prepared_cull_views(OrbitCtx *ctx, const PreparedCullViews &pc, hipStream_t s) {
    hipError_t e;
    if (pc.fused) {
        e = launch_cull_fused_views(pc.fv, pc.draws, pc.count, ctx->num_cus, s, ctx->fused_grid);
        if (e != hipSuccess) return hip_fail(ctx, e, "launch cull_fused");
        ctx->fused_culls += pc.count;
        return ORBIT_OK;
    }
    e = launch_entity_cull_views(pc.ev, pc.count, pc.max_draws, ctx->num_cus, s);
    if (e == hipSuccess && ctx->rec_shift > 5u && pc.n_mesh) e = launch_split_records_views(pc.sv, pc.n_mesh, s);
    if (e == hipSuccess) e = launch_meshlet_cull_views(pc.mv, pc.n_mesh, ctx->num_cus, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch cull_views");
    for (uint32_t i = 0; i < pc.n_mesh; i++) count_stream_cull(ctx, pc.mv.v[i]);
    return ORBIT_OK;
}

extern "C" {

int32_t orbit_entity_cull(OrbitCtx *ctx, const OrbitGpuCullInfo *cull_info, const OrbitEntityCullBufs *bufs,
                          uint32_t entity_draw_count, void *stream) {
    return entity_cull_impl(ctx, cull_info, bufs, 0u, entity_draw_count, false, stream);
}

int32_t orbit_entity_cull_range(OrbitCtx *ctx, const OrbitGpuCullInfo *cull_info, const OrbitEntityCullBufs *bufs,
                                uint32_t draw_first, uint32_t draw_count, void *stream) {
    return entity_cull_impl(ctx, cull_info, bufs, draw_first, draw_count, true, stream);
}

int32_t orbit_meshlet_cull(OrbitCtx *ctx, const OrbitGpuCullInfo *ci, const OrbitMeshletCullBufs *b, void *stream) {
    return meshlet_cull_impl(ctx, ci, b, MeshletCullOut{}, stream);
}

int32_t orbit_meshlet_task_cull(OrbitCtx *ctx, const OrbitGpuCullInfo *ci, const OrbitMeshletCullBufs *b,
                                OrbitMeshTaskRecord *task_records, void *stream) {
    return meshlet_cull_impl(ctx, ci, b, {MeshletCullOut::kTaskRecords, task_records}, stream);
}

int32_t orbit_meshlet_cull_visible_records(OrbitCtx *ctx, const OrbitGpuCullInfo *ci, const OrbitMeshletCullBufs *b,
                                           void *record_buffer, uint32_t record_capacity, void *stream) {
    return meshlet_cull_impl(ctx, ci, b, {MeshletCullOut::kRecordList, record_buffer, record_capacity}, stream);
}

int32_t orbit_meshlet_cull_records_and_commands(OrbitCtx *ctx, const OrbitGpuCullInfo *ci, const OrbitMeshletCullBufs *b,
                                                void *record_buffer, uint32_t record_capacity, void *stream) {
    return meshlet_cull_impl(ctx, ci, b, {MeshletCullOut::kRecordList, record_buffer, record_capacity, "records_and_commands"},
                             stream);
}

int32_t orbit_cull_views(OrbitCtx *ctx, const OrbitCullView *views, uint32_t count, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    PreparedCullViews pc;
    const int32_t rc = prepare_cull_views(ctx, views, count, 0u, pc);
    if (rc != ORBIT_OK) return rc;
    return launch_prepared_cull_views(ctx, pc, (hipStream_t)stream);
}

// One shard's cull of the sharded engine as one call: orbit_entity_cull_range + orbit_meshlet_cull_visible_records (or
// _records_and_commands) — and, for pass 0 and at most kShardMaxChunks x 256 entity-draws, ONE launch for both stages
// and the list (+ the emit launch for the commands).
int32_t orbit_cull_shard(OrbitCtx *ctx, const OrbitGpuCullInfo *ci, const OrbitEntityCullBufs *eb, uint32_t draw_first,
                         uint32_t draw_count, const OrbitMeshletCullBufs *mb, void *record_buffer,
                         uint32_t record_capacity, uint32_t with_commands, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (ctx->rec_shift != 5u)
        return fail(ctx, ORBIT_E_INVALID, "cull_shard: the sharded engine's record list is defined for dispatch_size 32; this "
                                          "context has %u", ctx->caps.dispatch_size);
    const hipStream_t s = (hipStream_t)stream;
    const MeshletCullOut out{MeshletCullOut::kRecordList, record_buffer, record_capacity, with_commands ? "cull_shard" : nullptr};
    EntityCullParams ep;
    MeshletCullParams p;
    int32_t rc = entity_cull_params(ctx, ctx, ci, eb, draw_first, draw_count, true, ep);
    if (rc == ORBIT_OK) rc = meshlet_cull_params(ctx, ctx, ci, mb, out, p);
    if (rc != ORBIT_OK) return rc;
    if (mb->meshlet_dispatch_buffer != eb->meshlet_dispatch_buffer)
        return fail(ctx, ORBIT_E_INVALID, "cull_shard: the meshlet stage must read the entity stage's dispatch buffer");
    hipEvent_t ev0, ev1;
    rc = profile_pair(ctx, ev0, ev1);
    if (rc == ORBIT_OK) rc = validate_stream(ctx, p, s);
    if (rc == ORBIT_OK) rc = validate_mesh_side(ctx, ep, s);
    if (rc != ORBIT_OK) return rc;
    const uint32_t chunks = (draw_count + 255u) / 256u;
    const bool one_launch = ci->occlusion_pass == 0u && chunks >= 1u && chunks <= kShardMaxChunks && ctx->caps.cull_path != 1u;
    hipError_t e;
    if (one_launch) {
        FusedCullParams f = fused_params(ep, p, ctx, chunks);
        f.done_flags = ctx->f_done;
        if (ev0 && (e = hipEventRecord(ev0, s)) != hipSuccess) return hip_fail(ctx, e, "hipEventRecord");
        e = launch_shard_cull(f, ctx->num_cus, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "launch shard_cull");
        if (ev1 && (e = hipEventRecord(ev1, s)) != hipSuccess) return hip_fail(ctx, e, "hipEventRecord");
        if (with_commands) { // scan + emit of the same evaluation's ballots, into the command buffer
            MeshletCullParams c = p;
            c.visible_list = 0u;
            c.draw_buffer = p.also_commands;
            c.draw_capacity = p.also_commands_capacity;
            e = launch_meshlet_scan_emit(c, ctx->num_cus, s);
            if (e != hipSuccess) return hip_fail(ctx, e, "launch scan + emit");
        }
        ctx->shard_culls++;
    } else {
        e = launch_entity_cull(ep, draw_count, ctx->num_cus, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "launch entity_cull");
        e = launch_meshlet_cull(p, ctx->num_cus, s, ev0, ev1);
        if (e != hipSuccess) return hip_fail(ctx, e, "launch meshlet_cull");
    }
    count_stream_cull(ctx, p);
    return ORBIT_OK;
}

int32_t orbit_expand_visible_records(OrbitCtx *ctx, const void *record_buffer, const void *meshlet_buffer,
                                     void *draw_commands_buffer, uint32_t draw_capacity, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!record_buffer || !meshlet_buffer || !draw_commands_buffer)
        return fail(ctx, ORBIT_E_MISSING, "expand_visible_records: NULL argument");
    const MeshletStreamView view = stream_view_for(ctx->meshlet_stream, meshlet_buffer, nullptr);
    if (view.sphere && ctx->caps.validate_streams)
        (void)launch_meshlet_stream_validate((const OrbitMeshlet *)meshlet_buffer, view, nullptr, 0, ctx->status,
                                             (hipStream_t)stream);
    const hipError_t e = launch_visible_records_expand((const uint8_t *)record_buffer, ctx->x_block_pop, kExpandBlocks,
                                                       (const OrbitMeshlet *)meshlet_buffer, view,
                                                       (uint8_t *)draw_commands_buffer, draw_capacity, ctx->zero_page,
                                                       ctx->status, (hipStream_t)stream);
    if (view.cmd) ctx->stream_culls++;
    if (e != hipSuccess) return hip_fail(ctx, e, "launch visible_records_expand");
    return ORBIT_OK;
}

// ------------------------------------------------------------- scene update
// EntityData rows from transforms (scene_update.hip).  No allocation, no scratch, no host sync: capturable on the first
// call.  The sparse form's out-of-range indices are latched on the device (ORBIT_E_RANGE), not checked here.
int32_t orbit_scene_update_entities(OrbitCtx *ctx, const OrbitEntityTransform *transforms,
                                    const uint32_t *instance_indices, uint32_t count, OrbitEntityData *entity_data,
                                    uint32_t entity_capacity, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    if (count == 0) return ORBIT_OK;
    if (!transforms || !entity_data) return fail(ctx, ORBIT_E_INVALID, "scene_update_entities: NULL buffer");
    if (((uintptr_t)transforms & 3u) || ((uintptr_t)instance_indices & 3u) || ((uintptr_t)entity_data & 15u))
        return fail(ctx, ORBIT_E_INVALID, "scene_update_entities: transforms and instance_indices must be 4-B aligned, "
                                          "entity_data 16-B aligned");
    if (!instance_indices && count > entity_capacity)
        return fail(ctx, ORBIT_E_INVALID, "scene_update_entities: dense update of %u rows into a capacity of %u", count,
                    entity_capacity);
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_scene_update_entities(transforms, instance_indices, count, entity_data, entity_capacity,
                                                      ctx->status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch scene_update_entities");
    return ORBIT_OK;
}

// The whole of update_scene from per-entity descriptors and transforms (scene_full.hip): two launches on the stream, the
// scan scratch is the context's.  No allocation, no host sync: capturable on the first call.  Capacity overflows and
// light kinds the host cannot produce are latched on the device, not checked here.
int32_t orbit_scene_update(OrbitCtx *ctx, const OrbitSceneUpdate *update, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    if (!update) return fail(ctx, ORBIT_E_INVALID, "scene_update: update is NULL");
    const OrbitSceneUpdate &u = *update;
    if (u.entity_count > 0 && (!u.entities || !u.transforms || !u.entity_data || !u.entity_draw_buffer || !u.light_data))
        return fail(ctx, ORBIT_E_INVALID, "scene_update: NULL buffer");
    if ((uintptr_t)u.entity_data & 15u) return fail(ctx, ORBIT_E_INVALID, "scene_update: entity_data must be 16-B aligned");
    if (((uintptr_t)u.entities | (uintptr_t)u.transforms | (uintptr_t)u.entity_draw_buffer | (uintptr_t)u.light_data |
         (uintptr_t)u.shadow_orientations | (uintptr_t)u.instance_of_entity | (uintptr_t)u.light_of_entity |
         (uintptr_t)u.counts) & 3u)
        return fail(ctx, ORBIT_E_INVALID, "scene_update: every buffer must be 4-B aligned");
    if (u.entity_count > ctx->caps.max_entities)
        return fail(ctx, ORBIT_E_CAPACITY, "scene_update: %u entities > caps.max_entities %u", u.entity_count,
                    ctx->caps.max_entities);
    if (u.entity_count == 0 && !u.entity_draw_buffer && !u.counts) return ORBIT_OK; // nothing to write
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_scene_update(u, ctx->s_block_sums, ctx->status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch scene_update");
    return ORBIT_OK;
}

// ------------------------------------------------------------- cull statistics
// What orbit_entity_cull + orbit_meshlet_cull with these arguments would do, counted (cull_stats.hip).  Validated by the
// culls' own parameter blocks, so it refuses what they refuse with their codes; the meshlet stage's block is the Meshlet-
// buffer evaluation's (no stream, no class path — the stream holds the same bits).  No allocation, no scratch, no host
// sync: capturable on the first call.
int32_t orbit_cull_stats(OrbitCtx *ctx, const OrbitGpuCullInfo *cull_info, const OrbitEntityCullBufs *ebufs,
                         uint32_t entity_draw_count, const OrbitMeshletCullBufs *mbufs, OrbitCullStats *stats,
                         void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    if (!stats || ((uintptr_t)stats & 7u)) return fail(ctx, ORBIT_E_INVALID, "cull_stats: stats is NULL or not 8-B aligned");
    if (ctx->rec_shift != 5u)
        return fail(ctx, ORBIT_E_INVALID, "cull_stats serves dispatch_size 32; this context has %u", ctx->caps.dispatch_size);
    std::lock_guard<std::mutex> lock(ctx->mu);
    CullStatsParams p;
    int32_t rc = entity_cull_params(ctx, ctx, cull_info, ebufs, 0u, entity_draw_count, false, p.e, false);
    if (rc) return rc;
    rc = meshlet_cull_params(ctx, ctx, cull_info, mbufs, MeshletCullOut{}, p.m);
    if (rc) return rc;
    p.m.ms = MeshletStreamView{};
    p.stats = reinterpret_cast<unsigned long long *>(stats);
    const hipError_t e = launch_cull_stats(p, ctx->num_cus, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch cull_stats");
    return ORBIT_OK;
}

} // extern "C"
