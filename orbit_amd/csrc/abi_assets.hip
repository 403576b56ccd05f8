// abi_assets.hip — the C ABI's calls that read the vertex buffer (include/orbit_abi_ext.h): orbit_meshlet_bounds and
// orbit_mesh_bounds, the refit of Meshlet and MeshInfo bounds on the device (meshlet_bounds.hip), orbit_raster_depth,
// the depth prepass of the draw commands in compute (raster_depth.hip), and orbit_raster_visibility with
// orbit_visibility_resolve, the same pass keeping the winner's identity and its resolve (raster_visibility.hip), and
// orbit_visibility_compact, the visible draw list of such a buffer (visibility_compact.hip), and
// orbit_visibility_surface, its barycentrics, differences and ids per pixel (visibility_surface.hip), with
// orbit_visibility_surface_drawn, the same for a buffer drawn with the raster flags (visibility_surface_drawn.hip), and
// orbit_surface_fragments, the fragment shader's inputs per pixel from those and the vertex attributes
// (surface_fragments.hip), and orbit_fragments_shade, the clustered lighting of those pixels (fragments_shade.hip), with
// orbit_fragments_shade_shadowed, the same with cascaded shadows served (fragments_shade_shadowed.hip), and what follows
// the colour plane they leave: orbit_bloom with orbit_bloom_layout and orbit_post_process (bloom.hip), and orbit_ssao, the
// reference's ambient occlusion of the depth plane (ssao.hip).
#include "abi_internal.h"
#include "post_common.h" // bloom_layout
#include "env_common.h"  // env_layout, env_map_check, env_sample_check
#include "sky_common.h"  // sky_check

namespace {

// the two calls' view of a vertex buffer: 3 floats at i * stride + offset
int32_t check_vertex_layout(OrbitCtx *ctx, const char *who, uint32_t stride, uint32_t offset) {
    if ((uint64_t)stride < (uint64_t)offset + 12u || (stride & 3u) || (offset & 3u))
        return fail(ctx, ORBIT_E_INVALID, "%s: vertex_stride %u, position_offset %u (multiples of 4, stride >= offset + 12)",
                    who, stride, offset);
    return ORBIT_OK;
}

// what orbit_raster_depth and orbit_raster_visibility (`who`) check alike; the target buffer is the caller's to check
int32_t check_raster_job(OrbitCtx *ctx, const char *who, uint32_t flags, uint32_t vertex_stride, uint32_t position_offset,
                         uint32_t width, uint32_t height, const void *draw_commands, const void *meshlet_data,
                         const void *vertices, const void *entity_data, const void *stats) {
    if (flags & ~(ORBIT_RASTER_CLEAR | ORBIT_RASTER_CULL_NONE | ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD)) return fail(ctx, ORBIT_E_INVALID, "%s: flags %#x", who, flags);
    if (const int32_t rc = check_vertex_layout(ctx, who, vertex_stride, position_offset)) return rc;
    if (width == 0 || height == 0 || width > ORBIT_RASTER_MAX_DIM || height > ORBIT_RASTER_MAX_DIM)
        return fail(ctx, ORBIT_E_INVALID, "%s: target %u x %u (1..%u each)", who, width, height, ORBIT_RASTER_MAX_DIM);
    if (!draw_commands || !meshlet_data || !vertices || !entity_data) return fail(ctx, ORBIT_E_INVALID, "%s: NULL buffer", who);
    if ((((uintptr_t)draw_commands | (uintptr_t)meshlet_data | (uintptr_t)vertices | (uintptr_t)stats) & 3u) ||
        ((uintptr_t)entity_data & 15u))
        return fail(ctx, ORBIT_E_INVALID, "%s: every buffer must be 4-B aligned, entity_data 16-B aligned", who);
    return ORBIT_OK;
}

// orbit_ctx_set_raster_grid: the workgroups a raster launch (and its clear) may take, `grid_cap` at most (0 = no cap)
uint32_t capped_raster_grid(uint32_t resident_blocks, uint32_t grid_cap) {
    return grid_cap != 0u && (resident_blocks == 0u || grid_cap < resident_blocks) ? grid_cap : resident_blocks;
}

// The kernel of job.flags on that kernel's own resident grid, both picked by the one variant (resident_blocks: the
// context's row of the call)
hipError_t launch_raster_depth_by_flags(const OrbitRasterDepth &job, const uint32_t (&resident_blocks)[kRasterVariants],
                                        uint32_t grid_cap, int32_t *status, hipStream_t s) {
    return with_raster_variant(raster_variant(job.flags), [&](auto v) {
        return launch_raster_depth<v.value>(job, capped_raster_grid(resident_blocks[(uint32_t)v.value], grid_cap), status, s);
    });
}
hipError_t launch_raster_visibility_by_flags(const OrbitRasterVisibility &job, const uint32_t (&resident_blocks)[kRasterVariants],
                                             uint32_t grid_cap, int32_t *status, hipStream_t s) {
    return with_raster_variant(raster_variant(job.flags), [&](auto v) {
        return launch_raster_visibility<v.value>(job, capped_raster_grid(resident_blocks[(uint32_t)v.value], grid_cap), status, s);
    });
}

} // namespace

extern "C" {

// No allocation, no scratch, no host sync: capturable on the first call.  Everything that depends on the buffers'
// contents (indices, offsets, counts) is checked on the device and latched (ORBIT_E_RANGE).
int32_t orbit_meshlet_bounds(OrbitCtx *ctx, const OrbitMeshletBoundsJob *job, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    if (!job) return fail(ctx, ORBIT_E_INVALID, "meshlet_bounds: job is NULL");
    const OrbitMeshletBoundsJob &j = *job;
    if (j.flags & ~ORBIT_BOUNDS_KEEP_RECORDS) return fail(ctx, ORBIT_E_INVALID, "meshlet_bounds: flags %#x", j.flags);
    if ((j.flags & ORBIT_BOUNDS_KEEP_RECORDS) && !j.full)
        return fail(ctx, ORBIT_E_INVALID, "meshlet_bounds: KEEP_RECORDS without `full` computes nothing");
    if (const int32_t rc = check_vertex_layout(ctx, "meshlet_bounds", j.vertex_stride, j.position_offset)) return rc;
    if ((uintptr_t)j.meshlets & 15u) return fail(ctx, ORBIT_E_INVALID, "meshlet_bounds: meshlets must be 16-B aligned");
    if (((uintptr_t)j.meshlet_data | (uintptr_t)j.vertices | (uintptr_t)j.meshlet_indices | (uintptr_t)j.full) & 3u)
        return fail(ctx, ORBIT_E_INVALID, "meshlet_bounds: every buffer must be 4-B aligned");
    if (j.meshlet_count == 0) return ORBIT_OK;
    if (!j.meshlets || !j.meshlet_data || !j.vertices) return fail(ctx, ORBIT_E_INVALID, "meshlet_bounds: NULL buffer");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_meshlet_bounds(j, ctx->num_cus, ctx->status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch meshlet_bounds");
    return ORBIT_OK;
}

// Three launches per batch of ranges on the stream; the slices' partial results go through the context's scratch
// (kMeshBoundsSlots (range, slice) pairs: few ranges are cut fine, many ranges are not cut).  No allocation, no host sync.
int32_t orbit_mesh_bounds(OrbitCtx *ctx, const OrbitMeshBoundsRange *ranges, uint32_t range_count, const void *vertices,
                          uint64_t vertex_count, uint32_t vertex_stride, uint32_t position_offset,
                          OrbitMeshInfo *mesh_infos, uint32_t mesh_capacity, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    if (const int32_t rc = check_vertex_layout(ctx, "mesh_bounds", vertex_stride, position_offset)) return rc;
    if ((((uintptr_t)ranges | (uintptr_t)vertices) & 3u) || ((uintptr_t)mesh_infos & 15u))
        return fail(ctx, ORBIT_E_INVALID, "mesh_bounds: ranges and vertices must be 4-B aligned, mesh_infos 16-B aligned");
    if (range_count == 0) return ORBIT_OK;
    if (!ranges || !vertices || !mesh_infos) return fail(ctx, ORBIT_E_INVALID, "mesh_bounds: NULL buffer");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const uint32_t slices = range_count >= kMeshBoundsSlots ? 1u : kMeshBoundsSlots / range_count > 64u ? 64u : kMeshBoundsSlots / range_count;
    const uint32_t batch = kMeshBoundsSlots / slices;
    for (uint32_t first = 0; first < range_count; first += batch) {
        const uint32_t n = range_count - first < batch ? range_count - first : batch;
        const hipError_t e = launch_mesh_bounds(ranges + first, n, slices, vertices, vertex_count, vertex_stride,
                                                position_offset, mesh_infos, mesh_capacity, ctx->b_mesh_slices,
                                                ctx->status, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "launch mesh_bounds");
    }
    return ORBIT_OK;
}

// A clearing launch (CLEAR, stats) and the raster launch on the stream; the command count stays on the device.  No allocation, no scratch, no
// host sync: capturable on the first call.
int32_t orbit_raster_depth(OrbitCtx *ctx, const OrbitRasterDepth *job, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    if (!job) return fail(ctx, ORBIT_E_INVALID, "raster_depth: job is NULL");
    const OrbitRasterDepth &j = *job;
    if (const int32_t rc = check_raster_job(ctx, "raster_depth", j.flags, j.vertex_stride, j.position_offset, j.width, j.height,
                                            j.draw_commands, j.meshlet_data, j.vertices, j.entity_data, j.stats))
        return rc;
    if (!j.depth || ((uintptr_t)j.depth & 3u)) return fail(ctx, ORBIT_E_INVALID, "raster_depth: depth is NULL or not 4-B aligned");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_raster_depth_by_flags(j, ctx->raster_blocks, ctx->raster_grid, ctx->status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch raster_depth");
    return ORBIT_OK;
}

// As orbit_raster_depth, into the u64 buffer: a clearing launch (CLEAR, stats) and the raster launch.  No allocation, no
// scratch, no host sync: capturable on the first call.
int32_t orbit_raster_visibility(OrbitCtx *ctx, const OrbitRasterVisibility *job, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    if (!job) return fail(ctx, ORBIT_E_INVALID, "raster_visibility: job is NULL");
    const OrbitRasterVisibility &j = *job;
    if (const int32_t rc = check_raster_job(ctx, "raster_visibility", j.flags, j.vertex_stride, j.position_offset, j.width,
                                            j.height, j.draw_commands, j.meshlet_data, j.vertices, j.entity_data, j.stats))
        return rc;
    if ((uint64_t)j.command_base + j.max_commands > ORBIT_VIS_MAX_COMMANDS)
        return fail(ctx, ORBIT_E_INVALID, "raster_visibility: command_base %u + max_commands %u > %u (24 bits of id)",
                    j.command_base, j.max_commands, ORBIT_VIS_MAX_COMMANDS);
    if (!j.visibility || ((uintptr_t)j.visibility & 7u))
        return fail(ctx, ORBIT_E_INVALID, "raster_visibility: visibility is NULL or not 8-B aligned");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_raster_visibility_by_flags(j, ctx->visibility_blocks, ctx->raster_grid, ctx->status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch raster_visibility");
    return ORBIT_OK;
}

// A clearing launch (command_pixels, stats) and the resolve launch.  No allocation, no scratch, no host sync.
int32_t orbit_visibility_resolve(OrbitCtx *ctx, const OrbitVisibilityResolve *job, void *stream) {
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ctx is NULL");
    if (!job) return fail(ctx, ORBIT_E_INVALID, "visibility_resolve: job is NULL");
    const OrbitVisibilityResolve &j = *job;
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        return fail(ctx, ORBIT_E_INVALID, "visibility_resolve: target %u x %u (1..%u each)", j.width, j.height, ORBIT_RASTER_MAX_DIM);
    if ((uint64_t)j.command_base + j.max_commands > ORBIT_VIS_MAX_COMMANDS)
        return fail(ctx, ORBIT_E_INVALID, "visibility_resolve: command_base %u + max_commands %u > %u (24 bits of id)",
                    j.command_base, j.max_commands, ORBIT_VIS_MAX_COMMANDS);
    if (!j.visibility || ((uintptr_t)j.visibility & 7u))
        return fail(ctx, ORBIT_E_INVALID, "visibility_resolve: visibility is NULL or not 8-B aligned");
    if (!j.depth && !j.command_pixels && !j.stats) return fail(ctx, ORBIT_E_INVALID, "visibility_resolve: no output");
    if (((uintptr_t)j.depth | (uintptr_t)j.command_pixels | (uintptr_t)j.stats) & 3u)
        return fail(ctx, ORBIT_E_INVALID, "visibility_resolve: every output must be 4-B aligned");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_visibility_resolve(j, ctx->num_cus, ctx->visibility_grid, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch visibility_resolve");
    return ORBIT_OK;
}

uint64_t orbit_visibility_compact_workspace(uint32_t max_commands) { return visibility_compact_workspace_bytes(max_commands); }

// Five launches (clear, mark, scan, totals, emit) on the stream; the command count stays on the device and all scratch is
// the caller's.  No allocation, no host sync: capturable on the first call.  The job is checked before the context is
// looked at (the checks read neither), so each of them can be reached without a device: a NULL context is the last error.
int32_t orbit_visibility_compact(OrbitCtx *ctx, const OrbitVisibilityCompact *job, void *stream) {
    if (!job) return fail(ctx, ORBIT_E_INVALID, "visibility_compact: job is NULL");
    const OrbitVisibilityCompact &j = *job;
    if (j.flags & ~ORBIT_COMPACT_TRIANGLES) return fail(ctx, ORBIT_E_INVALID, "visibility_compact: flags %#x", j.flags);
    const bool cut = (j.flags & ORBIT_COMPACT_TRIANGLES) != 0u;
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        return fail(ctx, ORBIT_E_INVALID, "visibility_compact: target %u x %u (1..%u each)", j.width, j.height, ORBIT_RASTER_MAX_DIM);
    if ((uint64_t)j.command_base + j.max_commands > ORBIT_VIS_MAX_COMMANDS)
        return fail(ctx, ORBIT_E_INVALID, "visibility_compact: command_base %u + max_commands %u > %u (24 bits of id)",
                    j.command_base, j.max_commands, ORBIT_VIS_MAX_COMMANDS);
    if (j.visible_data_words > (1u << 30))
        return fail(ctx, ORBIT_E_INVALID, "visibility_compact: visible_data_words %u > 2^30 (cmd_first_index is a byte offset)",
                    j.visible_data_words);
    if (!j.visibility || !j.draw_commands || !j.triangle_masks || !j.visible_commands || !j.workspace)
        return fail(ctx, ORBIT_E_INVALID, "visibility_compact: NULL buffer");
    if (cut && (!j.meshlet_data || !j.visible_data))
        return fail(ctx, ORBIT_E_INVALID, "visibility_compact: ORBIT_COMPACT_TRIANGLES needs meshlet_data and visible_data");
    if ((((uintptr_t)j.visibility | (uintptr_t)j.workspace) & 7u) ||
        (((uintptr_t)j.draw_commands | (uintptr_t)j.meshlet_data | (uintptr_t)j.triangle_masks | (uintptr_t)j.visible_commands |
          (uintptr_t)j.visible_ids | (uintptr_t)j.visible_data | (uintptr_t)j.stats) & 3u))
        return fail(ctx, ORBIT_E_INVALID, "visibility_compact: visibility and workspace must be 8-B aligned, every other buffer 4-B aligned");
    if (j.workspace_bytes < visibility_compact_workspace_bytes(j.max_commands))
        return fail(ctx, ORBIT_E_INVALID, "visibility_compact: workspace of %llu bytes, %llu needed", (unsigned long long)j.workspace_bytes,
                    (unsigned long long)visibility_compact_workspace_bytes(j.max_commands));
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "visibility_compact: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_visibility_compact(j, ctx->num_cus, ctx->visibility_grid, ctx->status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch visibility_compact");
    return ORBIT_OK;
}

// What orbit_visibility_surface and orbit_visibility_surface_drawn ask of their block, each error with a message of its
// own under the prefix `what`.  Reads neither the context nor a device.
static int32_t check_surface_job(OrbitCtx *ctx, const char *what, const OrbitVisibilitySurface &j) {
    if (j.flags & ~ORBIT_SURFACE_CLEAR) return fail(ctx, ORBIT_E_INVALID, "%s: flags %#x", what, j.flags);
    if (const int32_t rc = check_vertex_layout(ctx, what, j.vertex_stride, j.position_offset)) return rc;
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        return fail(ctx, ORBIT_E_INVALID, "%s: target %u x %u (1..%u each)", what, j.width, j.height, ORBIT_RASTER_MAX_DIM);
    if ((uint64_t)j.command_base + j.max_commands > ORBIT_VIS_MAX_COMMANDS)
        return fail(ctx, ORBIT_E_INVALID, "%s: command_base %u + max_commands %u > %u (24 bits of id)", what, j.command_base,
                    j.max_commands, ORBIT_VIS_MAX_COMMANDS);
    if (!j.visibility || !j.draw_commands || !j.meshlet_data || !j.vertices || !j.entity_data)
        return fail(ctx, ORBIT_E_INVALID, "%s: NULL buffer", what);
    if (!j.bary && !j.grad && !j.triangle) return fail(ctx, ORBIT_E_INVALID, "%s: no output", what);
    if (j.triangle && j.vertex_count > (1ull << 32))
        return fail(ctx, ORBIT_E_INVALID, "%s: triangle with vertex_count %llu > 2^32 (a global vertex is a u32)", what,
                    (unsigned long long)j.vertex_count);
    if (((uintptr_t)j.visibility & 7u) || ((uintptr_t)j.entity_data & 15u) ||
        (((uintptr_t)j.draw_commands | (uintptr_t)j.meshlet_data | (uintptr_t)j.vertices | (uintptr_t)j.bary | (uintptr_t)j.grad |
          (uintptr_t)j.triangle | (uintptr_t)j.stats) & 3u))
        return fail(ctx, ORBIT_E_INVALID, "%s: visibility must be 8-B aligned, entity_data 16-B aligned, every other buffer 4-B aligned", what);
    return ORBIT_OK;
}

// A clearing launch (stats, and the outputs with ORBIT_SURFACE_CLEAR) and the surface launch; the command count stays on
// the device.  No allocation, no scratch, no host sync: capturable on the first call.  As orbit_visibility_compact, the job
// is checked before the context is looked at, each error with a message of its own: a NULL context is the last error.
int32_t orbit_visibility_surface(OrbitCtx *ctx, const OrbitVisibilitySurface *job, void *stream) {
    if (!job) return fail(ctx, ORBIT_E_INVALID, "visibility_surface: job is NULL");
    if (const int32_t rc = check_surface_job(ctx, "visibility_surface", *job)) return rc;
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "visibility_surface: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_visibility_surface(*job, ctx->num_cus, ctx->visibility_grid, ctx->status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch visibility_surface");
    return ORBIT_OK;
}

// orbit_visibility_surface for a buffer drawn with the raster flags `raster_flags` (S2d, S3c, S3w): the same two launches,
// the same checks.  With no flag it IS orbit_visibility_surface's launches; with one, visibility_surface_drawn.hip's.
int32_t orbit_visibility_surface_drawn(OrbitCtx *ctx, const OrbitVisibilitySurface *job, uint32_t raster_flags, void *stream) {
    if (!job) return fail(ctx, ORBIT_E_INVALID, "visibility_surface_drawn: job is NULL");
    if (raster_flags & ~(ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD))
        return fail(ctx, ORBIT_E_INVALID, "visibility_surface_drawn: raster_flags %#x (ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD)",
                    raster_flags);
    if (const int32_t rc = check_surface_job(ctx, "visibility_surface_drawn", *job)) return rc;
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "visibility_surface_drawn: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = raster_flags == 0u
                             ? launch_visibility_surface(*job, ctx->num_cus, ctx->visibility_grid, ctx->status, (hipStream_t)stream)
                             : launch_visibility_surface_drawn(*job, raster_flags, ctx->num_cus, ctx->visibility_grid, ctx->status,
                                                               (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch visibility_surface_drawn");
    return ORBIT_OK;
}

// A clearing launch (stats, and the outputs with ORBIT_FRAGMENTS_CLEAR) and the fragment launch (surface_fragments.hip);
// the command count stays on the device.  No allocation, no scratch, no host sync: capturable on the first call.  As its
// siblings, the job is checked before the context is looked at, each error with a message of its own.
int32_t orbit_surface_fragments(OrbitCtx *ctx, const OrbitSurfaceFragments *job, void *stream) {
    if (!job) return fail(ctx, ORBIT_E_INVALID, "surface_fragments: job is NULL");
    const OrbitSurfaceFragments &j = *job;
    if (j.flags & ~ORBIT_FRAGMENTS_CLEAR) return fail(ctx, ORBIT_E_INVALID, "surface_fragments: flags %#x", j.flags);
    if ((j.vertex_stride | j.position_offset | j.normal_offset | j.uv_offset | j.tangent_offset) & 3u)
        return fail(ctx, ORBIT_E_INVALID, "surface_fragments: vertex_stride %u, offsets %u / %u / %u / %u (multiples of 4)", j.vertex_stride,
                    j.position_offset, j.normal_offset, j.uv_offset, j.tangent_offset);
    if ((uint64_t)j.vertex_stride < (uint64_t)j.position_offset + 12u || (uint64_t)j.vertex_stride < (uint64_t)j.normal_offset + 4u ||
        (uint64_t)j.vertex_stride < (uint64_t)j.uv_offset + 8u || (uint64_t)j.vertex_stride < (uint64_t)j.tangent_offset + 4u)
        return fail(ctx, ORBIT_E_INVALID, "surface_fragments: vertex_stride %u below an attribute's end (position %u + 12, normal %u + 4, uv %u + 8, tangent %u + 4)",
                    j.vertex_stride, j.position_offset, j.normal_offset, j.uv_offset, j.tangent_offset);
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        return fail(ctx, ORBIT_E_INVALID, "surface_fragments: target %u x %u (1..%u each)", j.width, j.height, ORBIT_RASTER_MAX_DIM);
    if ((uint64_t)j.command_base + j.max_commands > ORBIT_VIS_MAX_COMMANDS)
        return fail(ctx, ORBIT_E_INVALID, "surface_fragments: command_base %u + max_commands %u > %u (24 bits of id)", j.command_base,
                    j.max_commands, ORBIT_VIS_MAX_COMMANDS);
    if (j.vertex_count > (1ull << 32))
        return fail(ctx, ORBIT_E_INVALID, "surface_fragments: vertex_count %llu > 2^32 (a global vertex is a u32)",
                    (unsigned long long)j.vertex_count);
    if (!j.visibility || !j.draw_commands || !j.meshlets || !j.bary || !j.triangle || !j.vertices || !j.entity_data)
        return fail(ctx, ORBIT_E_INVALID, "surface_fragments: NULL buffer");
    if (!j.world_pos && !j.normal && !j.tangent && !j.uv && !j.uv_grad && !j.material)
        return fail(ctx, ORBIT_E_INVALID, "surface_fragments: no output");
    if (j.uv_grad && !j.grad) return fail(ctx, ORBIT_E_INVALID, "surface_fragments: uv_grad needs grad");
    const void *const inputs[8] = {j.visibility, j.draw_commands, j.meshlets, j.bary, j.grad, j.triangle, j.vertices, j.entity_data};
    const void *const outputs[7] = {j.world_pos, j.normal, j.tangent, j.uv, j.uv_grad, j.material, j.stats};
    uintptr_t low_bits = 0;
    for (const void *in : inputs) low_bits |= (uintptr_t)in;
    for (const void *out : outputs) low_bits |= (uintptr_t)out;
    if (((uintptr_t)j.visibility & 7u) || ((uintptr_t)j.entity_data & 15u) || (low_bits & 3u))
        return fail(ctx, ORBIT_E_INVALID, "surface_fragments: visibility must be 8-B aligned, entity_data 16-B aligned, every other buffer 4-B aligned");
    for (const void *out : outputs)
        for (const void *in : inputs)
            if (out && out == in) return fail(ctx, ORBIT_E_INVALID, "surface_fragments: an output is an input (%p)", out);
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "surface_fragments: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_surface_fragments(j, ctx->num_cus, ctx->visibility_grid, ctx->status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch surface_fragments");
    return ORBIT_OK;
}

// The checks of an OrbitFragmentsShade, for orbit_fragments_shade and for orbit_fragments_shade_shadowed, which starts with
// one: each error with a message of its own behind the caller's prefix `who`
static int32_t check_fragments_shade(OrbitCtx *ctx, const char *who, const OrbitFragmentsShade &j) {
    const uint32_t known = ORBIT_SHADE_CLEAR | ORBIT_SHADE_FORCE_PER_LANE | ORBIT_SHADE_FORCE_STAGED;
    if (j.flags & ~known) return fail(ctx, ORBIT_E_INVALID, "%s: flags %#x", who, j.flags);
    if ((j.flags & ORBIT_SHADE_FORCE_PER_LANE) && (j.flags & ORBIT_SHADE_FORCE_STAGED))
        return fail(ctx, ORBIT_E_INVALID, "%s: ORBIT_SHADE_FORCE_PER_LANE and ORBIT_SHADE_FORCE_STAGED together", who);
    if (j.render_mode != 0u && j.render_mode != 8u) return fail(ctx, ORBIT_E_INVALID, "%s: render_mode %u (0 or 8)", who, j.render_mode);
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        return fail(ctx, ORBIT_E_INVALID, "%s: target %u x %u (1..%u each)", who, j.width, j.height, ORBIT_RASTER_MAX_DIM);
    if (j.cluster_count[0] == 0 || j.cluster_count[1] == 0 || j.cluster_count[2] == 0 || j.tile_size_px == 0)
        return fail(ctx, ORBIT_E_INVALID, "%s: cluster_count %u x %u x %u, tile_size_px %u (none may be 0)", who, j.cluster_count[0],
                    j.cluster_count[1], j.cluster_count[2], j.tile_size_px);
    if (j.cluster_count[2] > 32u) return fail(ctx, ORBIT_E_INVALID, "%s: cluster_count[2] %u > 32", who, j.cluster_count[2]);
    if ((uint64_t)j.cluster_count[0] * j.cluster_count[1] > (1ull << 31) / j.cluster_count[2])
        return fail(ctx, ORBIT_E_INVALID, "%s: %u x %u x %u clusters > 2^31", who, j.cluster_count[0], j.cluster_count[1], j.cluster_count[2]);
    if ((j.flags & ORBIT_SHADE_FORCE_STAGED) && j.tile_size_px % 8u != 0u)
        return fail(ctx, ORBIT_E_INVALID, "%s: ORBIT_SHADE_FORCE_STAGED needs tile_size_px %u %% 8 == 0", who, j.tile_size_px);
    if (!j.visibility || !j.world_pos || !j.normal || !j.material || !j.materials || !j.lights || !j.cluster_offset_image ||
        !j.light_index_buffer || !j.color)
        return fail(ctx, ORBIT_E_INVALID, "%s: NULL buffer", who);
    const void *const inputs[8] = {j.visibility, j.world_pos, j.normal, j.material, j.materials, j.lights, j.cluster_offset_image, j.light_index_buffer};
    const void *const outputs[3] = {j.color, j.lights_walked, j.stats};
    uintptr_t low_bits = 0;
    for (const void *in : inputs) low_bits |= (uintptr_t)in;
    for (const void *out : outputs) low_bits |= (uintptr_t)out;
    if ((((uintptr_t)j.visibility | (uintptr_t)j.cluster_offset_image) & 7u) || (((uintptr_t)j.materials | (uintptr_t)j.lights) & 15u) || (low_bits & 3u))
        return fail(ctx, ORBIT_E_INVALID, "%s: visibility and cluster_offset_image must be 8-B aligned, materials and lights 16-B aligned, every other buffer 4-B aligned", who);
    for (const void *out : outputs)
        for (const void *in : inputs)
            if (out && out == in) return fail(ctx, ORBIT_E_INVALID, "%s: an output is an input (%p)", who, out);
    return ORBIT_OK;
}

// A clearing launch (stats, and with ORBIT_SHADE_CLEAR color and lights_walked) and the shading launch
// (fragments_shade.hip).  No allocation, no scratch, no host sync: capturable on the first call.  As its siblings, the
// job is checked before the context is looked at, each error with a message of its own.
int32_t orbit_fragments_shade(OrbitCtx *ctx, const OrbitFragmentsShade *job, void *stream) {
    if (!job) return fail(ctx, ORBIT_E_INVALID, "fragments_shade: job is NULL");
    const OrbitFragmentsShade &j = *job;
    const int32_t checked = check_fragments_shade(ctx, "fragments_shade", j);
    if (checked != ORBIT_OK) return checked;
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "fragments_shade: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_fragments_shade(j, ctx->num_cus, ctx->visibility_grid, ctx->status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch fragments_shade");
    return ORBIT_OK;
}

// The same two launches with the shadow term served (fragments_shade_shadowed.hip): the base job's checks under this
// call's prefix, then the shadow fields'.
int32_t orbit_fragments_shade_shadowed(OrbitCtx *ctx, const OrbitFragmentsShadeShadowed *job, void *stream) {
    const char *who = "fragments_shade_shadowed";
    if (!job) return fail(ctx, ORBIT_E_INVALID, "%s: job is NULL", who);
    const OrbitFragmentsShadeShadowed &j = *job;
    const OrbitFragmentsShade &b = j.shade;
    const int32_t checked = check_fragments_shade(ctx, who, b);
    if (checked != ORBIT_OK) return checked;
    if (j.shadow_count > 0u) {
        if (!j.shadows || !j.shadow_maps) return fail(ctx, ORBIT_E_INVALID, "%s: shadow_count %u with shadows or shadow_maps NULL", who, j.shadow_count);
        if ((uintptr_t)j.shadows & 15u) return fail(ctx, ORBIT_E_INVALID, "%s: shadows must be 16-B aligned", who);
        if (j.shadow_resolution == 0u || j.shadow_resolution > ORBIT_RASTER_MAX_DIM)
            return fail(ctx, ORBIT_E_INVALID, "%s: shadow_resolution %u (1..%u)", who, j.shadow_resolution, ORBIT_RASTER_MAX_DIM);
        if ((uint64_t)j.shadow_map_count * j.shadow_resolution * j.shadow_resolution > (1ull << 31))
            return fail(ctx, ORBIT_E_INVALID, "%s: %u maps of %u x %u floats > 2^31", who, j.shadow_map_count, j.shadow_resolution, j.shadow_resolution);
    }
    const void *const inputs[10] = {b.visibility, b.world_pos, b.normal, b.material, b.materials, b.lights, b.cluster_offset_image,
                                    b.light_index_buffer, j.shadows, j.shadow_maps};
    const void *const outputs[6] = {b.color, b.lights_walked, b.stats, j.shadow_factor, j.cascade, j.shadow_stats};
    if (((uintptr_t)j.shadow_maps | (uintptr_t)j.shadow_factor | (uintptr_t)j.cascade | (uintptr_t)j.shadow_stats) & 3u)
        return fail(ctx, ORBIT_E_INVALID, "%s: shadow_maps, shadow_factor, cascade and shadow_stats must be 4-B aligned", who);
    for (const void *out : outputs)
        for (const void *in : inputs)
            if (out && out == in) return fail(ctx, ORBIT_E_INVALID, "%s: an output is an input (%p)", who, out);
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "%s: ctx is NULL", who);
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_fragments_shade_shadowed(j, ctx->num_cus, ctx->visibility_grid, ctx->status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch fragments_shade_shadowed");
    return ORBIT_OK;
}

// The same two launches with the sky light's term and the skybox served (fragments_shade_sky.hip).  The whole job, the
// base job's and the shadow fields' parts included, is checked by sky_common.h's sky_check, the function the mirror uses.
int32_t orbit_fragments_shade_sky(OrbitCtx *ctx, const OrbitFragmentsShadeSky *job, void *stream) {
    if (!job) return fail(ctx, ORBIT_E_INVALID, "fragments_shade_sky: job is NULL");
    const char *wrong = orbit::raster::sky_check(*job);
    if (wrong) return fail(ctx, ORBIT_E_INVALID, "fragments_shade_sky: %s", wrong);
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "fragments_shade_sky: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_fragments_shade_sky(*job, ctx->num_cus, ctx->visibility_grid, ctx->status, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch fragments_shade_sky");
    return ORBIT_OK;
}

// B1's shape: host only, no context
int32_t orbit_bloom_layout(uint32_t width, uint32_t height, OrbitBloomLayout *out) {
    if (!out) return fail(nullptr, ORBIT_E_INVALID, "bloom_layout: out is NULL");
    if (width == 0 || height == 0 || width > ORBIT_RASTER_MAX_DIM || height > ORBIT_RASTER_MAX_DIM)
        return fail(nullptr, ORBIT_E_INVALID, "bloom_layout: target %u x %u (1..%u each)", width, height, ORBIT_RASTER_MAX_DIM);
    if (out->max_levels > ORBIT_BLOOM_MAX_LEVELS) return fail(nullptr, ORBIT_E_INVALID, "bloom_layout: max_levels %u (1..%u, 0 = %u)", out->max_levels, ORBIT_BLOOM_MAX_LEVELS, ORBIT_BLOOM_MAX_LEVELS);
    orbit::raster::bloom_layout(width, height, out->max_levels ? out->max_levels : ORBIT_BLOOM_MAX_LEVELS, *out);
    return ORBIT_OK;
}

// One launch that starts the counters and one per level of the chain (bloom.hip).  No allocation, no scratch, no host
// sync: capturable on the first call.  As its siblings, the job is checked before the context is looked at.
int32_t orbit_bloom(OrbitCtx *ctx, const OrbitBloom *job, void *stream) {
    if (!job) return fail(ctx, ORBIT_E_INVALID, "bloom: job is NULL");
    const OrbitBloom &j = *job;
    if (j.flags & ~(ORBIT_BLOOM_FORCE_PER_LEVEL | ORBIT_BLOOM_FORCE_DIRECT)) return fail(ctx, ORBIT_E_INVALID, "bloom: flags %#x", j.flags);
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        return fail(ctx, ORBIT_E_INVALID, "bloom: target %u x %u (1..%u each)", j.width, j.height, ORBIT_RASTER_MAX_DIM);
    if (j.max_levels == 0 || j.max_levels > ORBIT_BLOOM_MAX_LEVELS) return fail(ctx, ORBIT_E_INVALID, "bloom: max_levels %u (1..%u)", j.max_levels, ORBIT_BLOOM_MAX_LEVELS);
    for (const float v : {j.threshold, j.soft_threshold, j.filter_radius})
        if (!(v >= 0.0f && v < INFINITY))
            return fail(ctx, ORBIT_E_INVALID, "bloom: threshold %g, soft_threshold %g, filter_radius %g (finite, not negative)", j.threshold, j.soft_threshold, j.filter_radius);
    if (!j.color || !j.mips) return fail(ctx, ORBIT_E_INVALID, "bloom: NULL buffer");
    if (((uintptr_t)j.color & 15u) || (((uintptr_t)j.mips | (uintptr_t)j.stats) & 3u))
        return fail(ctx, ORBIT_E_INVALID, "bloom: color must be 16-B aligned, mips and stats 4-B aligned");
    if ((const void *)j.mips == (const void *)j.color || (j.stats && ((const void *)j.stats == (const void *)j.color || (const void *)j.stats == (const void *)j.mips)))
        return fail(ctx, ORBIT_E_INVALID, "bloom: an output is an input or the other output (%p)", (const void *)j.mips);
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "bloom: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_bloom(j, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch bloom");
    return ORBIT_OK;
}

// A launch that starts the counters and one pass over the pixels (bloom.hip); as orbit_bloom otherwise.
int32_t orbit_post_process(OrbitCtx *ctx, const OrbitPostProcess *job, void *stream) {
    if (!job) return fail(ctx, ORBIT_E_INVALID, "post_process: job is NULL");
    const OrbitPostProcess &j = *job;
    if (j.flags & ~ORBIT_POST_BGRA) return fail(ctx, ORBIT_E_INVALID, "post_process: flags %#x", j.flags);
    if (j.render_mode != 0u && j.render_mode != 8u) return fail(ctx, ORBIT_E_INVALID, "post_process: render_mode %u (0 or 8)", j.render_mode);
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        return fail(ctx, ORBIT_E_INVALID, "post_process: target %u x %u (1..%u each)", j.width, j.height, ORBIT_RASTER_MAX_DIM);
    if (!(fabsf(j.exposure) < INFINITY) || !(fabsf(j.bloom_intensity) < INFINITY))
        return fail(ctx, ORBIT_E_INVALID, "post_process: exposure %g, bloom_intensity %g (finite)", j.exposure, j.bloom_intensity);
    if (!j.color) return fail(ctx, ORBIT_E_INVALID, "post_process: color is NULL");
    if (!j.ldr && !j.rgba8) return fail(ctx, ORBIT_E_INVALID, "post_process: ldr and rgba8 are both NULL");
    if ((((uintptr_t)j.color | (uintptr_t)j.ldr) & 15u) || (((uintptr_t)j.bloom | (uintptr_t)j.rgba8 | (uintptr_t)j.stats) & 3u))
        return fail(ctx, ORBIT_E_INVALID, "post_process: color and ldr must be 16-B aligned, bloom, rgba8 and stats 4-B aligned");
    const void *const inputs[2] = {j.color, j.bloom};
    const void *const outputs[3] = {j.ldr, j.rgba8, j.stats};
    for (int a = 0; a < 3; a++) {
        for (const void *in : inputs)
            if (outputs[a] && outputs[a] == in) return fail(ctx, ORBIT_E_INVALID, "post_process: an output is an input (%p)", in);
        for (int b = a + 1; b < 3; b++)
            if (outputs[a] && outputs[a] == outputs[b]) return fail(ctx, ORBIT_E_INVALID, "post_process: two outputs are one buffer (%p)", outputs[a]);
    }
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "post_process: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_post_process(j, ctx->num_cus, ctx->visibility_grid, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch post_process");
    return ORBIT_OK;
}

// A launch that starts the counters, then the SSAO launch, the blur and the fragment read (ssao.hip); as orbit_bloom
// otherwise.
int32_t orbit_ssao(OrbitCtx *ctx, const OrbitSsao *job, void *stream) {
    if (!job) return fail(ctx, ORBIT_E_INVALID, "ssao: job is NULL");
    const OrbitSsao &j = *job;
    if (j.flags != 0u) return fail(ctx, ORBIT_E_INVALID, "ssao: flags %#x", j.flags);
    if (j.screen_w == 0 || j.screen_h == 0 || j.screen_w > ORBIT_RASTER_MAX_DIM || j.screen_h > ORBIT_RASTER_MAX_DIM)
        return fail(ctx, ORBIT_E_INVALID, "ssao: screen %u x %u (1..%u each)", j.screen_w, j.screen_h, ORBIT_RASTER_MAX_DIM);
    if (j.ssao_w == 0 || j.ssao_h == 0 || j.ssao_w > j.screen_w || j.ssao_h > j.screen_h)
        return fail(ctx, ORBIT_E_INVALID, "ssao: ssao size %u x %u (1..%u x 1..%u, the screen)", j.ssao_w, j.ssao_h, j.screen_w, j.screen_h);
    if (j.noise_size == 0 || j.noise_size > ORBIT_SSAO_MAX_NOISE_SIZE || j.samples_size == 0 || j.samples_size > ORBIT_SSAO_MAX_SAMPLES_SIZE)
        return fail(ctx, ORBIT_E_INVALID, "ssao: noise_size %u (1..%u), samples_size %u (1..%u)", j.noise_size, ORBIT_SSAO_MAX_NOISE_SIZE, j.samples_size, ORBIT_SSAO_MAX_SAMPLES_SIZE);
    if (j.sample_count == 0 || j.sample_count > ORBIT_SSAO_MAX_SAMPLES) return fail(ctx, ORBIT_E_INVALID, "ssao: sample_count %u (1..%u)", j.sample_count, ORBIT_SSAO_MAX_SAMPLES);
    for (const float v : {j.min_radius, j.max_radius})
        if (!(v >= 0.0f && v < INFINITY)) return fail(ctx, ORBIT_E_INVALID, "ssao: min_radius %g, max_radius %g (finite, not negative)", j.min_radius, j.max_radius);
    if (!j.depth || !j.noise || !j.samples) return fail(ctx, ORBIT_E_INVALID, "ssao: NULL input");
    if (!j.raw && !j.blurred && !j.ao_pixel) return fail(ctx, ORBIT_E_INVALID, "ssao: raw, blurred and ao_pixel are all NULL");
    if ((j.blurred && !j.raw) || (j.ao_pixel && !j.blurred)) return fail(ctx, ORBIT_E_INVALID, "ssao: blurred needs raw and ao_pixel needs blurred");
    if ((((uintptr_t)j.depth | (uintptr_t)j.ao_pixel | (uintptr_t)j.samples) & 3u) || ((uintptr_t)j.noise & 1u) || ((uintptr_t)j.stats & 7u))
        return fail(ctx, ORBIT_E_INVALID, "ssao: depth, ao_pixel and samples must be 4-B aligned, noise 2-B, stats 8-B");
    const void *const inputs[3] = {j.depth, j.noise, j.samples};
    const void *const outputs[4] = {j.raw, j.blurred, j.ao_pixel, j.stats};
    for (int a = 0; a < 4; a++) {
        for (const void *in : inputs)
            if (outputs[a] && outputs[a] == in) return fail(ctx, ORBIT_E_INVALID, "ssao: an output is an input (%p)", in);
        for (int b = a + 1; b < 4; b++)
            if (outputs[a] && outputs[a] == outputs[b]) return fail(ctx, ORBIT_E_INVALID, "ssao: two outputs are one buffer (%p)", outputs[a]);
    }
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "ssao: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_ssao(j, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch ssao");
    return ORBIT_OK;
}

// E0's shape: host only, no context
int32_t orbit_env_map_layout(uint32_t sky_size, uint32_t irradiance_size, uint32_t prefiltered_size, uint32_t prefiltered_levels,
                             uint32_t brdf_size, OrbitEnvMapLayout *out) {
    if (!out) return fail(nullptr, ORBIT_E_INVALID, "env_map_layout: out is NULL");
    if (sky_size > ORBIT_ENV_MAX_SIZE || irradiance_size > ORBIT_ENV_MAX_SIZE || prefiltered_size > ORBIT_ENV_MAX_SIZE || brdf_size > ORBIT_ENV_MAX_SIZE)
        return fail(nullptr, ORBIT_E_INVALID, "env_map_layout: sizes %u, %u, %u, %u (each at most %u)", sky_size, irradiance_size, prefiltered_size, brdf_size, ORBIT_ENV_MAX_SIZE);
    if (sky_size != 0u && !orbit::raster::env_power_of_two(sky_size)) return fail(nullptr, ORBIT_E_INVALID, "env_map_layout: sky_size %u is not a power of two", sky_size);
    if (prefiltered_size != 0u && (prefiltered_levels == 0u || prefiltered_levels > ORBIT_ENV_MAX_LEVELS))
        return fail(nullptr, ORBIT_E_INVALID, "env_map_layout: prefiltered_levels %u (1..%u)", prefiltered_levels, ORBIT_ENV_MAX_LEVELS);
    orbit::raster::env_layout(sky_size, irradiance_size, prefiltered_size, prefiltered_levels, brdf_size, *out);
    return ORBIT_OK;
}

// A launch that starts the counters and the launches of the products asked for (env_map.hip).  No allocation, no scratch,
// no host sync: capturable on the first call.  As its siblings, the job is checked before the context is looked at; the
// checks are env_common.h's, the host mirror's too.
int32_t orbit_env_map(OrbitCtx *ctx, const OrbitEnvMap *job, void *stream) {
    if (!job) return fail(ctx, ORBIT_E_INVALID, "env_map: job is NULL");
    const char *wrong = orbit::raster::env_map_check(*job);
    if (wrong) return fail(ctx, ORBIT_E_INVALID, "env_map: %s", wrong);
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "env_map: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_env_map(*job, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch env_map");
    return ORBIT_OK;
}

// E4 of n directions: a clearing launch and one thread per direction; as orbit_env_map otherwise.
int32_t orbit_env_sample(OrbitCtx *ctx, const OrbitEnvSample *job, void *stream) {
    if (!job) return fail(ctx, ORBIT_E_INVALID, "env_sample: job is NULL");
    const char *wrong = orbit::raster::env_sample_check(*job);
    if (wrong) return fail(ctx, ORBIT_E_INVALID, "env_sample: %s", wrong);
    if (!ctx) return fail(nullptr, ORBIT_E_INVALID, "env_sample: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const hipError_t e = launch_env_sample(*job, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "launch env_sample");
    return ORBIT_OK;
}

} // extern "C"
