/*
 * orbit_abi_ext.h — entry points of the engine BEYOND the drop-in core of orbit_abi.h.
 *
 * orbit_abi.h holds what a maintainer needs to swap the bodies of the reference's cull passes
 * (src/passes/draw_gen.rs:239-435,456-566, src/passes/cluster.rs:368-591): the context, entity_cull,
 * meshlet_cull, depth_reduce, the three light-cluster stages, the shard range and the RCCL gather.  Everything here is
 * optional on top of that — same conventions, same status codes, same context:
 *   - the mesh-shading path (task-shader records instead of draw commands),
 *   - several views in one call / one launch (orbit_cull_views),
 *   - derived meshlet streams (an MI355X-side re-layout of the static meshlet buffer),
 *   - several pyramids in one launch,
 *   - the late half of a frame with its independent chains side by side (orbit_frame_late),
 *   - the sharded engine: the shard cull, the record list, its device-side exchanges (HIP-IPC stores; RCCL all-gather)
 *     and the expansion of a gathered list,
 *   - the measurement hook of bench.py,
 *   - the scene update: model and normal matrices computed on the device from entity transforms,
 *   - cull statistics: every entity and meshlet of a cull counted by the first test that rejected it,
 *   - cluster statistics: the uncapped light counts of the cluster chain, by cluster and by depth sample.
 * A build that only needs the drop-in includes orbit_abi.h alone; liborbit_cull.so exports both sets.
 */
#ifndef ORBIT_ABI_EXT_H
#define ORBIT_ABI_EXT_H

#include "orbit_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The visible list of the sharded engine (no reference counterpart: the reference is single-GPU) — the ONE format a rank
 * sends: the ordered survivor list at RECORD granularity.  Buffer layout: {u32 records; u32 survivors} @0, entries[] @8,
 * one entry per dispatch record, in record order; bit b of `mask` set = meshlet `meshlet_offset + b` of entity
 * `entity_index` is drawn (mask 0: a record without a survivor).  12 B per record: never more than 3/8 of a byte per
 * dispatched meshlet on the xGMI links (28-B commands: 66 MB over one link at N = 2 of BASELINE config 5, slower than
 * not sharding) — and an entry's position is its record's index, so the evaluation launch writes the list itself: no
 * count, no scan, no launch behind it.  (Rounds 2-5 also carried an 8-B {meshlet, entity} item per survivor; retired
 * in round 6 — twice the bytes at config 5 and an emit launch to make it.) */
#define ORBIT_VISIBLE_HEADER 8u
typedef struct OrbitVisibleRecord {
    uint32_t entity_index;
    uint32_t meshlet_offset;
    uint32_t mask; /* should-draw ballot of the record's (up to) 32 meshlets (meshlet_cull.comp:207-213) */
} OrbitVisibleRecord;
ORBIT_STATIC_ASSERT(sizeof(OrbitVisibleRecord) == 12, "visible record is 12 B");

/* Mesh-shading path.  When mesh shading is on, the renderer
 * skips create_meshlet_draw_commands and culls meshlets in the task shader,
 * one workgroup per MeshletDispatch record
 * (shaders/forward/forward_depth_prepass.task:115-257, forward.task, fed by the
 * dispatch buffer of create_meshlet_dispatch_command).  This entry point
 * computes what those workgroups compute — per record the EmitMeshTasksEXT
 * count and the MeshTaskPayload — into `task_records` (dispatch_capacity
 * entries, dispatch order), so that a task shader only has to load its record.
 * Same decision as orbit_meshlet_cull; as in the task shaders, lanes past a
 * record's meshlet_count report `visible` in the pass-2 visibility words.
 * bufs->draw_commands_buffer / draw_capacity are not used (may be NULL / 0). */
int32_t orbit_meshlet_task_cull(OrbitCtx *ctx, const OrbitGpuCullInfo *cull_info,
                                const OrbitMeshletCullBufs *bufs,
                                OrbitMeshTaskRecord *task_records, void *stream);

/* ------------------------------------------------------------------------ */
/* Several views in one call.  A frame of the reference culls the same scene */
/* for the early forward pass and for each of the four shadow cascades        */
/* (forward.rs:286-403, shadow_renderer.rs:391-403) — independent culls,      */
/* each a chain of five short, latency-bound launches on a scene of a few     */
/* thousand entities.  orbit_cull_views puts them into ONE chain: every       */
/* kernel of the path takes all views at once (blockIdx.y = view, parameter   */
/* blocks from a table; the streaming evaluations are grouped by occlusion    */
/* pass and projection type, so the early pass + four cascades are two        */
/* launches), each view on its own scan scratch — 6 launches instead of 25.   */
/* Every view's outputs are exactly those of orbit_entity_cull +              */
/* orbit_meshlet_cull on its buffers.  Meant for scenes whose culls are bound */
/* by launch latency; a 50 M-meshlet view belongs in the single-view calls    */
/* (their kernels keep the parameters in scalar registers).                   */
/* ------------------------------------------------------------------------ */
typedef struct OrbitCullView {
    const OrbitGpuCullInfo *cull_info; /* HOST, 400 B: this view's CullInfo::to_gpu */
    OrbitEntityCullBufs entity;        /* its own dispatch buffer (and bitset / pyramid in the occlusion passes) */
    OrbitMeshletCullBufs meshlet;      /* meshlet_dispatch_buffer = entity.meshlet_dispatch_buffer */
    uint32_t entity_draw_count;
    uint32_t skip_meshlet_stage;       /* != 0: mesh-shading path, only the dispatch records are produced */
} OrbitCullView;
#define ORBIT_MAX_CULL_VIEWS 8
/* The views must not share output buffers; visibility buffers written by two views (occlusion_pass 2) must differ. */
int32_t orbit_cull_views(OrbitCtx *ctx, const OrbitCullView *views, uint32_t count, void *stream);
/* One launch instead of the chain.  A call whose views all have both stages and between 1 and 16 384 entity-draws
 * each — every scene the reference itself can hold: MAX_INSTANCE_COUNT = 100 000 instances, MAX_MESHLET_COUNT = 256 k
 * (src/scene.rs:303, src/assets/mod.rs:202), a cull being one clear and two dispatches there (draw_gen.rs:283-322) —
 * runs as ONE persistent launch per (occlusion pass, projection type) among its views: entity test, record append,
 * meshlet test and ordered command append hand over inside the launch (orbit_amd/csrc/cull_fused.hip), which is what
 * such a cull costs: its dependent memory round trips once, not once per launch.  count = 1 is the single cull
 * (create_draw_commands, draw_gen.rs:239-322).  The outputs are those of the chain bit for bit; the path reads the 32-B
 * Meshlet buffer (a bound stream is not consulted) and can be captured into a graph like every other call.
 * OrbitCaps.cull_path overrides the choice.  Returns how many views this context has culled that way. */
uint64_t orbit_ctx_fused_culls(const OrbitCtx *ctx);

/* ------------------------------------------------------------------------ */
/* Derived meshlet streams — an MI355X-side copy of the static meshlet       */
/* buffer in the layout the cull streams best.                               */
/*                                                                           */
/* GpuAssets::add_mesh writes a mesh's Meshlet records into meshlet_buffer   */
/* once (src/assets/mod.rs:441-445); every frame's meshlet cull then streams */
/* all 32 B of every dispatched meshlet, although the decision reads 22 of   */
/* them (bounding sphere, cone, material index) — 20 and a quarter once the  */
/* material's alpha_mode is known — and only the ~10 % that survive need the */
/* rest (vertex_offset, data_offset, counts) for their command.  A stream    */
/* object keeps derived arrays for a range of the buffer (37.65 B of HBM per */
/* meshlet on top of the buffer itself):                                     */
/*   spheres 16 B, cones 4 B, material indices 2 B — what every meshlet's    */
/*     test reads;                                                           */
/*   alpha classes, 2 bits — the material's alpha_mode, so that the test     */
/*     reads no material index (set_materials below);                        */
/*   command words 12 B — gathered per survivor by                           */
/*     orbit_expand_visible_records;                                         */
/*   counts 2 B + 1 link bit — the command chain: compute_meshlets /         */
/*     add_mesh lay a mesh's meshlets out so that a meshlet's data_offset is */
/*     its predecessor's plus the predecessor's vertex_count +               */
/*     ceil(3 * triangle_count / 4) words, with one vertex_offset per        */
/*     submesh (src/assets/mesh.rs:309-316, assets/mod.rs:413-416); the link */
/*     bit records where that holds, and the emit launch then derives a      */
/*     survivor's offsets from one gathered base per chain and the counts    */
/*     streamed at 2 B per meshlet instead of gathering 12 B per survivor.   */
/*     Meshlets laid out any other way are served by gathers: the chain is   */
/*     an acceleration, never an assumption.                                 */
/* With a stream bound to a context, orbit_meshlet_cull / _task_cull /       */
/* _cull_visible_records / orbit_cull_shard calls whose bufs->meshlet_buffer */
/* is the pointer the stream was last updated from evaluate occlusion passes */
/* 0 and 2 from the arrays and write no survivor payload, and                */
/* orbit_expand_visible_records gathers 12 B instead of touching the         */
/* survivors' Meshlets.  Results are bit-identical                           */
/* to the plain path (every test of tests/test_gpu_parity.py runs all ways). */
/* orbit_cull_views applies the same rule per view.  Pass 1 (list-driven     */
/* gathers) and any call with another meshlet_buffer pointer read the        */
/* Meshlet buffer as before.                                                 */
/*                                                                           */
/*   create   arrays for global meshlet indices [first_meshlet,              */
/*            first_meshlet + capacity), capacity <= 2^27 (device memory:    */
/*            37.65 B x capacity, zero-filled)                               */
/*   update   re-derives [first, first + count) from `meshlet_buffer` (same  */
/*            global indexing as bufs->meshlet_buffer), enqueued on `stream`;*/
/*            call it wherever the renderer writes meshlets (add_mesh) —     */
/*            meshlets changed without an update are culled from stale data  */
/*            (caps.validate_streams / orbit_meshlet_stream_validate find    */
/*            that).  Culls read the HULL of the ranges updated from the     */
/*            same buffer pointer; meshlets inside it that no update reached */
/*            are empty (zero) meshlets.  An update from another pointer     */
/*            starts the range over.                                         */
/*   set_materials  derives every meshlet's alpha class from                 */
/*            material_buffer[material_index].alpha_mode (material_count     */
/*            entries; indices beyond it and modes > 2 are looked up at cull */
/*            time as before) and remembers the pointer: later updates       */
/*            derive the classes of their range from it, and culls whose     */
/*            bufs->material_buffer is that pointer read the classes instead */
/*            of the material indices — provided NO meshlet of the stream    */
/*            needs the look-up; a stream that holds one keeps evaluating    */
/*            through the indices.  Call it wherever the renderer writes     */
/*            materials (add_material, assets/mod.rs:520); NULL forgets.     */
/*            An upload-time call: unless `stream` is being captured into a  */
/*            graph it returns once the derivation has run (it waits for its */
/*            own launch on `stream`), so that which evaluation kernel the   */
/*            next cull takes never depends on timing.  The pointer is       */
/*            dereferenced on the device by every later update: call         */
/*            set_materials(NULL) (or with the new buffer) BEFORE the         */
/*            material buffer is freed or re-created.                        */
/*   validate compares the stream with `meshlet_buffer` (and the classes     */
/*            with `material_buffer`, may be NULL) over the readable range   */
/*            and latches ORBIT_E_STALE in the context's status on any       */
/*            difference.                                                    */
/*   bind     NULL unbinds; one stream can be bound to any number of         */
/*            contexts of its device, and cannot be destroyed while bound    */
/*            (ORBIT_E_INVALID; destroying a context unbinds).  The stream   */
/*            must cover every meshlet the culls dispatch: a meshlet outside */
/*            its range is not read from it (the lane evaluates zeros, the   */
/*            command carries zeros) and ORBIT_E_RANGE is latched            */
/* ------------------------------------------------------------------------ */
typedef struct OrbitMeshletStream OrbitMeshletStream;
int32_t orbit_meshlet_stream_create(OrbitCtx *ctx, uint64_t first_meshlet, uint64_t capacity,
                                    OrbitMeshletStream **out_stream);
int32_t orbit_meshlet_stream_update(OrbitCtx *ctx, OrbitMeshletStream *ms, const void *meshlet_buffer,
                                    uint64_t first, uint64_t count, void *stream);
int32_t orbit_meshlet_stream_set_materials(OrbitCtx *ctx, OrbitMeshletStream *ms, const void *material_buffer,
                                           uint32_t material_count, void *stream);
int32_t orbit_meshlet_stream_validate(OrbitCtx *ctx, OrbitMeshletStream *ms, const void *meshlet_buffer,
                                      const void *material_buffer, void *stream);
/* The entity stage's share of the same idea.  GpuAssets::add_mesh also writes the mesh's 128-B MeshInfo
 * (src/assets/mod.rs:18-28, types.glsl:123-141) once, and every frame's entity cull then fetches that whole line per
 * entity-draw for 28 bytes of it: the bounding sphere, lod_count and the chosen MeshLod.  update_meshes derives a 32-B
 * side entry {sphere, lod_count, mesh_lods[0]} for meshes [first_mesh, first_mesh + count) of `mesh_info_buffer`
 * (32 B of device memory per mesh; the table — at least 2^20 entries, zero-filled — is allocated by the first call);
 * entity culls (orbit_entity_cull[_range], orbit_cull_views, orbit_cull_shard) of contexts the stream is bound to whose
 * bufs->mesh_info_buffer is that pointer read the entry instead of the MeshInfo, and the MeshInfo itself only where a
 * LOD other than 0 is picked or where no update reached the mesh.  Same results bit for bit.  Call it wherever the
 * renderer writes mesh infos; an update from another buffer pointer starts the table over, NULL forgets it;
 * orbit_meshlet_stream_validate (and every entity cull of a context with validate_streams) compares the table with the
 * buffer it was derived from (ORBIT_E_STALE).  orbit_ctx_mesh_side_culls: entity culls that were handed the table. */
int32_t orbit_meshlet_stream_update_meshes(OrbitCtx *ctx, OrbitMeshletStream *ms, const void *mesh_info_buffer,
                                           uint32_t first_mesh, uint32_t count, void *stream);
uint64_t orbit_ctx_mesh_side_culls(const OrbitCtx *ctx);
int32_t orbit_meshlet_stream_destroy(OrbitMeshletStream *ms);
int32_t orbit_ctx_bind_meshlet_stream(OrbitCtx *ctx, OrbitMeshletStream *ms);
/* Calls this context has served from a bound stream so far — meshlet culls of passes 0 and 2 (each such view of
 * orbit_cull_views' launch chain counts) and orbit_expand_visible_records (tests and integration checks: a call whose
 * meshlet_buffer is not the stream's source silently takes the plain path).  Views that orbit_cull_views runs as its
 * ONE launch (up to 16 384 entity-draws, OrbitCaps.cull_path) read the 32-B Meshlet buffer and do not count —
 * orbit_ctx_fused_culls counts those — and neither ORBIT_E_RANGE nor the validate_streams check applies to them
 * (a context created with validate_streams keeps the chain for that reason). */
uint64_t orbit_ctx_meshlet_stream_culls(const OrbitCtx *ctx);
/* ... of which evaluated from the alpha classes (no material index read): culls whose material buffer the classes
 * mirror, of a stream known to hold no meshlet of class 3 — known when set_materials returns (it waits for its
 * derivation unless it is being captured); after an update that derives classes, once that launch has finished
 * (polled, never waited for: culls enqueued before that read the material indices). */
uint64_t orbit_ctx_meshlet_class_culls(const OrbitCtx *ctx);
/* ... of which decided per block of 32 meshlets: every orbit_meshlet_stream_update also derives, for each 32-aligned
 * block of global meshlet indices it touches, a bound of the block's spheres (centre, radius of the centres, largest
 * radius; 32 B per block), and orbit_meshlet_cull of occlusion pass 0, perspective projection, canonical arithmetic,
 * from a stream with alpha classes decides a meshlet from its 4-byte cone word and its block's bound wherever that
 * verdict is certain, and evaluates it as before where it is not: the outputs are the same, bit for bit.  On by
 * default; orbit_ctx_set_block_cull(ctx, 0) — or ORBIT_BLOCK_CULL=0 in the environment when the context is created —
 * keeps the per-meshlet evaluation.  orbit_meshlet_stream_validate also checks every sphere of the buffer against
 * its block's bound (ORBIT_E_STALE). */
uint64_t orbit_ctx_block_culls(const OrbitCtx *ctx);
int32_t orbit_ctx_set_block_cull(OrbitCtx *ctx, uint32_t enable);
/* Tests: the per-block evaluation's launch takes at most `max_workgroups` workgroups (of four waves; a wave takes its
 * tiles one after another, so a small grid gives every wave a sequence of tiles from a small scene).  0, the default,
 * leaves the grid as the library sizes it.  The outputs do not depend on the grid; no other launch is touched. */
int32_t orbit_ctx_set_block_cull_grid(OrbitCtx *ctx, uint32_t max_workgroups);
/* Tests: every launch of orbit_raster_depth and orbit_raster_visibility, whichever flags pick the kernel, and the
 * clearing launch in front of it take at most `max_workgroups` workgroups (of four waves; a wave takes its commands one
 * after another, so under a cap of c wave k takes commands k, k + 4c, ... of even a short list).  0, the default,
 * restores the resident grid.  The outputs do not depend on the grid; no other launch is touched. */
int32_t orbit_ctx_set_raster_grid(OrbitCtx *ctx, uint32_t max_workgroups);
/* Tests: every launch of the one-launch cull behind orbit_cull_views (either arithmetic profile, every tile shape) takes
 * at most `max_workgroups` workgroups per view (of four waves; work is handed out by tickets, so under a cap of 1 or 2 a
 * wave runs many tiles in a row and one workgroup runs every entity chunk).  Read when the launch is enqueued: a
 * prepared call follows it too.  0, the default, restores the sized grid.  The outputs do not depend on the grid; the
 * shard launch and every other launch are not touched. */
int32_t orbit_ctx_set_fused_grid(OrbitCtx *ctx, uint32_t max_workgroups);
/* Tests: the strided launches of the visibility buffer's six readers — orbit_visibility_resolve's clear and its tile
 * walk, orbit_visibility_compact's clear and its mark, orbit_visibility_surface's clear and its tile walk (and
 * orbit_visibility_surface_drawn's), orbit_surface_fragments' clear and its tile walk, orbit_fragments_shade's clear and
 * its tile walk, orbit_fragments_shade_shadowed's clear and its tile walk — and orbit_post_process' pass over the pixels
 * (a thread per pixel, workgroup b taking pixels 256 b, 256 (b + c), ...) take at most
 * `max_workgroups` workgroups (of four waves; a wave takes its 8 x 8 tiles one after another, so under a cap of c wave g
 * takes tiles g, g + 4c, ... of even a small target).  Read when the call is enqueued: a captured launch carries its
 * grid.  0, the default, restores num_cus * 8.  The outputs do not depend on the grid; the compaction's scan, totals and
 * emit, sized per chunk of commands, and every other launch are not touched. */
int32_t orbit_ctx_set_visibility_grid(OrbitCtx *ctx, uint32_t max_workgroups);
/* Tests: the bounds of blocks [first_block, first_block + count) (block = global meshlet index / 32) into the HOST
 * array `out`, 32 B each: {float centre[3], centre_radius, max_radius; uint32_t valid, pad[2]}.  Waits for `stream`. */
int32_t orbit_meshlet_stream_block_bounds(OrbitCtx *ctx, OrbitMeshletStream *ms, uint64_t first_block, uint64_t count,
                                          void *out, void *stream);
/* Tests: the derived arrays of meshlets [first, first + count) (inside the stream's range, else ORBIT_E_CAPACITY) into
 * HOST arrays, every one of which must be given: per meshlet `sphere` 16 B, `cone` 4 B, `mat` 2 B, `cmd` 12 B and `cnt`
 * 2 B; and the words of `link`, `cls0`, `cls1` (4 B) and the entries of `base32` (8 B) that hold those meshlets — words
 * first / 32 .. (first + count - 1) / 32 of global meshlet indices, as the bounds above are addressed.  Bits of such a
 * word that belong to meshlets outside the stream's range mean nothing.  Waits for `stream`; launches nothing. */
typedef struct OrbitMeshletStreamArrays {
    void *sphere, *cone, *mat, *cmd, *cnt, *link, *cls0, *cls1, *base32;
} OrbitMeshletStreamArrays;
ORBIT_STATIC_ASSERT(sizeof(OrbitMeshletStreamArrays) == 72, "stream arrays block is nine pointers");
int32_t orbit_meshlet_stream_read_arrays(OrbitCtx *ctx, OrbitMeshletStream *ms, uint64_t first, uint64_t count,
                                         const OrbitMeshletStreamArrays *out, void *stream);

/* One pyramid of a batch.  `depth_row_pitch` = texels per row of the depth buffer (0 = screen_width: tightly
 * packed); exactly one of `pyramid` (packed chain) and `levels` (HOST array of the mip_levels the pyramid has for
 * this screen size, orbit_depth_pyramid_desc; each entry holds DEVICE pointers) is non-NULL. */
typedef struct OrbitDepthReduceItem {
    const float *depth;
    uint32_t screen_width, screen_height;
    uint32_t depth_row_pitch;
    uint32_t _pad;
    float *pyramid;
    const OrbitDepthPyramidLevel *levels;
} OrbitDepthReduceItem;
ORBIT_STATIC_ASSERT(sizeof(OrbitDepthReduceItem) == 40, "depth-reduce item is 40 B");
#define ORBIT_MAX_PYRAMID_BATCH 8
/* update_multiple_depth_pyramids::<C> (draw_gen.rs:569-628): `count` (<= 8) pyramids — the main view's and the
 * shadow cascades' — in ONE launch pair instead of C x 12 dispatches; pyramids of different sizes may be mixed.
 * Also the entry point for pyramids made of separate per-mip images (`levels`) and pitched depth buffers. */
int32_t orbit_depth_reduce_multi(OrbitCtx *ctx, const OrbitDepthReduceItem *items, uint32_t count, void *stream);

/* ------------------------------------------------------------------------ */
/* The late half of a frame as ONE call with its independent chains side by  */
/* side.  Between "the depth buffer exists" and the forward pass the renderer */
/* records (src/app.rs:1151-1212): the depth pyramid(s) and the late          */
/* (VisibilityWrite) culls of render_depth_prepass (forward.rs:371-403,      */
/* draw_gen.rs:510-566), render_shadows' cascade culls (shadow_renderer.rs:  */
/* 391-403: occlusion_pass 0, no pyramid) and compute_clusters (cluster.rs:  */
/* 368-397).  Three chains that share no output: on scenes of the            */
/* reference's own size each is a handful of dependent, latency-bound        */
/* launches on a device that is 95 % idle during any one of them — issued    */
/* one after the other on one stream they cost their sum.                    */
/* orbit_frame_late runs                                                     */
/*   A  pyramids (orbit_depth_reduce_multi) -> late_views (orbit_cull_views), */
/*   B  cascade_views (orbit_cull_views) and                                  */
/*   C  clusters (orbit_compute_clusters)                                     */
/* side by side: the chain with the most dependent launches stays on         */
/* `stream`, the other two run on two streams of the context, forked behind  */
/* whatever `stream` holds when                                              */
/* the call is made and joined into `stream` before it returns — events only, */
/* no host wait: the call can be captured into a graph, and work enqueued    */
/* on `stream` behind it sees all three chains' outputs.  Outputs are byte   */
/* for byte those of the serial calls.  Every group is optional (count 0 /   */
/* NULL); late + cascade views together at most ORBIT_MAX_CULL_VIEWS (each   */
/* view on its own scan scratch, OrbitCaps.max_views); everything is         */
/* validated before anything is enqueued.  The chains' inputs must be        */
/* complete in `stream` order when the call is made (the depth buffer, last  */
/* frame's visibility words); their output buffers must differ.  The two     */
/* side streams are created by the first call that needs them.               */
/* ------------------------------------------------------------------------ */
typedef struct OrbitClusterFrame { /* orbit_compute_clusters' arguments */
    const OrbitMarkActivePush *push;
    const OrbitClusterCullInfo *info;
    const float *depth;
    const OrbitLightData *lights;
    uint32_t *tile_depth_slice_mask;
    OrbitClusterDepthBounds *depth_bounds;
    void *unique_cluster_buffer;
    void *light_index_buffer;
    uint32_t *cluster_offset_image;
    uint32_t index_capacity;
    uint32_t light_index_capacity;
} OrbitClusterFrame;
ORBIT_STATIC_ASSERT(sizeof(OrbitClusterFrame) == 80, "cluster frame block is 80 B");
typedef struct OrbitFrameLate {
    const OrbitDepthReduceItem *pyramids; /* chain A, first: the late views' pyramids (NULL / 0: none) */
    const OrbitCullView *late_views;      /* chain A, then: the VisibilityWrite culls that read them */
    const OrbitCullView *cascade_views;   /* chain B */
    const OrbitClusterFrame *clusters;    /* chain C (NULL: none) */
    uint32_t pyramid_count, late_view_count, cascade_view_count, _pad;
} OrbitFrameLate;
ORBIT_STATIC_ASSERT(sizeof(OrbitFrameLate) == 48, "frame-late descriptor is 48 B");
int32_t orbit_frame_late(OrbitCtx *ctx, const OrbitFrameLate *frame, void *stream);

/* ------------------------------------------------------------------------ */
/* Measurement hook (bench.py).  While enabled, every orbit_meshlet_cull     */
/* records a HIP event pair on the caller's stream around the op's dominant  */
/* kernel (the streaming meshlet evaluation); profile_read waits for the     */
/* recorded pairs and returns their mean duration.  Never on by default.     */
/* `enable` = n > 0 times every n-th call (an event pair costs a few          */
/* microseconds of stream time: it keeps the next launch from being          */
/* prefetched), 0 switches the hook off.                                     */
/* ------------------------------------------------------------------------ */
int32_t orbit_ctx_profile(OrbitCtx *ctx, int32_t enable);
/* The pairs are created on first use (a hipEventCreate and a first record each: host time inside the region that is
 * being timed); _reserve creates `pairs` of them up front, each recorded once on `stream`. */
int32_t orbit_ctx_profile_reserve(OrbitCtx *ctx, uint32_t pairs, void *stream);
int32_t orbit_ctx_profile_read(OrbitCtx *ctx, float *avg_ms, uint32_t *launches);

/* ------------------------------------------------------------------------ */
/* The sharded engine — ONE product.  Per rank and frame:    */
/*   1. orbit_cull_shard: the rank's entity range through both stages; ends  */
/*      in the record list of its shard (what it sends) and, optionally, the */
/*      28-B MeshletDrawCommandBuffer of its shard (what it draws from);     */
/*   2. the rank-ordered all-gather of the record lists — every rank's list  */
/*      is in canonical order and the shards are contiguous in entity order, */
/*      so the concatenation in rank order IS the single-GPU sequence:       */
/*      orbit_exchange_list (direct xGMI stores into the peers' IPC-mapped   */
/*      buffers, counts and completion signalled on the device; default) or  */
/*      orbit_allgather_list (north_star's RCCL all-gather; the fallback);   */
/*      neither reads a count on the host, both are capturable;              */
/*   3. where a GPU wants the WHOLE scene's commands: orbit_expand_visible_   */
/*      records of the gathered list (needs the meshlet buffer there).       */
/*                                                                           */
/*   orbit_meshlet_cull_visible_records  orbit_meshlet_cull, but              */
/*       `record_buffer` ({records, survivors} @0, OrbitVisibleRecord[] @8,  */
/*       record_capacity entries) replaces bufs->draw_commands_buffer /      */
/*       draw_capacity (not used).  Entry i is dispatch record i with its    */
/*       should-draw ballot, written by the evaluation launch itself (ONE    */
/*       launch for the whole cull; the header by its last workgroup):       */
/*       records = the dispatched records, survivors = the set bits of all   */
/*       of them.  ORBIT_E_CAPACITY is latched if the records do not fit     */
/*       (the header holds the clamped count, the first record_capacity      */
/*       entries are written);                                               */
/*   orbit_expand_visible_records  record list -> MeshletDrawCommandBuffer   */
/*       in list order (= the canonical order), the command words read from  */
/*       `meshlet_buffer` under global indices (or from a bound stream that  */
/*       mirrors it).  What is written depends on the list and on            */
/*       draw_capacity only.  With S the set bits of all the list's masks    */
/*       (an entry's mask may be 0: a list can be far longer than what it    */
/*       expands to, and draw_capacity may be sized for the survivors): the  */
/*       header is min(S, draw_capacity), the first min(S, draw_capacity)    */
/*       commands follow in list order and nothing behind them is written;   */
/*       ORBIT_E_CAPACITY is latched if and only if S > draw_capacity or the */
/*       list holds more than 64 M records (it is cut there).  No read-back, */
/*       no synchronisation: capturable.  The gathered header's second word  */
/*       is not maintained by the exchanges and not read here.               */
/* ------------------------------------------------------------------------ */
int32_t orbit_meshlet_cull_visible_records(OrbitCtx *ctx, const OrbitGpuCullInfo *cull_info,
                                           const OrbitMeshletCullBufs *bufs, void *record_buffer,
                                           uint32_t record_capacity, void *stream);
int32_t orbit_expand_visible_records(OrbitCtx *ctx, const void *record_buffer, const void *meshlet_buffer,
                                     void *draw_commands_buffer, uint32_t draw_capacity, void *stream);
/* Both products of ONE evaluation: the record list (as orbit_meshlet_cull_visible_records: what the rank sends) and the
 * rank's own MeshletDrawCommandBuffer in bufs->draw_commands_buffer / draw_capacity (as orbit_meshlet_cull: what it
 * draws from, "each rank keeps its shard and issues its own indirect draws") — the evaluation writes the
 * list, scan + emit of the same ballots follow; cheaper than the list followed by orbit_expand_visible_records of it. */
int32_t orbit_meshlet_cull_records_and_commands(OrbitCtx *ctx, const OrbitGpuCullInfo *cull_info,
                                                const OrbitMeshletCullBufs *bufs, void *record_buffer,
                                                uint32_t record_capacity, void *stream);
/* A rank's whole cull as ONE call — orbit_entity_cull_range over [draw_first, draw_first + draw_count) followed by
 * orbit_meshlet_cull_visible_records (with_commands == 0) or orbit_meshlet_cull_records_and_commands (!= 0) on the
 * records it appended (meshlet_bufs->meshlet_dispatch_buffer must be entity_bufs->meshlet_dispatch_buffer) — and, for
 * occlusion pass 0 and at most 65 536 entity-draws, ONE launch for the entity test, the record append, the meshlet
 * test and the record list (+ the emit launch when the commands are wanted): a shard's step is mostly its launches'
 * fixed costs, and this is what a 1/8 shard of BASELINE config 5 pays them once for instead of four times.  Other
 * passes and larger ranges run the two calls' launch chain; the outputs are the same bit for bit either way
 * (OrbitCaps.cull_path = 1 forces the chain).  orbit_ctx_shard_culls: calls that took the one launch. */
int32_t orbit_cull_shard(OrbitCtx *ctx, const OrbitGpuCullInfo *cull_info, const OrbitEntityCullBufs *entity_bufs,
                         uint32_t draw_first, uint32_t draw_count, const OrbitMeshletCullBufs *meshlet_bufs,
                         void *record_buffer, uint32_t record_capacity, uint32_t with_commands, void *stream);
uint64_t orbit_ctx_shard_culls(const OrbitCtx *ctx);

/* ------------------------------------------------------------------------ */
/* The exchange by direct stores (one node, one process per GPU, peers       */
/* reachable over xGMI): the bulk data does not go through RCCL at all —     */
/* every rank copies its list straight into every peer's output buffer at    */
/* the rank-ordered position, the offsets computed on the device from counts */
/* that travelled the same way.  Nothing waits for the host.                 */
/* ------------------------------------------------------------------------ */

#define ORBIT_P2P_HANDLE_BYTES 64 /* hipIpcMemHandle_t */
#define ORBIT_P2P_MAX_WORLD 16
#define ORBIT_P2P_CTRL_BYTES 1024 /* a rank's control block of orbit_exchange_list (orbit_p2p_alloc'ed, zero-filled) */

/* Exchange buffers: FINE-GRAINED device memory of this context's GPU that peers may map (hipExtMallocWithFlags,
 * hipDeviceMallocFinegrained: what a peer stores into it over xGMI — list segments, and the control words a waiting
 * kernel of this device polls while it runs — is visible here without a kernel boundary in between; ordinary device
 * memory is coherent between devices only at kernel boundaries).
 * orbit_p2p_alloc returns the pointer and an opaque handle to send to the other
 * processes (any host channel: a file, torch.distributed.all_gather_object);
 * orbit_p2p_open maps a peer's buffer into this process (hipIpcOpenMemHandle;
 * dmabuf IPC: HSA_ENABLE_IPC_MODE_LEGACY=0).  The buffers stay caller-visible
 * for the life of the context; *_close / *_free undo the calls. */
int32_t orbit_p2p_alloc(OrbitCtx *ctx, uint64_t bytes, void **out_ptr,
                        uint8_t out_handle[ORBIT_P2P_HANDLE_BYTES]);
int32_t orbit_p2p_free(OrbitCtx *ctx, void *ptr);
int32_t orbit_p2p_open(OrbitCtx *ctx, const uint8_t handle[ORBIT_P2P_HANDLE_BYTES], void **out_peer_ptr);
int32_t orbit_p2p_close(OrbitCtx *ctx, void *peer_ptr);

/* The whole exchange on the device — no collective, no host in the step, capturable into a graph.
 *   local_list   {u32 count @0 | header_bytes | items of `stride` bytes}: a record list (header 8, stride 12); any
 *                header / stride that are multiples of 4 work (a MeshletDrawCommandBuffer: 4 / 28)
 *   out_buffers  HOST array of `world` device pointers: rank r's output buffer as mapped in THIS process
 *                (out_buffers[rank] = this rank's own buffer); same layout as local_list, `out_capacity` items
 * Counts and completion travel like the lists themselves, as stores into the peers' IPC-mapped memory: every rank
 * owns a CONTROL BLOCK (ORBIT_P2P_CTRL_BYTES from orbit_p2p_alloc, which
 * zero-fills it; mapped by every peer with orbit_p2p_open).  One call enqueues two launches on `stream`: a scatter that
 * first stores this rank's count into every peer's block, waits (on the device, bounded: ORBIT_E_TIMEOUT) for the counts
 * of the ranks before it, copies the list to its rank-ordered position in every rank's `out_buffers[r]` and then raises
 * "done" in that rank's block; and a one-workgroup launch that waits until every rank's count and "done" for this
 * exchange have arrived and writes the header {total, 0 ..} of this rank's own buffer.  Work enqueued behind the call
 * reads the complete list.  Exchanges are numbered by a counter in the control block (all ranks count in step), so a
 * captured graph replays correctly.  Every rank must call it the same number of times, with the same `world`; a
 * rank's out buffer must not be rewritten (by the next exchange into the same buffer) while its consumers still read
 * it: alternate two (buffer, control block) pairs, as bench.py does.
 *   ctrl_buffers  HOST array of `world` device pointers: rank r's control block as mapped in THIS process */
int32_t orbit_exchange_list(OrbitCtx *ctx, const void *local_list, uint32_t rank, uint32_t world,
                            void *const *out_buffers, void *const *ctrl_buffers, uint32_t out_capacity,
                            uint32_t header_bytes, uint32_t stride, void *stream);

/* ------------------------------------------------------------------------ */
/* north_star's transport — "an RCCL all-gather of the compacted visible    */
/* list" — with no host in it either.  RCCL send/recv take message sizes as  */
/* host arguments (orbit_gather_visible of orbit_abi.h reads them back); a   */
/* collective of a FIXED size needs no size: every rank contributes its     */
/* whole list buffer as a segment {count | header | segment_capacity items},*/
/* ONE ncclAllGather moves all segments to all ranks, and one launch         */
/* compacts them — the counts are read on the device — into the contiguous  */
/* rank-ordered list {total | header | items}: byte for byte what            */
/* orbit_exchange_list delivers.  Nothing is read back, no stream is         */
/* synchronised, both steps can be captured into a graph.  The price is the */
/* segments' slack on the links (capacity - count items per rank): nothing  */
/* for the record list, which holds an entry per dispatch record and is as  */
/* long as the shard's entity stage made it — the list this is meant for    */
/* (28-B commands or 8-B items sized for the worst case would move mostly    */
/* slack: those keep orbit_gather_visible*).                                 */
/*   local_list        this rank's list; the buffer holds at least           */
/*                     header_bytes + stride * segment_capacity bytes        */
/*   segment_capacity  items per segment, the same on every rank             */
/*   segments          world x (header_bytes + stride * segment_capacity)    */
/*                     bytes of device memory: the collective's receive      */
/*                     buffer (caller-owned like every buffer)               */
/*   out_list          {total | header | out_capacity items}; a total beyond */
/*                     out_capacity latches ORBIT_E_CAPACITY                 */
/* orbit_compact_segments is the second half alone, for callers that issue   */
/* the collective themselves (bench.py: torch.distributed's                  */
/* all_gather_into_tensor, which is ncclAllGather on ROCm).                  */
/* ------------------------------------------------------------------------ */
int32_t orbit_allgather_list(OrbitCtx *ctx, void *nccl_comm, uint32_t rank, uint32_t world, const void *local_list,
                             uint32_t segment_capacity, void *segments, void *out_list, uint32_t out_capacity,
                             uint32_t header_bytes, uint32_t stride, void *stream);
int32_t orbit_compact_segments(OrbitCtx *ctx, const void *segments, uint32_t world, uint32_t segment_capacity,
                               void *out_list, uint32_t out_capacity, uint32_t header_bytes, uint32_t stride,
                               void *stream);

/* ------------------------------------------------------------------------ */
/* Scene update on the device.  SceneData::update_scene (src/scene.rs:404-492) */
/* builds every entity's EntityData on the CPU each frame: the model matrix    */
/* Mat4::from_scale_rotation_translation of its Transform, the normal matrix   */
/* the upper 3x3 of model.inverse().transpose() (identity elsewhere), and     */
/* uploads all 128-B rows again.  This entry point computes the rows from the */
/* 40-B transforms instead, bit for bit what the host mirror's               */
/* EntityData::entity_gpu_data gives (scalar cofactor inverse, the products   */
/* in the host's association, correctly rounded 1/det, f32 denormals kept).   */
/*   dense   instance_indices == NULL: entity_data[i] for i < count; count >  */
/*           entity_capacity is refused (ORBIT_E_INVALID)                     */
/*   sparse  instance_indices != NULL (DEVICE, count u32): only the rows      */
/*           entity_data[instance_indices[i]] are written, every other byte   */
/*           stays as it was.  An index >= entity_capacity writes nothing and */
/*           latches ORBIT_E_RANGE (orbit_ctx_status); the other rows are     */
/*           still written.  With duplicate indices one of the writers wins,  */
/*           which one is unspecified.                                        */
/* transforms is a DEVICE array of `count` entries (4-B alignment suffices;   */
/* 16 B is faster), entity_data a DEVICE array of entity_capacity rows,       */
/* 16-B aligned.  count == 0 is ORBIT_OK with no launch; a NULL transforms or */
/* entity_data with count > 0 is ORBIT_E_INVALID.  Stream semantics are those */
/* of the other entry points.  The call allocates nothing, uses no scratch    */
/* and never synchronises the host, so it can be captured into a graph on its */
/* very first call.  OrbitCaps.arith_profile does not apply: this arithmetic  */
/* is the reference's host (glam on the CPU), the same in both profiles.      */
/* ------------------------------------------------------------------------ */
typedef struct OrbitEntityTransform { /* scene.rs Transform, field order of OrbitHostEntity */
    float position[3];
    float orientation[4]; /* quaternion x, y, z, w; not required to be normalised */
    float scale[3];
} OrbitEntityTransform;
ORBIT_STATIC_ASSERT(sizeof(OrbitEntityTransform) == 40, "EntityTransform is 40 B");

/* entity_data[i] (or entity_data[instance_indices[i]]) = EntityData::entity_gpu_data() of transforms[i], i < count */
int32_t orbit_scene_update_entities(OrbitCtx *ctx, const OrbitEntityTransform *transforms,
                                    const uint32_t *instance_indices, uint32_t count,
                                    OrbitEntityData *entity_data, uint32_t entity_capacity, void *stream);

/* ------------------------------------------------------------------------ */
/* The whole scene update on the device.  orbit_scene_update_entities above  */
/* leaves two thirds of SceneData::update_scene (src/scene.rs:404-492) on    */
/* the CPU: the EntityDrawBuffer, the LightData[] array with its shadow      */
/* indices, and the instance order of the transforms themselves.             */
/* orbit_scene_update builds all of it from two DEVICE arrays in ENTITY      */
/* order: one 48-B descriptor and one 40-B transform per entity.  It is      */
/* three ordered stream compactions (entities with a mesh, with a light,     */
/* directional lights that cast shadows); order comes from prefix sums,      */
/* never from atomics, and the outputs equal the host mirror's               */
/* SceneData::update_scene byte for byte.  With e running over the entities: */
/*   mesh   mesh_index != ORBIT_SCENE_NONE.  r = the mesh-bearing entities   */
/*          before e: entity_data[r] = entity_gpu_data() of transforms[e]    */
/*          (the bits of orbit_scene_update_entities), draw r = {r,          */
/*          mesh_index, visibility_offset} (mesh_index is copied, not        */
/*          validated), instance_of_entity[e] = r.  The draw buffer's count  */
/*          word is min(draws, instance_capacity).                           */
/*   light  light_kind <= 2.  l = the light-bearing entities before e:       */
/*          light_data[l] = light_gpu_data(luminance_cutoff): colour,        */
/*          intensity and light_type copied; Sky: the two map indices;       */
/*          Directional: direction = -(orientation * (0, 0, -1)) in glam's   */
/*          mul_vec3 expression (its zero products kept), inner_radius =     */
/*          light_param; Point: position, inner_radius = light_param,        */
/*          outer_radius = sqrt(intensity / cutoff), both correctly rounded; */
/*          every other field zero.  light_of_entity[e] = l.                 */
/*   shadow Directional with bit 0 of light_flags.  s = such lights before   */
/*          e: shadow_data_index = shadow_index_base + s (u32 arithmetic),   */
/*          shadow_orientations[s] = the four orientation words as bits.     */
/*          Every other light's shadow_data_index is 0xFFFFFFFF.             */
/*   A light_kind in 3 .. 0xFFFFFFFE is none the host can produce: the       */
/*   entity counts as having no light and ORBIT_E_RANGE is latched.          */
/* Capacities: a row whose rank is >= its capacity is dropped, nothing       */
/* behind a capacity is written and ORBIT_E_CAPACITY is latched; ranks and   */
/* shadow_data_index are assigned as if every row fitted, and *counts and    */
/* the two maps hold the uncapped values.  shadow_capacity applies only with */
/* a shadow_orientations array.  Output rows behind the counts are not       */
/* touched.  Every pointer is a DEVICE pointer, 4-B aligned (entities and    */
/* transforms: 16 B is faster), entity_data 16-B aligned.                    */
/*   entity_count == 0  ORBIT_OK: the count word and *counts are written as  */
/*                      zeros (where given), nothing else                    */
/*   ORBIT_E_INVALID    NULL update; with entity_count > 0 a NULL entities,  */
/*                      transforms, entity_data, entity_draw_buffer or       */
/*                      light_data; a misaligned pointer                     */
/*   ORBIT_E_CAPACITY   entity_count > caps.max_entities                     */
/* The entity cull reads the draw count from the buffer on the device and    */
/* clamps it with its entity_draw_count argument: pass the entity count (an  */
/* upper bound) and a device-built draw buffer feeds the cull with no        */
/* read-back.  The call enqueues two launches on the stream, allocates       */
/* nothing (its scan scratch is part of the context), never synchronises the */
/* host and can be captured into a graph on its first call; calls on one     */
/* context must be ordered against each other like the culls.                */
/* OrbitCaps.arith_profile does not apply.                                   */
/* Cost beyond the buffers: every workgroup of 256 entities sums the 12-B    */
/* totals of the workgroups in front of it, so the call reads about          */
/* 6 B * (entity_count / 256)^2 from L2 on top: 3.5 MB at 195 313 entities,  */
/* 100 MB at one million (a quarter of the call's own traffic there), and    */
/* growing with the square beyond.  It is meant for scenes of up to about a  */
/* million entities; larger ones still give the right bytes, more slowly.    */
/* ------------------------------------------------------------------------ */
#define ORBIT_SCENE_NONE 0xFFFFFFFFu
typedef struct OrbitSceneEntity { /* one per ENTITY, entity order, DEVICE; 48 B */
    uint32_t mesh_index;        /* MeshHandle slot, ORBIT_SCENE_NONE = no mesh (scene.rs:420) */
    uint32_t visibility_offset; /* first meshlet-visibility word: the host allocator's (scene.rs:422-431) */
    uint32_t light_kind;        /* 0 Sky, 1 Directional, 2 Point, ORBIT_SCENE_NONE = no light */
    uint32_t light_flags;       /* bit 0: cast_shadows */
    float light_color[3], light_intensity;
    float light_param;          /* Directional: angular_size, Point: inner_radius */
    uint32_t irradiance_map_index, prefiltered_map_index; /* Sky */
    uint32_t _pad;
} OrbitSceneEntity;
ORBIT_STATIC_ASSERT(sizeof(OrbitSceneEntity) == 48, "SceneEntity is 48 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitSceneEntity, light_kind) == 8, "light_kind @8");
ORBIT_STATIC_ASSERT(offsetof(OrbitSceneEntity, light_color) == 16, "light_color @16");
ORBIT_STATIC_ASSERT(offsetof(OrbitSceneEntity, light_param) == 32, "light_param @32");
typedef struct OrbitSceneCounts { uint32_t draws, lights, shadows, entities; } OrbitSceneCounts; /* uncapped */
ORBIT_STATIC_ASSERT(sizeof(OrbitSceneCounts) == 16, "SceneCounts is 16 B");
typedef struct OrbitSceneUpdate {
    const OrbitSceneEntity *entities;       /* entity_count entries */
    const OrbitEntityTransform *transforms; /* entity_count entries, ENTITY order */
    OrbitEntityData *entity_data;           /* instance_capacity rows, 16-B aligned */
    void *entity_draw_buffer;               /* {u32 count; OrbitEntityDraw[instance_capacity]} */
    OrbitLightData *light_data;             /* light_capacity rows */
    float *shadow_orientations;             /* 4 floats per shadow command, shadow_capacity rows; may be NULL */
    uint32_t *instance_of_entity;           /* entity_count words, NONE where no mesh; may be NULL */
    uint32_t *light_of_entity;              /* entity_count words, NONE where no light; may be NULL */
    OrbitSceneCounts *counts;               /* may be NULL */
    uint32_t entity_count, instance_capacity, light_capacity, shadow_capacity;
    float luminance_cutoff;
    uint32_t shadow_index_base;             /* MAX_SHADOW_COMMANDS * frame_index (scene.rs:461) */
} OrbitSceneUpdate;
ORBIT_STATIC_ASSERT(sizeof(OrbitSceneUpdate) == 96, "SceneUpdate is 96 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitSceneUpdate, counts) == 64, "counts @64");
ORBIT_STATIC_ASSERT(offsetof(OrbitSceneUpdate, entity_count) == 72, "entity_count @72");
ORBIT_STATIC_ASSERT(offsetof(OrbitSceneUpdate, luminance_cutoff) == 88, "luminance_cutoff @88");

/* draws, EntityData rows, LightData rows, shadow orientations and both maps of SceneData::update_scene; see above */
int32_t orbit_scene_update(OrbitCtx *ctx, const OrbitSceneUpdate *update, void *stream);

/* ------------------------------------------------------------------------ */
/* Cull statistics.  The cull returns survivors only (dispatch records,     */
/* draw commands, visibility bits); orbit_cull_stats counts, on the device, */
/* what it did with every entity-draw and every meshlet: each is counted    */
/* ONCE, by the first reason in the shaders' own order of evaluation        */
/* (shaders/entity_cull.comp:106-230, meshlet_cull.comp:108-214).           */
/*                                                                          */
/* Contract: *stats is OVERWRITTEN with what                                */
/*     orbit_entity_cull(ctx, cull_info, ebufs, entity_draw_count, stream)  */
/*     orbit_meshlet_cull(ctx, cull_info, mbufs, stream)                    */
/* would do if they were enqueued NEXT on the same stream, with the same    */
/* arguments and under the context's current dispatch_size and             */
/* arith_profile (the classes are the cull's own in either profile).       */
/* CALL IT BEFORE THE CULL: passes 1 and 2 rewrite the visibility words the */
/* counts depend on.  The call reads what those two calls read, except      */
/* mbufs->meshlet_dispatch_buffer: the meshlet stage's records are worked   */
/* out from the entity stage itself (the pointer must still be non-NULL,    */
/* as for the cull).  It writes *stats and nothing else — no visibility     */
/* word, no dispatch or draw buffer, no latched status (only its own        */
/* argument errors are returned).  The meshlets are read from the caller's  */
/* 32-B Meshlet buffer; a bound meshlet stream holds the same bits, so the  */
/* counts hold for every cull path.                                         */
/* Served: caps.dispatch_size 32, occlusion passes 0, 1 and 2, both         */
/* projections.  Refused like the culls refuse (same checks, same codes):   */
/*   ORBIT_E_INVALID  dispatch_size != 32, projection_type > 1, stats NULL  */
/*                    or not 8-B aligned, NULL bufs / cull_info            */
/*   ORBIT_E_PLANES   cull_plane_count > 12                                 */
/*   ORBIT_E_MISSING  a buffer a cull requires is NULL (pyramid, visibility */
/*                    buffers of the occlusion passes)                      */
/*   ORBIT_E_CAPACITY entity_draw_count > caps.max_entities, dispatch       */
/*                    capacity > caps.max_dispatches                        */
/* The call allocates nothing and never synchronises the host: a graph can  */
/* capture it on its first call.  The counters are cleared on the stream    */
/* and summed with 64-bit device atomics: the result is deterministic.      */
/*                                                                          */
/* Invariants (every counter is uncapped: dispatch_capacity and            */
/* draw_capacity cut the cull's OUTPUT, not these counts):                 */
/*   entities == entity_skipped_prev_invisible + entity_frustum_culled +    */
/*               entity_occlusion_culled + entity_drawn_in_early_pass +     */
/*               entity_drawn                                               */
/*   sum(lod_drawn) == entity_drawn                                         */
/*   meshlets == meshlet_skipped_prev_invisible + meshlet_frustum_culled +  */
/*               meshlet_cone_culled + meshlet_occlusion_culled +           */
/*               meshlet_alpha_filtered + meshlet_drawn_in_early_pass +     */
/*               meshlet_drawn                                              */
/*   records == the workgroup_count_x the entity cull writes                */
/*              (records > dispatch_capacity: the cull drops the rest and   */
/*              latches ORBIT_E_CAPACITY)                                   */
/*   meshlet_drawn == the cull's command count whenever neither capacity is */
/*              exceeded (meshlet_drawn > draw_capacity: commands dropped)  */
/* ------------------------------------------------------------------------ */
typedef struct OrbitCullStats {
    /* entity stage: entity-draws evaluated (gID < min(in-buffer count, 256 * ceil(entity_draw_count / 256)), :106) */
    uint64_t entities;
    uint64_t entity_skipped_prev_invisible; /* pass 1: not visible last frame (:123) */
    uint64_t entity_frustum_culled;         /* a cull plane (:137-144) */
    uint64_t entity_occlusion_culled;       /* pass 2: the HiZ test (:147-191) */
    uint64_t entity_drawn_in_early_pass;    /* pass 2: visible now and last frame, no meshlet occlusion (:198-200) */
    uint64_t entity_drawn;                  /* records emitted for it (:203) */
    uint64_t records;                       /* MeshletDispatch records of the drawn entities: ceil(meshlets / 32) each */
    uint64_t reserved0;
    uint64_t lod_drawn[8];                  /* entity_drawn by the LOD whose MeshLod was used (min(lod, lod_count - 1)) */
    /* meshlet stage, over the meshlets of the records above */
    uint64_t meshlets;
    uint64_t meshlet_skipped_prev_invisible; /* pass 1 with meshlet occlusion: not visible last frame (:137) */
    uint64_t meshlet_frustum_culled;         /* a cull plane (:139-146) */
    uint64_t meshlet_cone_culled;            /* the normal cone (:148-158) */
    uint64_t meshlet_occlusion_culled;       /* pass 2 with meshlet occlusion: the HiZ test (:161-205) */
    uint64_t meshlet_alpha_filtered;         /* visible, but (1 << alpha_mode) & alpha_mode_flag == 0 (:207) */
    uint64_t meshlet_drawn_in_early_pass;    /* pass 2 with meshlet occlusion, alpha mode not in noskip_alphamode, visible
                                                last frame: drawn by pass 1 (:210-213; the alpha flag is not consulted) */
    uint64_t meshlet_drawn;                  /* a draw command (:215) */
    uint64_t reserved1[8];
} OrbitCullStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitCullStats) == 256, "CullStats is 256 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitCullStats, records) == 48, "records @48");
ORBIT_STATIC_ASSERT(offsetof(OrbitCullStats, lod_drawn) == 64, "lod_drawn @64");
ORBIT_STATIC_ASSERT(offsetof(OrbitCullStats, meshlets) == 128, "meshlets @128");
ORBIT_STATIC_ASSERT(offsetof(OrbitCullStats, meshlet_drawn) == 184, "meshlet_drawn @184");
ORBIT_STATIC_ASSERT(offsetof(OrbitCullStats, reserved1) == 192, "reserved1 @192");

/* *stats (DEVICE, 8-B aligned) = the counts of orbit_entity_cull + orbit_meshlet_cull with these arguments; see above */
int32_t orbit_cull_stats(OrbitCtx *ctx, const OrbitGpuCullInfo *cull_info, const OrbitEntityCullBufs *ebufs,
                         uint32_t entity_draw_count, const OrbitMeshletCullBufs *mbufs, OrbitCullStats *stats,
                         void *stream);

/* ------------------------------------------------------------------------ */
/* Cluster statistics.  The cluster chain returns capped results only: an   */
/* (offset, count) image whose counts stop at 256 (light_culling.comp:135), */
/* a compacted list and a light_count header that stop at the capacities.   */
/* orbit_cluster_stats counts, on the device, what the chain finds before   */
/* any cap, and what the forward pass will loop over.                       */
/*                                                                          */
/* Contract: *stats is OVERWRITTEN with what                                */
/*     orbit_compute_clusters(ctx, push, info, depth, lights, ...)          */
/* computes for these inputs.  No counter depends on index_capacity or      */
/* light_index_capacity: every counter is uncapped.  push and info are host */
/* pointers; depth, lights and stats are device pointers, stats 8-B aligned.*/
/* The call reads only the chain's inputs and writes *stats and nothing     */
/* else — no mask, bounds, compacted list, index buffer, image or latched   */
/* status — so it may come before or after the chain.  It uses no scratch   */
/* of the context: on a stream beside the chain (orbit_frame_late runs the  */
/* chain on side streams) it does not race with it.  It allocates nothing   */
/* and never synchronises the host: a graph can capture it on its first     */
/* call.  The counters are cleared on the stream and summed with 64-bit     */
/* device atomics: the result is deterministic.  The cluster passes are     */
/* canonical in either arith_profile: one build serves both.                */
/* Refused exactly like orbit_compute_clusters refuses the same push, info, */
/* depth and lights (same checks, same codes), and also:                   */
/*   ORBIT_E_INVALID  stats NULL or not 8-B aligned                         */
/*                                                                          */
/* Definitions.  A depth sample is depth[(py W + px) samples + s]; its      */
/* slice is mark_active's, depth_slice(z_near / d) (orbit_device.h); it is  */
/* in the grid iff slice < cz, and then its cluster is (px/ts, py/ts,       */
/* slice).  A cluster is active iff it holds an in-grid sample (the         */
/* compaction's clusters, uncut).  count(c) = the lights < global_light_    */
/* count for which is_light_in_cluster(aabb(c), l) holds (:108-133; a       */
/* non-point light is in every cluster), uncapped; capped(c) =              */
/* min(count(c), 256).  The classes of count(c):                            */
/*   [0] 0, [1] 1-16, [2] 17-64, [3] 65-256, [4] > 256.                     */
/*                                                                          */
/* Invariants:                                                              */
/*   samples == samples_outside_grid + sum(samples_by_lights)               */
/*   active_clusters == sum(clusters_by_lights)                             */
/*   light_refs - light_indices = the lights lost to the 256 cap; it is 0   */
/*              iff clusters_by_lights[4] == 0                              */
/*   with index_capacity >= active_clusters, the chain's compaction header  */
/*              is active_clusters and its light_count header is            */
/*              light_indices (the index capacity the frame needs)          */
/* ------------------------------------------------------------------------ */
typedef struct OrbitClusterStats {
    uint64_t samples;              /* W * H * depth_buffer_sample_count */
    uint64_t samples_outside_grid; /* slice >= cz: the forward pass's imageLoad misses, no clustered light (clear 0.0) */
    uint64_t active_clusters;      /* the compaction's count, uncut by index_capacity */
    uint64_t light_refs;           /* sum over active clusters of count(c) */
    uint64_t light_indices;        /* sum over active clusters of capped(c): the chain's light_count header */
    uint64_t max_cluster_lights;   /* max of count(c), or 0 */
    uint64_t sample_light_refs;    /* sum over in-grid samples of capped(their cluster): the trips of forward.frag:371's
                                      loop, each sample shaded once at its own depth (MSAA: per sample, an upper bound) */
    uint64_t reserved0;
    uint64_t clusters_by_lights[5]; /* active clusters per class of count(c) */
    uint64_t reserved1[3];
    uint64_t samples_by_lights[5];  /* in-grid samples per class of their cluster's count(c) */
    uint64_t reserved2[11];
} OrbitClusterStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitClusterStats) == 256, "ClusterStats is 256 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitClusterStats, sample_light_refs) == 48, "sample_light_refs @48");
ORBIT_STATIC_ASSERT(offsetof(OrbitClusterStats, clusters_by_lights) == 64, "clusters_by_lights @64");
ORBIT_STATIC_ASSERT(offsetof(OrbitClusterStats, samples_by_lights) == 128, "samples_by_lights @128");
ORBIT_STATIC_ASSERT(offsetof(OrbitClusterStats, reserved2) == 168, "reserved2 @168");

/* *stats (DEVICE, 8-B aligned) = the uncapped counts of orbit_compute_clusters for these inputs; see above */
int32_t orbit_cluster_stats(OrbitCtx *ctx, const OrbitMarkActivePush *push, const OrbitClusterCullInfo *info,
                            const float *depth, const OrbitLightData *lights, OrbitClusterStats *stats, void *stream);

/* ------------------------------------------------------------------------ */
/* Geometry bounds on the device.  The 20 bytes of a Meshlet that decide    */
/* the frustum, cone and HiZ tests (bounding sphere, snorm8 cone axis and   */
/* cutoff) and the 40 bytes of a MeshInfo that decide the entity test       */
/* (sphere, AABB) are functions of the vertex positions.  A renderer that   */
/* moves vertices on the device (skinning, morphing, a streamed LOD)        */
/* refits them here instead of reading the vertex buffer back.              */
/*                                                                          */
/* orbit_meshlet_bounds: for every selected meshlet m the device decodes    */
/* the meshlet as the mesh shader does (forward_depth_prepass.mesh:44,55:   */
/* global vertex = vertex_offset + meshlet_data[data_offset + local], u8    */
/* corners from byte (data_offset + vertex_count) * 4) and computes         */
/* meshopt_computeClusterBounds as the host mirror restates it              */
/* (orbit_amd/host/orbit_assets.cpp compute_meshlet_bounds): the Ritter     */
/* sphere of the corners of the non-degenerate triangles, the sphere of     */
/* their unit normals as the cone axis, sqrt(1 - mindp^2), snorm8 with the  */
/* cutoff rounded up.  Contract: the bytes equal the host mirror's, bit for */
/* bit, for EVERY input (degenerate triangles, NaN, infinities, denormals,  */
/* overflowing squares, triangle and vertex counts up to 255).  One thing   */
/* is canonical: a float that is NaN is written as the quiet NaN 0x7FC00000 */
/* by the device and by the host export alike (the sign and payload of an   */
/* x86-64 NaN depend on the host compiler's operand order, not on the       */
/* algorithm).  It writes                                                   */
/* bytes 0..19 of record m unless ORBIT_BOUNDS_KEEP_RECORDS is set, and the */
/* whole bounds to full[i] if `full` is given; bytes 20..31 of a record and */
/* every unselected record are never written.  A meshlet selected twice by  */
/* an index list is computed twice, to the same bytes.                      */
/*                                                                          */
/* Range checks, on the device: a selected meshlet whose index is >=        */
/* meshlet_capacity, whose data reaches beyond meshlet_data_words, that     */
/* names a vertex >= vertex_count (the sum is taken in 64 bits) or has a    */
/* corner >= its own vertex_count is left unwritten, its `full` row is      */
/* zero-filled and ORBIT_E_RANGE is latched (orbit_ctx_status); the other   */
/* meshlets are still written.  Nothing out of range is read.               */
/*   ORBIT_E_INVALID  job NULL; meshlets, meshlet_data or vertices NULL     */
/*                    with meshlet_count > 0; vertex_stride <               */
/*                    position_offset + 12; stride or offset no multiple of */
/*                    4; meshlets not 16-B aligned, another pointer not 4-B */
/*                    aligned; KEEP_RECORDS without `full`; unknown flags   */
/* A count of 0 is ORBIT_OK without a launch.  The call allocates nothing,  */
/* uses no scratch and never synchronises the host: a graph can capture it  */
/* on its first call.  caps.arith_profile and dispatch_size do not apply.   */
/*                                                                          */
/* THE RECORDS ARE THE SOURCE OF THE DERIVED STREAMS: after a refit, call   */
/* orbit_meshlet_stream_update of the same range before the next cull that  */
/* reads a bound stream (caps.validate_streams finds a forgotten one:       */
/* ORBIT_E_STALE).  Likewise orbit_meshlet_stream_update_meshes after       */
/* orbit_mesh_bounds when a mesh side table is bound.                       */
/* ------------------------------------------------------------------------ */
typedef struct OrbitMeshletBoundsFull { /* meshopt::Bounds, 48 B */
    float center[3], radius;
    float cone_apex[3], cone_cutoff;
    float cone_axis[3];
    int8_t cone_axis_s8[3], cone_cutoff_s8;
} OrbitMeshletBoundsFull;
ORBIT_STATIC_ASSERT(sizeof(OrbitMeshletBoundsFull) == 48, "MeshletBoundsFull is 48 B");

#define ORBIT_BOUNDS_KEEP_RECORDS 1u /* flags: compute, write `full` only */
typedef struct OrbitMeshletBoundsJob { /* HOST block, 96 B; every pointer a DEVICE pointer */
    void *meshlets;                  /* OrbitMeshlet[meshlet_capacity], global indexing */
    const uint32_t *meshlet_data;    /* meshlet_data_buffer: vertex indices at data_offset, then the u8 corners */
    const void *vertices;            /* position i = 3 floats at i * vertex_stride + position_offset */
    const uint32_t *meshlet_indices; /* NULL: the range [first_meshlet, first_meshlet + meshlet_count);
                                        else meshlet_count global indices (first_meshlet not used) */
    OrbitMeshletBoundsFull *full;    /* NULL, or row i = the i-th selected meshlet */
    uint64_t first_meshlet, meshlet_count, meshlet_capacity, meshlet_data_words, vertex_count;
    uint32_t vertex_stride, position_offset, flags, _pad;
} OrbitMeshletBoundsJob;
ORBIT_STATIC_ASSERT(sizeof(OrbitMeshletBoundsJob) == 96, "MeshletBoundsJob is 96 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitMeshletBoundsJob, first_meshlet) == 40, "first_meshlet @40");
ORBIT_STATIC_ASSERT(offsetof(OrbitMeshletBoundsJob, vertex_stride) == 80, "vertex_stride @80");

/* sphere, cone axis and cutoff of the selected meshlets from the vertex buffer; see above */
int32_t orbit_meshlet_bounds(OrbitCtx *ctx, const OrbitMeshletBoundsJob *job, void *stream);

/* orbit_mesh_bounds: per range, assets::compute_mesh_bounds (gltf_loader.rs:480-506) of the vertices              */
/* [first_vertex, first_vertex + vertex_count): the AABB, then the sphere — the AABB's centre, the radius through   */
/* the farthest vertex.  Writes bounding_sphere[0..3], aabb_min[0..2] and aabb_max[0..2] of mesh_infos[mesh_index]; */
/* the two w words and bytes 48..127 stay untouched.  Contract: equal to the host mirror as float VALUES for finite */
/* positions (+0 and -0 compare equal: fmin / fmax leave a zero's sign open); an empty range gives the host's +inf, */
/* -inf, a NaN centre and radius 0.  A range reaching beyond vertex_count, or a mesh_index >= mesh_capacity, writes */
/* nothing for that mesh and latches ORBIT_E_RANGE.  Ranges naming the same mesh are not ordered.  Large ranges are */
/* cut over several workgroups; the scratch is the context's, so calls on one context are ordered by their stream   */
/* (use one stream per context for this call).  ORBIT_E_INVALID for NULL ranges, vertices or mesh_infos with a      */
/* count above 0, a stride below position_offset + 12, a stride or offset no multiple of 4, a pointer not 4-B       */
/* aligned (mesh_infos: 16 B).  No allocation, no host synchronisation: capturable on its first call.               */
typedef struct OrbitMeshBoundsRange { /* DEVICE, 12 B */
    uint32_t mesh_index, first_vertex, vertex_count;
} OrbitMeshBoundsRange;
ORBIT_STATIC_ASSERT(sizeof(OrbitMeshBoundsRange) == 12, "MeshBoundsRange is 12 B");
int32_t orbit_mesh_bounds(OrbitCtx *ctx, const OrbitMeshBoundsRange *ranges, uint32_t range_count,
                          const void *vertices, uint64_t vertex_count, uint32_t vertex_stride, uint32_t position_offset,
                          OrbitMeshInfo *mesh_infos, uint32_t mesh_capacity, void *stream);

/* ------------------------------------------------------------------------ */
/* Depth prepass on the device.  What turns the early cull's                */
/* MeshletDrawCommandBuffer into the depth buffer that orbit_depth_reduce   */
/* and the late cull read is the reference's depth prepass                  */
/* (forward_depth_prepass.mesh / .vert plus fixed-function raster,          */
/* forward.rs:300-356).  An Instinct part has no rasteriser:                */
/* orbit_raster_depth is that pass in compute.  It consumes the draw        */
/* commands exactly as orbit_meshlet_cull wrote them ({u32 count;           */
/* OrbitMeshletDrawCommand[]}; the count is read ON THE DEVICE and clamped  */
/* by max_commands, never read back) and writes reversed-z depth (clear     */
/* 0.0, compare GREATER) into width * height floats, row pitch = width.     */
/*                                                                          */
/* ONE definition, shared by the device and the host mirror                 */
/* (orbit_host_raster_depth); the two agree on every byte of `depth` and of */
/* `stats`.  All arithmetic is fp32, round-to-nearest, never contracted,    */
/* IEEE divides.                                                            */
/*  R1 decode (forward_depth_prepass.vert / .mesh:44-59): nt =              */
/*     cmd_index_count / 3; vcount = cmd_first_index / 4 - cmd_vertex_offset*/
/*     (cmd_vertex_offset taken as its u32 bits); corner bytes start at     */
/*     byte cmd_first_index of meshlet_data; global vertex =                */
/*     meshlet_vertex_offset + meshlet_data[cmd_vertex_offset + corner], in */
/*     64 bits; entity = cmd_first_instance.  cmd_instance_count and        */
/*     meshlet_index are not read.                                          */
/*  R2 mvp = view_proj x model (OpMatrixTimesMatrix), clip = mvp x (p, 1)   */
/*     (OpMatrixTimesVector): left-to-right rounded sums.                   */
/*  R3 per vertex w > 0 && z >= 0 && z <= w (false for NaN).  A triangle    */
/*     with a failing vertex is NOT DRAWN (clip_skipped).  NEAR-PLANE       */
/*     CLIPPING IS OUT OF SCOPE: skipping only leaves the depth farther,    */
/*     the safe side for occlusion.                                         */
/*  R3c only with ORBIT_RASTER_CLIP_NEAR (without it R3 stands as above):   */
/*     a triangle with a failing vertex is cut at the near plane z = w.     */
/*     c_k = (x, y, z, w) are R2's clip coordinates, in_k is R3's test.     */
/*     All three in: nothing changes.  Otherwise the triangle is ELIGIBLE   */
/*     iff all twelve coordinates are finite, every z_k >= 0 and at least   */
/*     one in_k holds; not eligible is clip_skipped as before (all three    */
/*     out, a NaN or infinity, a vertex beyond the far plane).              */
/*     New vertices: b_k = w_k - z_k.  N(i, o), on the edge from an in      */
/*     vertex i to an out vertex o: den = b_i - b_o; !(den > 0): the whole  */
/*     triangle is clip_skipped; t = b_i / den; x = x_i + t * (x_o - x_i),  */
/*     y and w alike; !(w > 0): the whole triangle is clip_skipped; its     */
/*     depth is d = 1.0f exactly (it lies on the near plane; its z is not   */
/*     computed); X, Y and the guard flag are R4's on (x, y, w).  N depends */
/*     on the ordered pair (in, out) only, not on the winding: two          */
/*     triangles sharing a crossing edge get the same vertex, the mesh      */
/*     stays watertight.                                                    */
/*     Pieces: (v0, v1, v2) is rotated cyclically to (a, b, c), a the lone  */
/*     vertex (the only in vertex, or the only out vertex).  One in:        */
/*     piece0 = (a, N(a,b), N(a,c)).  One out: P = N(b,a), Q = N(c,a),      */
/*     piece0 = (b, c, Q), piece1 = (b, Q, P).  Both forms keep the         */
/*     orientation.  Each piece goes through R4's guard test and R5-R8 as   */
/*     a triangle of its own (area, facing, box, edges, depth plane); in    */
/*     the visibility word every piece carries the ORIGINAL triangle's t.   */
/*     The diagonal b-Q is shared with identical snapped ends: the          */
/*     top-left rule gives each sample on it to exactly one piece.          */
/*     Counters: a clipped triangle is counted ONCE, under the best         */
/*     outcome of its pieces, in the priority drawn, guard_skipped,         */
/*     back_facing, no_coverage (guard_skipped only when no piece drew      */
/*     and one failed R4's guard); triangles = clip_skipped +               */
/*     guard_skipped + no_coverage + back_facing + drawn still holds;       */
/*     fragments sums over the pieces.                                      */
/*     Consequences: a triangle R3 accepts goes through unchanged, so the   */
/*     flagged result is pixel-wise >= the unflagged one on the u32 view;   */
/*     with the flag on both calls V4 holds unchanged (high halves = the    */
/*     depth call's bytes, equal stats); everything still depends on one    */
/*     triangle only: independent of scheduling.  Clipping against the      */
/*     SIDE planes stays out of scope: a piece whose vertex leaves R4's     */
/*     guard band is guard_skipped, the safe side.  With a near plane at    */
/*     0.01 that is every crossing triangle further than about              */
/*     0.01 * 2^15 / (W / 2) to the side of the eye.                        */
/*  R4 ndc = clip.xyz / w; xs = (ndc.x * 0.5 + 0.5) * W; ys = (ndc.y * -0.5 */
/*     + 0.5) * H (negative viewport height, commands.rs:303-313; the       */
/*     cull's uv, entity_cull.comp:99-101); X = rint(xs * 256), Y =         */
/*     rint(ys * 256), ties to even.  A triangle with a vertex whose        */
/*     |xs * 256| or |ys * 256| is not below 2^23 is not drawn              */
/*     (guard_skipped).                                                     */
/*  R4w only with ORBIT_RASTER_WIDE_GUARD (without it R4 stands as above):   */
/*     xf = xs * 256 and yf = ys * 256 are R4's floats.  A vertex is NARROW  */
/*     if |xf| < 2^23 and |yf| < 2^23 (R4's test, R4's X, Y); otherwise WIDE */
/*     if |xf| < 2^60 and |yf| < 2^60 (false for NaN and infinity), with     */
/*     X = (int64)rintf(xf), Y = (int64)rintf(yf) — exact, as a float of     */
/*     2^23 or more is an integer (a coordinate still below 2^23 beside a    */
/*     wide one rounds as in R4); anything else is OUT OF BAND.  A triangle, */
/*     or a piece of R3c, whose vertices are all narrow goes through R5-R8   */
/*     unchanged: the same bytes and counters as without the flag.  One with */
/*     a vertex out of band is guard_skipped.  Any other is a WIDE TRIANGLE: */
/*      R5w A is R5's expression in 128-bit integers; A == 0, the facing and */
/*          the swap to A > 0 as in R5.                                      */
/*      R6w the box is R6's formula on the int64 X, Y, clamped to the        */
/*          target; E is R6's expression in 128-bit integers, with the same  */
/*          top-left rule.  |X|, |Y| < 2^60, so a difference is below 2^61,  */
/*          a product below 2^122 and A or an edge value below 2^123:        */
/*          nothing overflows.                                               */
/*      R7w the depth plane in double precision, every operation rounded on  */
/*          its own, never contracted (d_i are R7's floats):                 */
/*          A_d = (double)(int64)(A >> 64) * 2^64 + (double)(uint64)A;       */
/*          D10 = (double)d1 - (double)d0; D20 = (double)d2 - (double)d0;    */
/*          gx = (D10 * (double)(Y2-Y0) - D20 * (double)(Y1-Y0)) / A_d;      */
/*          gy = (D20 * (double)(X1-X0) - D10 * (double)(X2-X0)) / A_d;      */
/*          d = (float)(((double)d0 + gx * (double)(px-X0))                  */
/*                      + gy * (double)(py-Y0));                             */
/*          then d = min(d, 1), d > 0, R8 / V2 as before.                    */
/*     Counters as before; in R3c's best-outcome rule guard_skipped now      */
/*     means "a vertex out of band".  Consequences: a triangle R4 accepts is */
/*     untouched, so the flagged result is pixel-wise >= the unflagged one   */
/*     on the u32 view; V4 holds with the flag on both calls; a word still   */
/*     depends on one triangle only.  An edge shared by a narrow and a wide  */
/*     triangle has two narrow ends, hence the same integers on both sides;  */
/*     an edge with a wide end is shared by two wide triangles that snap it  */
/*     alike; E is the same expression either way, so the top-left rule      */
/*     gives every sample on a shared edge to exactly one side: the mesh     */
/*     stays watertight.  No vertex and no piece is added: the side planes   */
/*     are still not clipped, the integers are wide enough not to need it.   */
/*  R5 A = (X1-X0)(Y2-Y0) - (X2-X0)(Y1-Y0) in int64.  A == 0: no_coverage.  */
/*     Front <=> A < 0 (cull BACK, front COUNTER_CLOCKWISE,                 */
/*     pipeline.rs:201-202); back faces are dropped (back_facing) unless    */
/*     ORBIT_RASTER_CULL_NONE.  The survivor is normalised to A > 0 by      */
/*     swapping vertices 1 and 2.                                           */
/*  R6 sample = pixel centre (256 x + 128, 256 y + 128); pixels = the       */
/*     centres inside the snapped bounding box, clamped to the target;      */
/*     E(a, b, p) = (bx-ax)(py-ay) - (by-ay)(px-ax) in int64; inside iff    */
/*     for all three edges E > 0, or E == 0 and the edge is top-left        */
/*     (dy < 0 || (dy == 0 && dx > 0)).  No inside sample: no_coverage.     */
/*  R7 d_i = z_i / w_i; A_f = (float)(double)A;                             */
/*     gx = ((d1-d0) * (float)(Y2-Y0) - (d2-d0) * (float)(Y1-Y0)) / A_f;    */
/*     gy = ((d2-d0) * (float)(X1-X0) - (d1-d0) * (float)(X2-X0)) / A_f;    */
/*     d = (d0 + gx * (float)(px-X0)) + gy * (float)(py-Y0); d = min(d, 1); */
/*     a sample with !(d > 0) writes nothing.  fragments = inside samples   */
/*     with d > 0.                                                          */
/*  R8 depth[y * W + x] = max(old, d) on the u32 view (atomicMax): the      */
/*     buffer is independent of scheduling and of command order; no counter */
/*     depends on order.                                                    */
/*  R9 range checks on the device, before anything is read: a command whose */
/*     index words or corner bytes reach beyond meshlet_data_words, with    */
/*     cmd_first_index / 4 < cmd_vertex_offset, vcount > 255, a corner >=   */
/*     vcount, a vertex >= vertex_count or an entity >= entity_count is     */
/*     skipped whole (range_errors) and ORBIT_E_RANGE is latched            */
/*     (orbit_ctx_status); the other commands are still drawn.              */
/* stats (may be NULL) is cleared by the call on the stream, then counts:   */
/* commands = min(count, max_commands); triangles = the nt of the commands  */
/* that passed R9 = clip_skipped + guard_skipped + no_coverage +            */
/* back_facing + drawn (tested in that order: R3, R4, A == 0, facing, R6;   */
/* with ORBIT_RASTER_CLIP_NEAR a cut triangle counts once, see R3c).        */
/*                                                                          */
/* ORBIT_RASTER_CLEAR is LoadOp::Clear(0.0): the call clears `depth` on the */
/* stream first; without it the call is LoadOp::Load, the late pass, and    */
/* `depth` must hold what an earlier call left (floats in [0, 1]).          */
/* Masked materials cannot be alpha-tested here (no textures): an OCCLUDER  */
/* depth should come from a cull with alpha_mode_flag = ORBIT_ALPHA_OPAQUE. */
/*   ORBIT_E_INVALID  job, draw_commands, meshlet_data, vertices,           */
/*                    entity_data or depth NULL; a pointer not 4-B aligned  */
/*                    (entity_data: 16 B); vertex_stride < position_offset  */
/*                    + 12, stride or offset no multiple of 4; width or     */
/*                    height 0 or above ORBIT_RASTER_MAX_DIM (the target    */
/*                    must lie inside the guard band of R4); unknown flags  */
/* A count of 0 is ORBIT_OK (with CLEAR it still clears).  The call         */
/* allocates nothing, uses no scratch and never synchronises the host: a    */
/* graph can capture it on its first call.  caps.arith_profile and          */
/* dispatch_size do not apply.                                              */
/* ------------------------------------------------------------------------ */
typedef struct OrbitRasterStats { /* DEVICE, 32 B */
    uint32_t commands, triangles, clip_skipped, guard_skipped, back_facing, no_coverage, fragments, range_errors;
} OrbitRasterStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitRasterStats) == 32, "RasterStats is 32 B");

#define ORBIT_RASTER_CLEAR 1u     /* flags: LoadOp::Clear(0.0) instead of LoadOp::Load */
#define ORBIT_RASTER_CULL_NONE 2u /* flags: draw back faces too */
/* (bit 2, value 4, is not a flag: it stays unknown and rejected, the value the tests of unknown flags use) */
#define ORBIT_RASTER_CLIP_NEAR 8u /* flags: R3c, near-plane clipping of the triangles R3 rejects */
/* (bit 4, value 16, is not a flag either) */
#define ORBIT_RASTER_WIDE_GUARD 32u /* flags: R4w, triangles with a vertex beyond R4's guard band are drawn */
#define ORBIT_RASTER_MAX_DIM 32768u
typedef struct OrbitRasterDepth { /* HOST block, 160 B; every pointer a DEVICE pointer */
    const void *draw_commands;          /* {u32 count; OrbitMeshletDrawCommand[max_commands]} */
    const uint32_t *meshlet_data;       /* meshlet_data_buffer */
    const void *vertices;               /* position i = 3 floats at i * vertex_stride + position_offset */
    const OrbitEntityData *entity_data; /* entity_count rows */
    float *depth;                       /* width * height floats */
    OrbitRasterStats *stats;            /* NULL, or the counters */
    uint64_t meshlet_data_words, vertex_count;
    uint32_t max_commands, entity_count, vertex_stride, position_offset, width, height, flags, _pad;
    float view_proj[16];                /* column-major (forward_depth_prepass.mesh:14) */
} OrbitRasterDepth;
ORBIT_STATIC_ASSERT(sizeof(OrbitRasterDepth) == 160, "RasterDepth is 160 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitRasterDepth, meshlet_data_words) == 48, "meshlet_data_words @48");
ORBIT_STATIC_ASSERT(offsetof(OrbitRasterDepth, max_commands) == 64, "max_commands @64");
ORBIT_STATIC_ASSERT(offsetof(OrbitRasterDepth, view_proj) == 96, "view_proj @96");

/* the depth prepass of the draw commands in compute; see above */
int32_t orbit_raster_depth(OrbitCtx *ctx, const OrbitRasterDepth *job, void *stream);

/* ------------------------------------------------------------------------ */
/* Visibility buffer on the device.  orbit_raster_visibility is             */
/* orbit_raster_depth with the identity of the winner kept: per pixel one   */
/* u64 holding depth, draw and triangle, merged by one 64-bit atomicMax;    */
/* orbit_visibility_resolve turns the buffer into depth, per-command pixel  */
/* counts and the visible set.  Same definition on the device and in the    */
/* host mirror (orbit_host_raster_visibility, orbit_host_visibility_resolve)*/
/*  V1 R1-R7 and R9 hold unchanged: the same decode, transform, snap,       */
/*     rejects, coverage and depth plane (raster_common.h).                 */
/*  V2 an inside sample with d > 0 of triangle t of command i (its position */
/*     in the list) produces the word                                       */
/*       (u64)float_bits(d) << 32 | (command_base + i) << 8 | t;            */
/*     visibility[y * W + x] = max(old, word) on the u64 view (64-bit       */
/*     atomicMax).  Cleared is 0, and 0 is an uncovered pixel: d > 0 for    */
/*     every written word.  Equal depth resolves to the larger id.  A word  */
/*     depends on one triangle and its position in the list only: the       */
/*     buffer is independent of scheduling (NOT of command order: the id is */
/*     the position), and every counter is order-free as before.            */
/*  V3 a command with nt > 256 is skipped whole (range_errors) and latches  */
/*     ORBIT_E_RANGE, like the R9 failures.  command_base + max_commands >  */
/*     ORBIT_VIS_MAX_COMMANDS, or visibility NULL or not 8-B aligned, is    */
/*     ORBIT_E_INVALID; every other argument error is orbit_raster_depth's. */
/*  V4 consequences: the high halves equal, byte for byte, the `depth`      */
/*     orbit_raster_depth leaves for the same job, and `stats` is identical */
/*     as long as no command has nt > 256.                                  */
/* ORBIT_RASTER_CLEAR clears the buffer to 0 on the stream first; without   */
/* it the call merges into what an earlier call left (the late pass), and   */
/* command_base keeps the late list's ids apart from the early one's.       */
/* ORBIT_RASTER_CULL_NONE, ORBIT_RASTER_CLIP_NEAR (R3c) and                 */
/* ORBIT_RASTER_WIDE_GUARD (R4w) as before.  No                             */
/* allocation, no scratch, no host                                          */
/* wait, the count is read on the device, kernels only: a graph captures    */
/* the call on a fresh context's first call.                                */
/*                                                                          */
/* orbit_visibility_resolve reads each word once.  Each output may be NULL; */
/* all three NULL is ORBIT_E_INVALID:                                       */
/*   depth[p]           the high half of word p as a float: what            */
/*                      orbit_depth_reduce and the late cull read           */
/*   command_pixels[k]  k < max_commands, cleared by the call: the pixels   */
/*                      whose winner is command command_base + k            */
/*   stats              cleared by the call.  covered_pixels: words != 0;   */
/*                      foreign_pixels: covered pixels whose command lies   */
/*                      outside [command_base, command_base + max_commands);*/
/*                      visible_commands: non-zero entries of               */
/*                      command_pixels, 0 when command_pixels is NULL       */
/* All outputs are integer sums: independent of scheduling.                 */
/*   ORBIT_E_INVALID  job or visibility NULL, visibility not 8-B aligned,   */
/*                    an output not 4-B aligned, all outputs NULL, width or */
/*                    height 0 or above ORBIT_RASTER_MAX_DIM, command_base  */
/*                    + max_commands > ORBIT_VIS_MAX_COMMANDS               */
/* Capturable, with the same no-allocation and no-host-wait rules.          */
/* ------------------------------------------------------------------------ */
#define ORBIT_VIS_MAX_COMMANDS (1u << 24)
typedef struct OrbitRasterVisibility { /* HOST block, 160 B; every pointer a DEVICE pointer; as OrbitRasterDepth */
    const void *draw_commands;
    const uint32_t *meshlet_data;
    const void *vertices;
    const OrbitEntityData *entity_data;
    uint64_t *visibility;               /* width * height u64, 8-B aligned */
    OrbitRasterStats *stats;            /* NULL, or the counters */
    uint64_t meshlet_data_words, vertex_count;
    uint32_t max_commands, entity_count, vertex_stride, position_offset, width, height, flags, command_base;
    float view_proj[16];
} OrbitRasterVisibility;
ORBIT_STATIC_ASSERT(sizeof(OrbitRasterVisibility) == 160, "RasterVisibility is 160 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitRasterVisibility, visibility) == 32, "visibility @32");
ORBIT_STATIC_ASSERT(offsetof(OrbitRasterVisibility, meshlet_data_words) == 48, "meshlet_data_words @48");
ORBIT_STATIC_ASSERT(offsetof(OrbitRasterVisibility, max_commands) == 64, "max_commands @64");
ORBIT_STATIC_ASSERT(offsetof(OrbitRasterVisibility, command_base) == 92, "command_base @92");
ORBIT_STATIC_ASSERT(offsetof(OrbitRasterVisibility, view_proj) == 96, "view_proj @96");

typedef struct OrbitVisibilityStats { /* DEVICE, 16 B */
    uint32_t covered_pixels, visible_commands, foreign_pixels, _pad;
} OrbitVisibilityStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitVisibilityStats) == 16, "VisibilityStats is 16 B");
typedef struct OrbitVisibilityResolve { /* HOST block, 48 B; every pointer a DEVICE pointer */
    const uint64_t *visibility;  /* width * height u64 */
    float *depth;                /* NULL, or width * height floats */
    uint32_t *command_pixels;    /* NULL, or max_commands words */
    OrbitVisibilityStats *stats; /* NULL, or the counters */
    uint32_t width, height, command_base, max_commands;
} OrbitVisibilityResolve;
ORBIT_STATIC_ASSERT(sizeof(OrbitVisibilityResolve) == 48, "VisibilityResolve is 48 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitVisibilityResolve, stats) == 24, "stats @24");
ORBIT_STATIC_ASSERT(offsetof(OrbitVisibilityResolve, width) == 32, "width @32");

/* the visibility buffer of the draw commands in compute, and its resolve; see above */
int32_t orbit_raster_visibility(OrbitCtx *ctx, const OrbitRasterVisibility *job, void *stream);
int32_t orbit_visibility_resolve(OrbitCtx *ctx, const OrbitVisibilityResolve *job, void *stream);

/* ------------------------------------------------------------------------ */
/* The visible draw list.  orbit_visibility_compact turns a visibility      */
/* buffer and the list that produced it into the exact list of the commands */
/* that own a pixel, in the list's order, optionally cut down to the        */
/* triangles that own one.  The output has the layout orbit_meshlet_cull    */
/* writes and orbit_raster_depth / orbit_raster_visibility read.  ONE       */
/* definition for the device and the host mirror                            */
/* (orbit_host_visibility_compact); the two agree on every byte of every    */
/* output.                                                                  */
/*  C1 mark: n = min(count, max_commands), the count read ON THE DEVICE and */
/*     never read back.  A word != 0 with k = ((word >> 8) & 0xFFFFFF) -    */
/*     command_base (u32, wrapping) and t = word & 255 sets bit t & 31 of   */
/*     triangle_masks[8 * k + (t >> 5)] iff k < n; any other covered pixel  */
/*     is foreign.  THIS DIFFERS FROM orbit_visibility_resolve, which owns  */
/*     k < max_commands without reading the list.  covered_pixels = words   */
/*     != 0.  The masks of k >= n stay 0 (all 8 * max_commands words are    */
/*     cleared by the call).                                                */
/*  C2 visible: command k is visible iff its 256-bit mask is non-zero; m_k  */
/*     is the mask's popcount.  It is CONSISTENT iff nt = cmd_index_count / */
/*     3 <= 256 and no mask bit t >= nt is set; with                        */
/*     ORBIT_COMPACT_TRIANGLES it must also pass R9's checks that concern   */
/*     meshlet_data: first_word = cmd_first_index / 4 >= cmd_vertex_offset  */
/*     (u32 bits), vcount = first_word - cmd_vertex_offset <= 255,          */
/*     first_word <= meshlet_data_words and (cmd_first_index + 3 * nt + 3)  */
/*     / 4 <= meshlet_data_words (in 64 bits).  A visible, inconsistent     */
/*     command is skipped whole, counted in range_errors, and latches       */
/*     ORBIT_E_RANGE; it only arises when the buffer was not made from this */
/*     list.  visible_commands and visible_triangles count the visible      */
/*     consistent commands and their set bits.                              */
/*  C3 order and capacity: the visible consistent commands are numbered j = */
/*     0, 1, ... in ascending k.  With the flag size_j = vcount + (3 * m +  */
/*     3) / 4 words, base_j = the sum of the sizes before j (in 64 bits),   */
/*     data_words_needed = the total (saturating at 2^32 - 1); without it   */
/*     every size is 0.  Command j is written iff j < visible_capacity and, */
/*     with the flag, base_j + size_j <= visible_data_words.  base_j +      */
/*     size_j grows with j, so the written commands are a prefix.           */
/*     visible_commands[0] (the output's count) = written_commands; the     */
/*     rest are dropped_commands; any drop latches ORBIT_E_CAPACITY.        */
/*     data_words_needed and stats.visible_commands tell the caller what to */
/*     allocate.  visible_ids[j] = command_base + k.  Entries behind the    */
/*     written ones are not touched.                                        */
/*  C4 without the flag the written command is the input command's seven    */
/*     words verbatim (it still reads the original meshlet_data).           */
/*  C5 with the flag visible_data[base_j, base_j + vcount) is a copy of     */
/*     meshlet_data[cmd_vertex_offset, + vcount); then come the corner      */
/*     bytes of the set triangles in ascending t, three bytes each, packed; */
/*     the pad bytes of the last word are 0.  The command is copied with    */
/*     cmd_index_count = 3 * m, cmd_vertex_offset = base_j and              */
/*     cmd_first_index = 4 * (base_j + vcount): R1 decodes the same vcount  */
/*     from it.  Words of visible_data beyond the written regions are not   */
/*     touched.                                                             */
/*  C6 consequences.  Let the buffer come from ONE ORBIT_RASTER_CLEAR call  */
/*     of the list with this command_base, and nothing be dropped.          */
/*     Rasterise the output list with the same flags, command_base 0, and   */
/*     visible_data (flag) or the original meshlet_data (no flag):          */
/*     (a) the high halves are equal byte for byte; (b) a pixel that held   */
/*     (command_base + k, t) holds (j, r) with visible_ids[j] =             */
/*     command_base + k; (c) r is the rank of t among the set bits of mask  */
/*     k, and r = t without the flag — ties keep their winner, because both */
/*     orders are preserved; (d) with the flag the output raster's          */
/*     `triangles` equals visible_triangles and its four skip counters are  */
/*     0.  Resolving the output buffer gives visible_commands ==            */
/*     written_commands and no entry of command_pixels is 0.                */
/* stats (may be NULL) is cleared by the call, as are triangle_masks, the   */
/* workspace and the output's count.  All outputs are integer sums, ORs and */
/* prefix sums: independent of scheduling.                                  */
/*   ORBIT_E_INVALID  job NULL; visibility, draw_commands, triangle_masks,  */
/*                    visible_commands or workspace NULL; meshlet_data or   */
/*                    visible_data NULL with ORBIT_COMPACT_TRIANGLES; a     */
/*                    pointer misaligned (visibility, workspace: 8 B, the   */
/*                    rest: 4 B); workspace_bytes <                         */
/*                    orbit_visibility_compact_workspace(max_commands);     */
/*                    width or height 0 or above ORBIT_RASTER_MAX_DIM;      */
/*                    command_base + max_commands > ORBIT_VIS_MAX_COMMANDS; */
/*                    visible_data_words > 2^30 (cmd_first_index is a byte  */
/*                    offset in 32 bits); unknown flags                     */
/* max_commands 0, or a count of 0, is ORBIT_OK with an empty list (the     */
/* pixels are still counted: all covered ones are foreign).  The call       */
/* allocates nothing, takes all scratch from the caller, never waits on the */
/* host and is kernel nodes only: a graph captures it on a fresh context's  */
/* first call.                                                              */
/* ------------------------------------------------------------------------ */
#define ORBIT_COMPACT_TRIANGLES 1u /* flags: cut each visible command down to its visible triangles */
typedef struct OrbitVisibilityCompactStats { /* DEVICE, 32 B, cleared by the call */
    uint32_t covered_pixels, foreign_pixels, visible_commands, visible_triangles, written_commands, dropped_commands,
        data_words_needed, range_errors;
} OrbitVisibilityCompactStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitVisibilityCompactStats) == 32, "VisibilityCompactStats is 32 B");
typedef struct OrbitVisibilityCompact { /* HOST block, 120 B; every pointer a DEVICE pointer */
    const uint64_t *visibility;         /* width * height u64, as orbit_raster_visibility left it */
    const void *draw_commands;          /* {u32 count; OrbitMeshletDrawCommand[max_commands]}: the list that was rasterised with this command_base */
    const uint32_t *meshlet_data;       /* its meshlet_data; may be NULL without ORBIT_COMPACT_TRIANGLES */
    uint32_t *triangle_masks;           /* required: 8 * max_commands words, cleared by the call */
    void *visible_commands;             /* required: {u32 count; OrbitMeshletDrawCommand[visible_capacity]} */
    uint32_t *visible_ids;              /* NULL, or visible_capacity words */
    uint32_t *visible_data;             /* required iff ORBIT_COMPACT_TRIANGLES: visible_data_words words */
    OrbitVisibilityCompactStats *stats; /* NULL, or the counters */
    void *workspace;                    /* required: orbit_visibility_compact_workspace(max_commands) bytes, 8-B aligned */
    uint64_t meshlet_data_words, workspace_bytes;
    uint32_t width, height, command_base, max_commands, visible_capacity, visible_data_words, flags, _pad;
} OrbitVisibilityCompact;
ORBIT_STATIC_ASSERT(sizeof(OrbitVisibilityCompact) == 120, "VisibilityCompact is 120 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitVisibilityCompact, meshlet_data_words) == 72, "meshlet_data_words @72");
ORBIT_STATIC_ASSERT(offsetof(OrbitVisibilityCompact, width) == 88, "width @88");

/* the scratch of the call below, in bytes: a function of max_commands alone, never 0 */
uint64_t orbit_visibility_compact_workspace(uint32_t max_commands);
/* the exact visible draw list of a visibility buffer; see above */
int32_t orbit_visibility_compact(OrbitCtx *ctx, const OrbitVisibilityCompact *job, void *stream);

/* ------------------------------------------------------------------------ */
/* The surface of a visibility buffer.  orbit_visibility_surface reads a    */
/* buffer and the list that made it and writes, for each pixel the list     */
/* owns, the perspective-correct barycentrics of the sample in the owning   */
/* triangle, their one-pixel differences, and the triangle's entity and     */
/* three global vertices: what a renderer behind a compute-only part needs  */
/* to shade, without restating R1-R6.  It uses the functions of the raster  */
/* (raster_common.h), so a written pixel has 0 <= l1, l2 <= 1.  ONE         */
/* definition for the device and the host mirror                            */
/* (orbit_host_visibility_surface); the two agree on every byte of every    */
/* output.  Float arithmetic as in R2-R7: fp32, round to nearest, every     */
/* operation rounded on its own, never contracted, IEEE divides.            */
/*  S1 decode: n = min(count, max_commands), the count read ON THE DEVICE.  */
/*     A word of 0 is uncovered.  Otherwise id = (word >> 8) & 0xFFFFFF, t  */
/*     = word & 255, k = id - command_base (u32, wrapping); k >= n is a     */
/*     FOREIGN pixel (C1's rule, not the resolve's).  Uncovered and foreign */
/*     pixels are not written: a frame's two lists are two calls with two   */
/*     bases into the same outputs, the second without ORBIT_SURFACE_CLEAR. */
/*  S2 consistency of (k, t): command k passes R9 WHOLE, as the drawing     */
/*     call asked it (its ranges, its entity, every index word and every    */
/*     corner byte; nothing is read before it is known to be in range) and  */
/*     V3's nt <= 256, and t < nt.  The three corners then go               */
/*     through R1-R4 (clip_position, vertex_from_clip; not R4w).  A vertex  */
/*     failing R3 or R4's guard makes the pixel UNSUPPORTED: what a buffer  */
/*     drawn with ORBIT_RASTER_CLIP_NEAR or ORBIT_RASTER_WIDE_GUARD         */
/*     legitimately holds; the status stays OK.  THE PIECES OF R3c AND THE  */
/*     WIDE TRIANGLES OF R4w ARE OUT OF SCOPE.  Otherwise R5-R7's setup     */
/*     runs with the facing not asked (it was the drawing call's decision). */
/*     The pixel is STALE, and ORBIT_E_RANGE is latched, if a check above   */
/*     failed, the setup does not draw (A == 0, an empty box), the sample   */
/*     (256 x + 128, 256 y + 128) is not inside (R6, top-left rule), or R7's */
/*     d there is not > 0 or its bits differ from the word's high half.     */
/*     Unsupported and stale pixels are not written.                        */
/*  S3 barycentrics B(px, py), defined for any sample: with R5's normalised */
/*     vertices (A > 0, 1 and 2 possibly swapped) and edges j = 0, 1, 2     */
/*     from vertex j to vertex j + 1, E_j = dx_j * (py - Y_j) - dy_j * (px  */
/*     - X_j) in int64 (R6's E WITHOUT the top-left bias; E_0 + E_1 + E_2 = */
/*     A); e_j = (float)(double)E_j; iw_j = 1.0f / w_j (R2's clip w);       */
/*     q0 = e1 * iw0; q1 = e2 * iw1; q2 = e0 * iw2; s = (q0 + q1) + q2;     */
/*     l1 = q1 / s; l2 = q2 / s; if R5 swapped, l1 and l2 are exchanged:    */
/*     bary[p] = (l1, l2) refers to the corner order in meshlet_data, and   */
/*     l0 is the consumer's 1 - l1 - l2.                                    */
/*  S4 differences: grad[p] = (B(px + 256, py) - B(px, py), B(px, py + 256) */
/*     - B(px, py)) as (dl1/dx, dl2/dx, dl1/dy, dl2/dy): the same triangle  */
/*     at the neighbouring sample, as a quad derivative is.  An axis whose  */
/*     neighbour has !(s > 0) gives (0, 0).                                 */
/*  S5 no non-finite bytes: any of the six floats that is not finite is     */
/*     written as +0.0f (a generated NaN's sign and payload differ between  */
/*     processors).  A pixel with such a float, or with an axis zeroed by   */
/*     S4, counts once in degenerate_pixels; it is still written and still  */
/*     counted in written_pixels.  All six floats are evaluated whichever   */
/*     outputs are given: no counter depends on a NULL output.              */
/*  S6 triangle[p] = (entity, g0, g1, g2): cmd_first_instance and R1's      */
/*     global vertices in meshlet_data's corner order.                      */
/*  S7 ORBIT_SURFACE_CLEAR first fills the given outputs: bary and grad     */
/*     with +0.0f, triangle with 0xFFFFFFFF.  stats (may be NULL) is        */
/*     cleared by the call; covered_pixels = written + foreign +            */
/*     unsupported + stale.  Every output depends on its own pixel only:    */
/*     independent of scheduling.                                           */
/*   ORBIT_E_INVALID  job, visibility, draw_commands, meshlet_data,         */
/*                    vertices or entity_data NULL; bary, grad and triangle */
/*                    all NULL; a pointer misaligned (visibility: 8 B,      */
/*                    entity_data: 16 B, the rest: 4 B); vertex_stride <    */
/*                    position_offset + 12, stride or offset no multiple of */
/*                    4; width or height 0 or above ORBIT_RASTER_MAX_DIM;   */
/*                    command_base + max_commands > ORBIT_VIS_MAX_COMMANDS; */
/*                    triangle given with vertex_count > 2^32; unknown      */
/*                    flags (the raster's flag values among them)           */
/* No allocation, no scratch, no host wait, kernel nodes only: a graph      */
/* captures the call on a fresh context's first call.                       */
/* ------------------------------------------------------------------------ */
#define ORBIT_SURFACE_CLEAR 1u /* flags: fill the given outputs first (S7) */
typedef struct OrbitSurfaceStats { /* DEVICE, 32 B, cleared by the call */
    uint32_t covered_pixels, written_pixels, foreign_pixels, unsupported_pixels, stale_pixels, degenerate_pixels;
    uint32_t cut_pixels, wide_pixels; /* orbit_visibility_surface_drawn only: written from a piece of R3c, from a wide setup; else 0 */
} OrbitSurfaceStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitSurfaceStats) == 32, "SurfaceStats is 32 B");
typedef struct OrbitVisibilitySurface { /* HOST block, 184 B; every pointer a DEVICE pointer */
    const uint64_t *visibility;         /* width * height u64, as orbit_raster_visibility left it */
    const void *draw_commands;          /* the list that was rasterised with this command_base; the rest as OrbitRasterVisibility */
    const uint32_t *meshlet_data;
    const void *vertices;
    const OrbitEntityData *entity_data;
    float *bary;                        /* NULL, or 2 floats per pixel: (l1, l2) */
    float *grad;                        /* NULL, or 4 floats per pixel: (dl1/dx, dl2/dx, dl1/dy, dl2/dy) */
    uint32_t *triangle;                 /* NULL, or 4 words per pixel: (entity, g0, g1, g2) */
    OrbitSurfaceStats *stats;           /* NULL, or the counters */
    uint64_t meshlet_data_words, vertex_count;
    uint32_t max_commands, entity_count, vertex_stride, position_offset, width, height, flags, command_base;
    float view_proj[16];
} OrbitVisibilitySurface;
ORBIT_STATIC_ASSERT(sizeof(OrbitVisibilitySurface) == 184, "VisibilitySurface is 184 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitVisibilitySurface, bary) == 40, "bary @40");
ORBIT_STATIC_ASSERT(offsetof(OrbitVisibilitySurface, stats) == 64, "stats @64");
ORBIT_STATIC_ASSERT(offsetof(OrbitVisibilitySurface, meshlet_data_words) == 72, "meshlet_data_words @72");
ORBIT_STATIC_ASSERT(offsetof(OrbitVisibilitySurface, max_commands) == 88, "max_commands @88");
ORBIT_STATIC_ASSERT(offsetof(OrbitVisibilitySurface, command_base) == 116, "command_base @116");
ORBIT_STATIC_ASSERT(offsetof(OrbitVisibilitySurface, view_proj) == 120, "view_proj @120");

/* barycentrics, their differences and the triangle's ids of every pixel the list owns; see above */
int32_t orbit_visibility_surface(OrbitCtx *ctx, const OrbitVisibilitySurface *job, void *stream);

/* ------------------------------------------------------------------------ */
/* The surface of a buffer drawn with ORBIT_RASTER_CLIP_NEAR and / or       */
/* ORBIT_RASTER_WIDE_GUARD.  orbit_visibility_surface_drawn takes           */
/* orbit_visibility_surface's block and, in raster_flags, how the buffer    */
/* was drawn: any subset of the two flags (CLIP, WIDE below).  With         */
/* raster_flags == 0 it IS orbit_visibility_surface: the same kernels, the  */
/* same bytes, counters and latched status.  Otherwise S1 and S4-S7 stand   */
/* as they are and S2, S3 are extended as follows; ONE definition for the   */
/* device and the host mirror (orbit_host_visibility_surface_drawn), equal  */
/* on every byte; float rules as in S1-S7.                                  */
/*  S2d the classes of a key (k, t).  Command k passes R9 and V3 and t < nt */
/*     as in S2 (else STALE).  c_i = clip_position(...), v_i =              */
/*     vertex_from_clip(c_i, W, H, false, WIDE) of the three corners.       */
/*     (a) every clip_in(c_i) holds and every vertex is narrow: S2-S6       */
/*         exactly, by the same functions, the same bytes.                  */
/*     (b) every clip_in(c_i) holds and some vertex fails the guard.        */
/*         Without WIDE: UNSUPPORTED.  With WIDE: a vertex out of band      */
/*         makes the pixel STALE (the raster guard_skipped it); otherwise   */
/*         setup_triangle_wide(cull_none = true) runs, and the pixel is     */
/*         STALE unless the setup draws, edge_at_wide >= 0 on all three     */
/*         edges and depth_at(SetupW) is > 0 and bit-equal to the word's    */
/*         high half.  Barycentrics by S3w.                                 */
/*     (c) some clip_in(c_i) fails.  Without CLIP: UNSUPPORTED.  With CLIP: */
/*         clip_near_pieces(c0, c1, c2, W, H, pieces, WIDE); count == 0 is  */
/*         STALE.  Otherwise the pieces q = 0 .. count - 1 are CANDIDATES   */
/*         in that order, with piece_vertices' vertices.  A piece with an   */
/*         out-of-band vertex is left out; one with a guard-failing vertex  */
/*         and no WIDE is left out AS NOT COVERED BY THE FLAGS; an          */
/*         all-narrow piece goes through setup_triangle(cull_none = true),  */
/*         edge_at and depth_at, a piece with a wide vertex through their   */
/*         wide forms.  A candidate OWNS the pixel iff its setup draws, the */
/*         sample is inside and the depth is > 0 and bit-equal to the       */
/*         word's high half.  The first owning candidate is the pixel's     */
/*         piece (in exact terms there is at most one: both pieces keep the */
/*         orientation and share the diagonal with identical snapped ends). */
/*         If none owns it the pixel is UNSUPPORTED when a piece was left   */
/*         out as not covered by the flags, STALE otherwise.                */
/*     With both flags given nothing is unsupported.                        */
/*  S3w a wide setup: S3 with E_j in 128-bit integers (R6w's expression     */
/*     without the bias) and e_j = (float)((double)(int64)(E_j >> 64) *     */
/*     2^64 + (double)(uint64)E_j): R7w's conversion, then one rounding to  */
/*     float.  The rest as S3.                                              */
/*  S3c a piece, in terms of the ORIGINAL corners.  P_0, P_1, P_2: the      */
/*     piece's vertices in piece_vertices' order.  w_i: the vertex's clip   */
/*     w; R2's for an original corner, for a new vertex N(i, o) the float   */
/*     w_i + t * (w_o - w_i) that R3c tests for > 0.  Q_i = e_opp(i) *      */
/*     (1.0f / w_i): S3's q of vertex P_i, R5's swap of the piece undone    */
/*     (e by S3, or by S3w for a wide piece).  Each P_i has weights m_i[c]  */
/*     over the original corners c = 0, 1, 2 in meshlet_data's order: an    */
/*     original corner c has m[c] = 1 and the others 0; N(i, o) has m[i] =  */
/*     1.0f - t, m[o] = t and the third 0, t = b_i / den being R3c's own    */
/*     float.  Then n_c = (Q_0 * m_0[c] + Q_1 * m_1[c]) + Q_2 * m_2[c];     */
/*     s = (n_0 + n_1) + n_2; l1 = n_1 / s; l2 = n_2 / s; S4's "positive"   */
/*     is s > 0.  The cut is linear in clip space, so (l1, l2) are the      */
/*     perspective-correct barycentrics of the UNCUT triangle: a consumer   */
/*     interpolates the original vertices' attributes and never sees the    */
/*     cut.  Inside a piece every Q_i >= 0 and 0 <= t <= 1, so n_c >= 0, s  */
/*     >= n_c and 0.0f <= l <= 1.0f on the bit patterns, as for S3.  S4     */
/*     uses the same piece at the neighbouring samples; triangle[p] holds   */
/*     the original three global vertices.                                  */
/*  stats: cut_pixels and wide_pixels count the written pixels of a piece   */
/*     and of a wide setup; a wide piece counts in both.                    */
/*   ORBIT_E_INVALID  orbit_visibility_surface's, under the prefix          */
/*                    visibility_surface_drawn:, and any bit of             */
/*                    raster_flags but the two; all checked before the      */
/*                    context is looked at                                  */
/* Kernel launches only: no allocation, no scratch, no host wait; a graph   */
/* captures the call on a fresh context's first call.                       */
/* ------------------------------------------------------------------------ */
int32_t orbit_visibility_surface_drawn(OrbitCtx *ctx, const OrbitVisibilitySurface *job, uint32_t raster_flags, void *stream);

/* ------------------------------------------------------------------------ */
/* The fragment inputs of a visibility buffer.  orbit_surface_fragments      */
/* reads a buffer, the list that made it, what a surface call left (bary,   */
/* grad, triangle) and the vertex attributes, and writes, for each pixel    */
/* the list owns, what the reference's fragment shader receives: the        */
/* VERTEX_OUTPUT block of shaders/forward/forward_common.glsl:22-28         */
/* (world_pos, uv, normal, tangent, flat material_index) and the dFdx /     */
/* dFdy of uv (forward.frag:250-251).  ONE definition for the device and    */
/* the host mirror (orbit_host_surface_fragments); the two agree on every   */
/* byte of every output.  Float arithmetic as in R2-R7 and S1-S7: fp32,     */
/* round to nearest, every operation rounded on its own, never contracted,  */
/* IEEE divides and square roots.                                           */
/*  F1 ownership is S1's decode: n = min(count, max_commands), the count    */
/*     read ON THE DEVICE.  A word of 0 is uncovered; k = id - command_base */
/*     (u32, wrapping) >= n is a FOREIGN pixel.  Neither is written: a      */
/*     frame's two lists are two calls with two bases into the same         */
/*     outputs, the second without ORBIT_FRAGMENTS_CLEAR.                   */
/*  F2 consistency of an owned pixel p of command k, with T = triangle[p] = */
/*     (entity, g0, g1, g2).  T.entity == 0xFFFFFFFF: the surface call left */
/*     the pixel out (unsupported or stale there, under its clear); the     */
/*     pixel is UNSHADED: not written, the status stays OK.  Otherwise the  */
/*     pixel is STALE, ORBIT_E_RANGE is latched and it is not written, if   */
/*     T.entity >= entity_count, T.entity != cmd[k].cmd_first_instance,     */
/*     some g_i >= vertex_count, or cmd[k].meshlet_index >= meshlet_count.  */
/*     Nothing is read before it is known to be in range.                   */
/*  F3 the vertex stage of corner c = 0, 1, 2 (forward.vert:15-30).  pos: 3 */
/*     floats at g_c * vertex_stride + position_offset; n_c = snorm8 of 3   */
/*     int8 at normal_offset (its 4 bytes are read, the fourth is not       */
/*     used); t_c = snorm8 of 4 int8 at tangent_offset; uv_c: 2 floats at   */
/*     uv_offset.  snorm8(i) = (float)i * 0x3C010204 (the float of those    */
/*     bits: the canonical one of the cull path); -128 is NOT clamped, as   */
/*     forward.vert:26 does not clamp.  wp_c = model_matrix x (pos, 1) by   */
/*     R2's clip_position expression: component r = ((m[r] * x + m[4 + r] * */
/*     y) + m[8 + r] * z) + m[12 + r] * 1.0f.  M3 x v, with M3 rows and     */
/*     columns 0..2 of normal_matrix: component r = (m[r] * x + m[4 + r] *  */
/*     y) + m[8 + r] * z.  normalize(v) = v / sqrtf((x * x + y * y) + z *   */
/*     z), component by component.  GLSL LEAVES Normalize's PRECISION TO    */
/*     THE DRIVER: THIS EXPRESSION IS THIS PROJECT'S CHOICE.  N_c =         */
/*     normalize(M3 x n_c); T_c = (normalize(M3 x t_c.xyz), t_c.w).         */
/*  F4 interpolation: (l1, l2) = bary[p]; l0 = (1.0f - l1) - l2, and l0 <   */
/*     0.0f becomes +0.0f.  Every component a of world_pos (4), normal (3), */
/*     tangent (4) and uv (2) is (a_0 * l0 + a_1 * l1) + a_2 * l2.  The     */
/*     normal is NOT renormalised (forward.frag:280 uses it as it arrives). */
/*  F5 uv_grad[p] = (du/dx, dv/dx, du/dy, dv/dy): with grad[p] = (a, b, c,  */
/*     d), d/dx = (uv_1 - uv_0) * a + (uv_2 - uv_0) * b per component, d/dy */
/*     the same with c, d.  The edge form keeps large uv values from        */
/*     cancelling.  With grad NULL (uv_grad is then NULL too) nothing of it */
/*     is read and the four floats are +0.0f.                               */
/*  F6 material[p] = meshlets[cmd[k].meshlet_index].material_index, widened */
/*     to u32 (forward.vert:32-33).  render_mode 9 is not served.           */
/*  F7 no non-finite bytes, as S5: any of the 17 floats that is not finite  */
/*     is written as +0.0f, and the pixel counts once in degenerate_pixels; */
/*     it is still written and still counted in written_pixels.  All 17     */
/*     floats are evaluated whichever outputs are given: no counter depends */
/*     on a NULL output.                                                    */
/*  F8 ORBIT_FRAGMENTS_CLEAR first fills the given float outputs with       */
/*     +0.0f and material with 0xFFFFFFFF.  stats (may be NULL) is cleared  */
/*     by the call; covered_pixels = written + foreign + unshaded + stale.  */
/*     Every output depends on its own pixel only: independent of           */
/*     scheduling.                                                          */
/* The reference's MeshVertex (types.glsl:64-73, assets/mesh.rs:14-20) is   */
/* vertex_stride 32 with position, normal, uv, tangent at 0 / 12 / 16 / 24. */
/* Only the attributes' own bytes are read (12 + 4 + 8 + 4 per vertex): a   */
/* buffer may end with the last attribute of its last vertex.               */
/*   ORBIT_E_INVALID  (message prefix surface_fragments:) job, visibility,  */
/*                    draw_commands, meshlets, bary, triangle, vertices or  */
/*                    entity_data NULL; all six outputs NULL; uv_grad given */
/*                    with grad NULL; a pointer misaligned (visibility: 8   */
/*                    B, entity_data: 16 B, the rest: 4 B); vertex_stride   */
/*                    or an offset no multiple of 4; vertex_stride smaller  */
/*                    than an attribute's offset + size (12, 4, 8, 4);      */
/*                    width or height 0 or above ORBIT_RASTER_MAX_DIM;      */
/*                    command_base + max_commands > ORBIT_VIS_MAX_COMMANDS; */
/*                    vertex_count > 2^32; unknown flags; an output pointer */
/*                    equal to an input pointer.  All checked before the    */
/*                    context is looked at.                                 */
/* Kernel launches only: no allocation, no scratch, no host wait; a graph   */
/* captures the call on a fresh context's first call.                       */
/* ------------------------------------------------------------------------ */
#define ORBIT_FRAGMENTS_CLEAR 1u /* flags: fill the given outputs first (F8) */
typedef struct OrbitFragmentStats { /* DEVICE, 32 B, cleared by the call */
    uint32_t covered_pixels, written_pixels, foreign_pixels, unshaded_pixels, stale_pixels, degenerate_pixels;
    uint32_t _pad[2];
} OrbitFragmentStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitFragmentStats) == 32, "FragmentStats is 32 B");
typedef struct OrbitSurfaceFragments { /* HOST block, 176 B; every pointer a DEVICE pointer */
    const uint64_t *visibility;         /* width * height u64, as orbit_raster_visibility left it */
    const void *draw_commands;          /* the list that was rasterised with this command_base */
    const OrbitMeshlet *meshlets;       /* meshlet_count records of 32 B; only material_index is read */
    const float *bary;                  /* 2 floats per pixel, as a surface call left them */
    const float *grad;                  /* NULL (then uv_grad is NULL), or 4 floats per pixel */
    const uint32_t *triangle;           /* 4 words per pixel: (entity, g0, g1, g2) */
    const void *vertices;
    const OrbitEntityData *entity_data;
    float *world_pos;                   /* NULL, or 4 floats per pixel */
    float *normal;                      /* NULL, or 3 floats per pixel */
    float *tangent;                     /* NULL, or 4 floats per pixel */
    float *uv;                          /* NULL, or 2 floats per pixel */
    float *uv_grad;                     /* NULL, or 4 floats per pixel: du/dx, dv/dx, du/dy, dv/dy */
    uint32_t *material;                 /* NULL, or 1 word per pixel */
    OrbitFragmentStats *stats;          /* NULL, or the counters */
    uint64_t vertex_count;
    uint32_t meshlet_count, max_commands, entity_count, vertex_stride, position_offset, normal_offset, uv_offset,
        tangent_offset, width, height, flags, command_base;
} OrbitSurfaceFragments;
ORBIT_STATIC_ASSERT(sizeof(OrbitSurfaceFragments) == 176, "SurfaceFragments is 176 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitSurfaceFragments, bary) == 24, "bary @24");
ORBIT_STATIC_ASSERT(offsetof(OrbitSurfaceFragments, world_pos) == 64, "world_pos @64");
ORBIT_STATIC_ASSERT(offsetof(OrbitSurfaceFragments, stats) == 112, "stats @112");
ORBIT_STATIC_ASSERT(offsetof(OrbitSurfaceFragments, vertex_count) == 120, "vertex_count @120");
ORBIT_STATIC_ASSERT(offsetof(OrbitSurfaceFragments, vertex_stride) == 140, "vertex_stride @140");
ORBIT_STATIC_ASSERT(offsetof(OrbitSurfaceFragments, command_base) == 172, "command_base @172");

/* forward.frag's inputs of every pixel the list owns; see above */
int32_t orbit_surface_fragments(OrbitCtx *ctx, const OrbitSurfaceFragments *job, void *stream);

/* ------------------------------------------------------------------------ */
/* Clustered lighting of a visibility buffer.  orbit_fragments_shade reads  */
/* a buffer, what orbit_surface_fragments left under ORBIT_FRAGMENTS_CLEAR  */
/* (world_pos, normal, material), the material and light tables and the     */
/* per-cluster light lists of orbit_compute_clusters, and writes the colour */
/* of every visible pixel: the texture-free part of forward.frag's          */
/* render_mode 0 (material factors, point and directional lights through    */
/* calculate_light) and render_mode 8, the light-count heat map.  ONE       */
/* definition for the device and the host mirror                            */
/* (orbit_host_fragments_shade); the two agree on every byte.  Arithmetic   */
/* as in F1-F8: fp32, round to nearest, every operation rounded on its own, */
/* never contracted, IEEE '/' and sqrtf, GLSL max / clamp (x < y ? y : x).  */
/* dot(a, b) = (ax * bx + ay * by) + az * bz; normalize is F3's v /         */
/* sqrtf((x * x + y * y) + z * z).                                          */
/*  L1 which pixels.  A word of 0 is uncovered.  A covered pixel with       */
/*     material[p] == 0xFFFFFFFF is UNSHADED: not written, the status stays */
/*     OK (the fragments calls of a frame's two lists already merged them:  */
/*     one shade call serves both).  material[p] >= material_count is       */
/*     STALE: ORBIT_E_RANGE is latched, the pixel is not written.           */
/*  L2 the cluster (forward.frag:352-363).  tile = (x / tile_size_px, y /   */
/*     tile_size_px); d = the float of the word's high half (gl_FragCoord.z */
/*     and the float the mark stage read when the clusters were built from  */
/*     orbit_visibility_resolve's depth); slice = uint(fma(log2c(z_near /   */
/*     d), z_scale, z_bias)), saturating, NaN -> 0: the integer of the mark */
/*     stage (the device may take it through the hardware log2 inside the   */
/*     proven guard band: the same integer by construction).  A tile or a   */
/*     slice outside cluster_count is OUTSIDE: zero lights, as an imageLoad */
/*     outside the image returns 0; the pixel is written and counts in      */
/*     outside.  Otherwise (offset, count) = image[tile.x + tile.y * cx +   */
/*     slice * cx * cy] and n = min(count, 256).  The pixel is STALE if     */
/*     offset + n > index_capacity (indices behind the 4-byte header), or   */
/*     if one of the n walked indices is >= light_count.  Nothing is read   */
/*     before it is known to be in range.  lights_walked[p] = n.            */
/*  L3 the material (forward.frag:277-339): the factors base_color.rgb,     */
/*     metallic_factor, roughness_factor, emissive_factor.  Textures are    */
/*     not served: a material with a texture index != 0xFFFFFFFF is shaded  */
/*     from its factors and the pixel counts in textured.  N = normal[p] as */
/*     it arrives; ao is unused.                                            */
/*  L4 V = normalize(view_pos - world_pos.xyz).                             */
/*  L5 the walk, in list order, light_sum starting at emissive.  lc_c =     */
/*     color_c * intensity.  POINT (:460-486): Ld = position - wp; dist =   */
/*     sqrtf(dot(Ld, Ld)); Ld = Ld / dist; dist = max(dist, inner_radius);  */
/*     d2 = dist * dist; att = max(intensity / d2 - (luminance_cutoff * d2) */
/*     / (outer_radius * outer_radius), 0).  DIRECTIONAL: Ld = direction as */
/*     stored, att = 1, shadow = 1: shadow maps are not served, a light     */
/*     with shadow_data_index != 0xFFFFFFFF makes the pixel count in        */
/*     unserved.  SKY is skipped (cube maps) and the pixel counts in        */
/*     unserved.  Any other type is ignored, as the switch has no default.  */
/*     light_sum_c = light_sum_c + L6_c.                                    */
/*  L6 calculate_light (:186-216, functions.glsl:82-100).  EPS = 0.0001f,   */
/*     PI = the float of 3.14159265359.  H = normalize(V + Ld); ndv =       */
/*     max(dot(N, V), EPS); ndl = max(dot(N, Ld), EPS); ndh = max(dot(N,    */
/*     H), 0); hv = max(dot(H, V), 0); r = roughness, a = r * r, a2 = a *   */
/*     a; den = (ndh * ndh) * (a2 - 1) + 1, then den = (PI * den) * den; D  */
/*     = a2 / max(den, EPS); rr = r + 1, k = (rr * rr) / 8; G = (ndv / (ndv */
/*     * (1 - k) + k)) * (ndl / (ndl * (1 - k) + k)); f0_c = 0.04f * (1 -   */
/*     metallic) + albedo_c * metallic; x = 1 - hv, p5 = ((x * x) * (x *    */
/*     x)) * x; F_c = f0_c + (1 - f0_c) * p5; spec_c = ((D * G) * F_c) /    */
/*     ((4 * ndv) * ndl); kD_c = (1 - F_c) * (1 - metallic); the light's    */
/*     term is ((((kD_c * albedo_c) / PI) + spec_c) * (lc_c * att)) * ndl.  */
/*     GLSL LEAVES pow's PRECISION TO THE DRIVER: p5 AS THREE PRODUCTS IS   */
/*     THIS PROJECT'S CHOICE.                                               */
/*  L7 color[p] = (light_sum, 1.0f).  render_mode 8 (:564-567): color[p] =  */
/*     heat_colormap(clamp((float)n / 32.0f, 0, 1)) of functions.glsl:      */
/*     142-171 (red: x < 0.7f ? 4 * x - 1.5f : -4 * x + 4.5f; green: x <    */
/*     0.5f ? 4 * x - 0.5f : -4 * x + 3.5f; blue: x < 0.3f ? 4 * x + 0.5f : */
/*     -4 * x + 2.5f; each clamped to [0, 1]), alpha 1.  L1-L3 hold as in   */
/*     mode 0 (the indices are range-checked), the light rows are not read: */
/*     unserved and degenerate stay 0.                                      */
/*  L8 no non-finite bytes: a colour float that is not finite is written as */
/*     +0.0f and the pixel counts once in degenerate; it is still written.  */
/*  L9 ORBIT_SHADE_CLEAR first fills color with +0.0f and lights_walked     */
/*     with 0.  stats (may be NULL) is cleared by the call; covered =       */
/*     written + unshaded + stale.  Every output depends on its own pixel   */
/*     only: independent of scheduling and of the form of the walk.         */
/* Two forms of the walk give the same bytes (every pixel adds its own list */
/* in list order): per lane, and staged through LDS per cluster when        */
/* tile_size_px is a multiple of 8.  ORBIT_SHADE_FORCE_PER_LANE /           */
/* ORBIT_SHADE_FORCE_STAGED select one; with neither the library chooses.   */
/*   ORBIT_E_INVALID  (message prefix fragments_shade:) job or a required   */
/*                    pointer NULL (all but lights_walked and stats); a     */
/*                    pointer misaligned (visibility, cluster_offset_image: */
/*                    8 B, materials, lights: 16 B, the rest: 4 B); width   */
/*                    or height 0 or above ORBIT_RASTER_MAX_DIM; a zero in  */
/*                    cluster_count or tile_size_px; cluster_count[2] > 32; */
/*                    cx * cy * cz > 2^31; render_mode not 0 or 8; unknown  */
/*                    flags; both FORCE flags; FORCE_STAGED with            */
/*                    tile_size_px % 8 != 0; an output pointer equal to an  */
/*                    input pointer.  All checked before the context is     */
/*                    looked at.                                            */
/* Kernel launches only: no allocation, no scratch, no host wait; a graph   */
/* captures the call on a fresh context's first call.                       */
/* ------------------------------------------------------------------------ */
#define ORBIT_SHADE_CLEAR 1u          /* flags: fill color and lights_walked first (L9) */
#define ORBIT_SHADE_FORCE_PER_LANE 2u /* flags: every lane walks its own list */
#define ORBIT_SHADE_FORCE_STAGED 4u   /* flags: a wave stages each cluster's list in LDS (tile_size_px % 8 == 0) */
#define ORBIT_SHADE_MAX_WALK 256u     /* forward.frag:363 */
typedef struct OrbitShadeStats { /* DEVICE, 32 B, cleared by the call */
    uint32_t covered_pixels, written_pixels, unshaded_pixels, stale_pixels, outside_pixels, degenerate_pixels,
        textured_pixels, unserved_pixels;
} OrbitShadeStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitShadeStats) == 32, "ShadeStats is 32 B");
typedef struct OrbitFragmentsShade { /* HOST block, 160 B; every pointer a DEVICE pointer */
    const uint64_t *visibility;           /* width * height u64, as orbit_raster_visibility left it */
    const float *world_pos;               /* 4 floats per pixel, as orbit_surface_fragments left them */
    const float *normal;                  /* 3 floats per pixel */
    const uint32_t *material;             /* 1 word per pixel; 0xFFFFFFFF: unshaded */
    const OrbitMaterialData *materials;   /* material_count rows of 80 B */
    const OrbitLightData *lights;         /* light_count rows of 64 B */
    const uint32_t *cluster_offset_image; /* cx * cy * cz (offset, count) pairs, as orbit_cluster_assign writes them */
    const void *light_index_buffer;       /* ClusterLightIndices: indices at byte 4 */
    float *color;                         /* 4 floats per pixel */
    uint32_t *lights_walked;              /* NULL, or 1 word per pixel */
    OrbitShadeStats *stats;               /* NULL, or the counters */
    uint32_t material_count, light_count, index_capacity;
    uint32_t cluster_count[3], tile_size_px; /* OrbitGpuClusterInfoBuffer's */
    float z_scale, z_bias, luminance_cutoff; /* OrbitGpuClusterInfoBuffer's */
    float z_near, view_pos[3];               /* PerFrameBuffer's */
    uint32_t render_mode;                    /* 0 or 8 */
    uint32_t width, height, flags;
} OrbitFragmentsShade;
ORBIT_STATIC_ASSERT(sizeof(OrbitFragmentsShade) == 160, "FragmentsShade is 160 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShade, materials) == 32, "materials @32");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShade, color) == 64, "color @64");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShade, material_count) == 88, "material_count @88");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShade, cluster_count) == 100, "cluster_count @100");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShade, z_scale) == 116, "z_scale @116");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShade, z_near) == 128, "z_near @128");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShade, render_mode) == 144, "render_mode @144");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShade, flags) == 156, "flags @156");

/* forward.frag's clustered lighting of every visible pixel; see above */
int32_t orbit_fragments_shade(OrbitCtx *ctx, const OrbitFragmentsShade *job, void *stream);

/* ------------------------------------------------------------------------ */
/* Clustered lighting with cascaded PCSS shadows.                           */
/* orbit_fragments_shade_shadowed is orbit_fragments_shade with L5's        */
/* directional branch served: a directional light whose shadow_data_index   */
/* is not 0xFFFFFFFF is multiplied by forward.frag's shadow term (:81-184,  */
/* :406-459): cascade selection, normal and oriented bias, the 12-tap       */
/* blocker search and the 32 x 4-tap percentage-closer filter over float    */
/* depth maps the caller drew (orbit_raster_depth under each cascade's      */
/* light_projection_matrix with ORBIT_RASTER_CLEAR: reversed z).  ONE       */
/* definition for the device and the host mirror                            */
/* (orbit_host_fragments_shade_shadowed, csrc/shadow_common.h); the two     */
/* agree on every byte.  The job starts with an OrbitFragmentsShade: same   */
/* meaning, same checks.  Arithmetic as in L: fp32, every operation rounded */
/* on its own, never contracted, IEEE '/', GLSL max / clamp, matrix x       */
/* vector as R2's left-to-right rounded sums ((m0 * x + m4 * y) + m8 * z) + */
/* m12 * w.  L1-L4, L6-L9 and L5's point and sky branches hold unchanged.   */
/*  H1 which lights.  A directional light with shadow_data_index = s !=     */
/*     0xFFFFFFFF is a SHADOWED light; its row is r = s - shadow_index_base */
/*     (u32 arithmetic).  r >= shadow_count makes the pixel STALE           */
/*     (ORBIT_E_RANGE, not written); nothing is read before it is known to  */
/*     be in range.  A shadowed light no longer counts the pixel in         */
/*     unserved_pixels; sky still does.                                     */
/*  H2 cascade selection (:414-421, check_ndc_bounds).  For i = 0..3: c =   */
/*     M_i x world_pos[p] (all four floats as they arrive), q = c / c.w     */
/*     over all four components; q is inside iff q.x >= -1, q.y >= -1, q.z  */
/*     >= 0, q.w >= 0 and every component <= 1 (NaN fails).  The first i    */
/*     inside wins.  None: shadow = 1, cascade = 4, the pixel counts in     */
/*     no_cascade_pixels.                                                   */
/*  H3 map = shadow_map_indices[cascade]; map >= shadow_map_count makes the */
/*     pixel STALE.  texel = 1.0f / (float)shadow_resolution.               */
/*  H4 bias (:426-435).  ndl = dot(N, direction); nos = clamp(1 - ndl, 0,   */
/*     1); off_c = ((texel * normal_bias_scale) * nos) * N_c; ob = ndl > 0  */
/*     ? -oriented_bias : oriented_bias; sp_c = (wp_c + off_c) + ob *       */
/*     direction_c.  oriented_bias is taken as given: the reference sends   */
/*     it negated (shadow_renderer.rs:129).                                 */
/*  H5 coordinates (:135-137, :437-442).  c = M_cascade x (sp, 1); x = c.x  */
/*     / c.w, y = (c.y / c.w) * -1, z = c.z / c.w; u = (x + 1) * 0.5, v =   */
/*     (y + 1) * 0.5; inv_ws = 1 / world_size[cascade]; light_uv =          */
/*     inner_radius * inv_ws.                                               */
/*  H6 noise and rotation (functions.glsl:109-112, :140-143).  The seed is  */
/*     the pixel centre (sx, sy) = (x + 0.5, y + 0.5); fract(a) = a -       */
/*     floorf(a); ign = fract(52.9829189f * fract(sx * 0.06711056f + sy *   */
/*     0.00583715f)); theta = (ign * 2) * PI (L6's PI); (s, c) = (sinc,     */
/*     cosc)(theta): k = (int)(theta * 0.636619772f + 0.5f); r = (theta - k */
/*     * 1.5703125f) - k * 4.83826794897e-4f; w = r * r; sin_r = ((((       */
/*     -1.9515295891e-4f * w + 8.3321608736e-3f) * w) + -1.6666654611e-1f)  */
/*     * w) * r + r; cos_r = ((((2.443315711809948e-5f * w +                */
/*     -1.388731625493765e-3f) * w) + 4.166664568298827e-2f) * w) * w + (1  */
/*     - 0.5f * w); (s, c) by k & 3: 0 (sin_r, cos_r), 1 (cos_r, -sin_r), 2 */
/*     (-sin_r, -cos_r), 3 (-cos_r, sin_r).  GLSL LEAVES sin AND cos        */
/*     PRECISION TO THE DRIVER: THIS ROUTINE IS THIS PROJECT'S CHOICE.  rot */
/*     . o = (c * o.x + (-s) * o.y, s * o.x + c * o.y); o_i =               */
/*     poisson_offsets[i] (forward.frag:14-79) as floats, i < 32.           */
/*  H7 blocker search (penumbra_poisson; NEAREST, clamp to edge).  rad =    */
/*     blocker_search_radius * inv_ws; for i < 12: suv = uv + ((rot . o_i)  */
/*     * rad) * inv_ws (the second inv_ws is the reference's); the texel is */
/*     (clamp((int)floorf(suv.x * res), 0, res - 1), the same of suv.y),    */
/*     the conversion saturating, NaN -> 0; t > z: avg = avg + (1 - t),     */
/*     count++.  count == 0: shadow = 1; count == 12: shadow = 0; both      */
/*     count in early_out_pixels.  Otherwise avg = avg / (float)count.      */
/*  H8 filter (:153-170; clamp to edge, GREATER_OR_EQUAL, textureGather).   */
/*     pen = (((1 - z) - avg) / avg) * light_uv; fr = max(pen * inv_ws,     */
/*     texel); for i < 32: sp = uv + (rot . o_i) * fr; fx = sp.x * res -    */
/*     0.5; i0 = floorf(fx), i1 = i0 + 1, both converted (saturating, NaN   */
/*     -> 0) and clamped to [0, res - 1]; sp.y alike; each of the four      */
/*     texels is lit iff z >= t (NaN fails).  shadow = (float)lit / 128.0f: */
/*     the GLSL's float sum, every partial sum an integer below 2^24.  THE  */
/*     SUB-TEXEL PRECISION OF A GATHER IS THE IMPLEMENTATION'S IN VULKAN:   */
/*     fp32 AS WRITTEN IS THIS PROJECT'S CHOICE.                            */
/*  H9 light_sum_c = light_sum_c + (L6_c * shadow) for EVERY directional    */
/*     light (x * 1.0f is x: with no shadowed light in any list color,      */
/*     lights_walked and the base stats equal orbit_fragments_shade's byte  */
/*     for byte).  render_mode 8: H1 still range-checks s (the light's type */
/*     and shadow_data_index are read), nothing else of H is evaluated,     */
/*     shadow_factor and cascade take their defaults and the four shadow    */
/*     counters stay 0.                                                     */
/*  H10 shadow_factor[p] = the shadow of the FIRST shadowed light of the    */
/*     pixel's walk, 1.0f if none (non-finite leaves as +0 under L8);       */
/*     cascade[p] = that light's cascade 0..3, 4 when none holds the pixel, */
/*     0xFFFFFFFF with no shadowed light.  Both are written for written     */
/*     pixels only; ORBIT_SHADE_CLEAR fills them with 1.0f and 0xFFFFFFFF.  */
/*     OrbitShadowStats, cleared by the call, over written pixels:          */
/*     shadowed_pixels evaluated H2 at least once; no_cascade_pixels /      */
/*     early_out_pixels had at least one evaluation end so;                 */
/*     shadow_evaluations = the sum of shadowed lights walked.  Every       */
/*     output depends on its own pixel only.                                */
/* shadow_count == 0 is valid: every shadowed light makes its pixel STALE.  */
/* OUT OF SCOPE: the reference's D16_UNORM quantisation of the maps and the */
/* rasteriser's slope-scaled depth bias (shadow_renderer.rs:414-416) — the  */
/* maps are whatever floats the caller drew —, render_mode 1 (the cascade   */
/* debug view: the cascade plane carries it), textures and sky.             */
/*   ORBIT_E_INVALID  (message prefix fragments_shade_shadowed:) everything */
/*                    orbit_fragments_shade rejects; shadow_count > 0 with  */
/*                    shadows or shadow_maps NULL, shadows not 16-B         */
/*                    aligned, shadow_resolution 0 or above                 */
/*                    ORBIT_RASTER_MAX_DIM, or shadow_map_count * res^2 >   */
/*                    2^31 floats; a buffer not 4-B aligned; an output      */
/*                    pointer equal to an input pointer.                    */
/* Kernel launches only: no allocation, no scratch, no host wait; a graph   */
/* captures the call on a fresh context's first call.                       */
/* ------------------------------------------------------------------------ */
typedef struct OrbitShadowData { /* DEVICE, 288 B: types.glsl:29-33 in std430 */
    float light_projection_matrices[4][16]; /* column-major */
    float shadow_map_world_sizes[4];
    uint32_t shadow_map_indices[4]; /* into shadow_maps: the caller maps its bindless indices onto that array */
} OrbitShadowData;
ORBIT_STATIC_ASSERT(sizeof(OrbitShadowData) == 288, "ShadowData is 288 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitShadowData, shadow_map_world_sizes) == 256, "shadow_map_world_sizes @256");
ORBIT_STATIC_ASSERT(offsetof(OrbitShadowData, shadow_map_indices) == 272, "shadow_map_indices @272");
typedef struct OrbitShadowStats { /* DEVICE, 16 B, cleared by the call (H10) */
    uint32_t shadowed_pixels, no_cascade_pixels, early_out_pixels, shadow_evaluations;
} OrbitShadowStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitShadowStats) == 16, "ShadowStats is 16 B");
typedef struct OrbitFragmentsShadeShadowed { /* HOST block, 232 B; every pointer a DEVICE pointer */
    OrbitFragmentsShade shade;      /* as orbit_fragments_shade takes it */
    const OrbitShadowData *shadows; /* shadow_count rows of 288 B, 16-B aligned */
    const float *shadow_maps;       /* shadow_map_count maps of res * res floats: map k at float k * res * res, row pitch res */
    float *shadow_factor;           /* NULL, or 1 float per pixel */
    uint32_t *cascade;              /* NULL, or 1 word per pixel */
    OrbitShadowStats *shadow_stats; /* NULL, or the counters */
    uint32_t shadow_count;
    uint32_t shadow_index_base; /* MAX_SHADOW_COMMANDS * frame_index, as orbit_scene_update takes it */
    uint32_t shadow_map_count, shadow_resolution;
    float blocker_search_radius, normal_bias_scale, oriented_bias; /* ShadowSettings, types.glsl:35-40 */
    uint32_t _pad;
} OrbitFragmentsShadeShadowed;
ORBIT_STATIC_ASSERT(sizeof(OrbitFragmentsShadeShadowed) == 232, "FragmentsShadeShadowed is 232 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeShadowed, shadows) == 160, "shadows @160");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeShadowed, shadow_factor) == 176, "shadow_factor @176");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeShadowed, shadow_stats) == 192, "shadow_stats @192");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeShadowed, shadow_count) == 200, "shadow_count @200");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeShadowed, shadow_resolution) == 212, "shadow_resolution @212");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeShadowed, blocker_search_radius) == 216, "blocker_search_radius @216");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeShadowed, oriented_bias) == 224, "oriented_bias @224");

/* forward.frag's clustered lighting with cascaded PCSS shadows of every visible pixel; see above */
int32_t orbit_fragments_shade_shadowed(OrbitCtx *ctx, const OrbitFragmentsShadeShadowed *job, void *stream);

/* ------------------------------------------------------------------------ */
/* orbit_bloom and orbit_post_process: from the shade calls' linear HDR     */
/* `color` plane (4 floats per pixel) to the shown image, as the reference  */
/* goes from its colour target to the swapchain: compute_bloom              */
/* (src/passes/bloom.rs, shaders/bloom/bloom_downsample.comp,               */
/* bloom_upsample.comp) and render_post_process (shaders/post_process.frag).*/
/* ONE definition for the device and the host mirror (orbit_host_bloom,     */
/* orbit_host_post_process; csrc/post_common.h); the two agree on every     */
/* byte.  Arithmetic as in L: fp32, every operation rounded on its own,     */
/* never contracted, IEEE '/', GLSL max / clamp.                            */
/*  B1 the chain (bloom.rs:96-171).  levels = min(max(1, floor(log2(max(w,  */
/*     h))) + 1), 6, max_levels); level k is max(w >> k, 1) x max(h >> k,   */
/*     1) texels (level 0 is the full size, bloom.rs:60-80) and starts at   */
/*     the texel count of the levels before it (orbit_bloom_layout).  Level */
/*     0 is downsampled from color, level k from level k - 1; then level    */
/*     k is upsampled into level k - 1 for k = levels - 1 .. 1.  With one   */
/*     level there is no upsample.  Afterwards level 0 holds the bloom      */
/*     image orbit_post_process reads.                                      */
/*  B2 the threshold vector (bloom.rs:106-111), on the host, in float: knee */
/*     = threshold * soft_threshold; tf = (threshold, threshold - knee, 2 * */
/*     knee, 0.25 / (knee + 0.00001)).                                      */
/*  B3 the sampler model of LinearClamp (image.rs:467, device.rs:1316-1320) */
/*     at (u, v) of a src_w x src_h level: s = u * float(src_w) - 0.5f; i0  */
/*     = floor(s), f = s - i0; i0 and i0 + 1 are clamped to [0, src_w - 1]  */
/*     (saturating: +-inf clamp, NaN -> 0); v alike; per channel texel =    */
/*     (t00 * (1 - fx) + t10 * fx) * (1 - fy) + (t01 * (1 - fx) + t11 * fx) */
/*     * fy.  HARDWARE FILTERS WITH FIXED-POINT WEIGHTS: fp32 AS WRITTEN IS */
/*     THIS PROJECT'S CANONICAL CHOICE, as the reduce-min sampler model is  */
/*     for the pyramid.  Taps of level 0 do NOT collapse to one texel: (x + */
/*     0.5 + d) * (1 / W) * W - 0.5 is not an integer in fp32 for most W,   */
/*     so every tap is the full four-texel expression.                      */
/*  B4 the downsample (bloom_downsample.comp:40-89).  uv = ((float(pixel) + */
/*     0.5f) + d) * (1.0f / float(size)) with the DESTINATION size; the 13  */
/*     taps x, y0..y3, z0..z7 and the five groups as the shader has them:   */
/*     g0 = (y0 + y1 + y2 + y3) * 0.125, g1 = (z0 + z0 + z3 + x) * 0.03125  */
/*     (:70 — the binary is the statement), g2 = (z1 + z2 + z4 + x) *       */
/*     0.03125, g3 = (z3 + z5 + z6 + x) * 0.03125, g4 = (z4 + z6 + z7 + x)  */
/*     * 0.03125; result = g0 + g1 + g2 + g3 + g4.  Sums run left to right, */
/*     as the binary's output confirms (tests/golden/spirv_bloom.npz).      */
/*  B5 level 0 only (:20-35, :75-87).  g_k = g_k * karis(g_k), karis(c) = 1 */
/*     / (1 + ((s.r * 0.2126f + s.g * 0.7152f) + s.b * 0.0722f) * 0.25f), s */
/*     = powc(c, 0.45454547f); powc(x, y) = exp2c(y * log2c(x)), 0 for x <= */
/*     0; log2c is L2's; exp2c(x): k = floor(x + 0.5f), r = x - k, p = the  */
/*     degree-7 Taylor polynomial of 2^r by Horner (c_n = ln(2)^n / n!      */
/*     rounded to float), the result 2^k * p; x >= 128 -> +inf, x < -126 -> */
/*     0.  Then prefilter: m = max(r, max(g, b)); soft = clamp(m - tf.y, 0, */
/*     tf.z); soft = (soft * soft) * tf.w; result = result * (max(m - tf.x, */
/*     soft) / max(m, 0.00001f)).  GLSL LEAVES pow's PRECISION TO THE       */
/*     DRIVER: THIS ROUTINE IS THIS PROJECT'S CHOICE, as p5 in L6 and H6's  */
/*     sine and cosine.  MEASURED: the largest relative error of powc(x, 1  */
/*     / 2.2) against float64 over [2^-20, 65504] is 6.65e-7; 3.95 % of the */
/*     packed texels of the hand-built cases differ from the GLSL in        */
/*     float64 packed the same way.                       */
/*  B6 the upsample (bloom_upsample.comp:19-44).  uv = float(pixel) * (1.0f */
/*     / float(size)) + offset, WITHOUT the half pixel, as the shader has   */
/*     it, with the destination's size; r = filter_radius in uv units; the  */
/*     nine taps x (0, 0), y0 (r, 0), y1 (0, r), y2 (-r, 0), y3 (0, -r), z0 */
/*     (r, r), z1 (-r, -r), z2 (-r, r), z3 (r, -r) of the source level by   */
/*     B3; result = (x * 0.25 + (y0 + y1 + y2 + y3) * 0.125) + (z0 + z1 +   */
/*     z2 + z3) * 0.0625; dst = pack(unpack(dst) + result).                 */
/*  B7 the storage is B10G11R11_UFLOAT_PACK32: R in bits 0-10 and G in bits */
/*     11-21 (5 + 6 bits each), B in bits 22-31 (5 + 5 bits), bias 15; the  */
/*     smallest step is 2^-20 for R and G, 2^-19 for B.  Encode: x <= 0 ->  */
/*     0; the rest is truncated toward zero; at or above the largest finite */
/*     value (65024 for R and G, 64512 for B) -> that value, and            */
/*     clamped_texels counts the texel.  Decode is exact.  TRUNCATION IS    */
/*     THE DIRECT3D CONVERSION RULE, WHICH COLOUR BACK ENDS IMPLEMENT;      */
/*     VULKAN LEAVES THE ROUNDING OPEN; NOBODY HAS MEASURED WHAT A DRIVER   */
/*     UNDER THE REFERENCE DOES.  Every level is stored through this        */
/*     encoding, between levels too, whatever the launch form.              */
/*  B8 non-finite values.  A color component that is NaN or +-inf reads as  */
/*     +0.0f in every tap; nonfinite_inputs counts such pixels (r, g or b)  */
/*     once each, as the centre tap of level 0.  A component that is not    */
/*     finite before encoding is stored as 0.  No non-finite bytes are ever */
/*     written.                                                             */
/*  B9 stats (may be NULL) is cleared by the call: levels; texels_written = */
/*     every store, of the downsamples and of the upsamples;                */
/*     nonfinite_inputs; clamped_texels over every store.  Every output     */
/*     texel depends on its inputs only: independent of scheduling and of   */
/*     the launch form.                                                     */
/* Launch form: one launch per level, 2 * levels - 1 in all, behind one     */
/* that clears the counters (ORBIT_BLOOM_FORCE_PER_LEVEL names it; it is    */
/* the only form built and the default).  A workgroup stages the source     */
/* texels its tile can touch in LDS, decoded, when they fit, and reads      */
/* global memory otherwise (a large filter_radius); ORBIT_BLOOM_FORCE_DIRECT*/
/* takes the second way everywhere: equal bytes.                            */
/* OUT OF SCOPE: hdr_resolve.frag (no MSAA in a visibility buffer; its      */
/* one-sample case writes vec4(1.0)); the skybox behind uncovered pixels    */
/* (they show whatever color holds); the sky light and textures;            */
/* render mode 7 and the depth-pyramid overlay; the fixed-point weights of  */
/* a hardware sampler.                                                      */
/*   ORBIT_E_INVALID  (message prefix bloom:) color or mips NULL, color not */
/*                    16-B or mips or stats not 4-B aligned; width or       */
/*                    height 0 or above ORBIT_RASTER_MAX_DIM; max_levels 0  */
/*                    or above 6; threshold, soft_threshold or              */
/*                    filter_radius negative or not finite; unknown flags;  */
/*                    mips equal to color.                                  */
/* Kernel launches only: no allocation, no scratch, no host wait; a graph   */
/* captures the call on a fresh context's first call.                       */
/*                                                                          */
/* orbit_post_process (post_process.frag) per pixel p:                      */
/*  T1 hdr = color[p].rgb: the blit's texture(image, in_uv) at a 1 : 1      */
/*     full-screen triangle is the texel itself; in_uv is the rasteriser's  */
/*     to interpolate, so the rule is a fetch.  render_mode == 0 and bloom  */
/*     != NULL: hdr += unpack(bloom[p]) * bloom_intensity (:59-64).         */
/*  T2 render_mode 8 takes the same path without bloom: the shader's `if    */
/*     (render_mode == 8)` assignment (:66) is overwritten by the else      */
/*     branch below it (:78-82).  Any other render_mode is ORBIT_E_INVALID  */
/*     (mode 7 and the depth-pyramid overlay are out of scope).             */
/*  T3 mapped = aces_hill(hdr * exposure) (:8-34): the two mat3 x vec3      */
/*     products column-major as R2's left-to-right rounded sums (m[0] * x + */
/*     m[3] * y) + m[6] * z; the fit a / b as written; then clamped to [0,  */
/*     1], NaN to 0.  ldr[p] = (mapped, 1.0f).                              */
/*  T4 rgba8[p] is the sRGB encoding a B8G8R8A8_SRGB attachment applies: c  */
/*     < 0.0031308f ? c * 12.92f : 1.055f * powc(c, 0.41666666f) - 0.055f;  */
/*     the byte is uint8(c * 255.0f + 0.5f); alpha 255; bytes in R, G, B, A */
/*     order, with ORBIT_POST_BGRA in the swapchain's B, G, R, A.  THE      */
/*     CONVERSION'S LAST BIT IS THE IMPLEMENTATION'S IN VULKAN: THIS IS THE */
/*     PROJECT'S CHOICE.  MEASURED: powc(x, 1 / 2.4) over [0.0031308, 1] is */
/*     within 2.71e-7 of float64; 3.9e-6 of the hand-built cases' bytes     */
/*     differ from the GLSL in float64, by 1.                               */
/*  T5 a non-finite hdr component, as fetched or after the bloom term,      */
/*     reads as +0.0f and the pixel counts in nonfinite_pixels.  stats (may */
/*     be NULL) is cleared by the call: pixels, nonfinite_pixels,           */
/*     bloom_pixels (pixels with a bloom term that is not 0).               */
/*   ORBIT_E_INVALID  (message prefix post_process:) color NULL; ldr and    */
/*                    rgba8 both NULL; color or ldr not 16-B, bloom, rgba8  */
/*                    or stats not 4-B aligned; width or height 0 or above  */
/*                    ORBIT_RASTER_MAX_DIM; render_mode not 0 or 8;         */
/*                    exposure or bloom_intensity not finite; unknown       */
/*                    flags; an output equal to an input or to the other.   */
/* One launch behind a clearing one; capturable on the first call.          */
/* ------------------------------------------------------------------------ */
#define ORBIT_BLOOM_MAX_LEVELS 6u       /* bloom.rs:9 */
#define ORBIT_BLOOM_FORCE_PER_LEVEL 1u  /* flags: one launch per level (the only form built) */
#define ORBIT_BLOOM_FORCE_DIRECT 4u     /* flags: every tap reads global memory, no LDS staging */
#define ORBIT_POST_BGRA 1u              /* flags: rgba8 in B, G, R, A order */
typedef struct OrbitBloomLayout { /* HOST, 88 B */
    uint32_t max_levels; /* IN: 1..6, 0 = 6 */
    uint32_t levels, total_texels, _pad;
    uint32_t level_width[ORBIT_BLOOM_MAX_LEVELS], level_height[ORBIT_BLOOM_MAX_LEVELS], level_offset[ORBIT_BLOOM_MAX_LEVELS]; /* 0 beyond levels */
} OrbitBloomLayout;
ORBIT_STATIC_ASSERT(sizeof(OrbitBloomLayout) == 88, "BloomLayout is 88 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitBloomLayout, level_width) == 16, "level_width @16");
ORBIT_STATIC_ASSERT(offsetof(OrbitBloomLayout, level_offset) == 64, "level_offset @64");
typedef struct OrbitBloomStats { /* DEVICE, 16 B, cleared by the call (B9) */
    uint32_t levels, texels_written, nonfinite_inputs, clamped_texels;
} OrbitBloomStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitBloomStats) == 16, "BloomStats is 16 B");
typedef struct OrbitBloom { /* HOST block, 56 B; every pointer a DEVICE pointer */
    const float *color;     /* width * height * 4 floats, 16-B aligned */
    uint32_t *mips;         /* OrbitBloomLayout.total_texels words */
    OrbitBloomStats *stats; /* NULL, or the counters */
    uint32_t width, height;
    float threshold, soft_threshold, filter_radius; /* BloomSettings, bloom.rs:12-17 */
    uint32_t max_levels;                            /* 1..6 */
    uint32_t flags, _pad;
} OrbitBloom;
ORBIT_STATIC_ASSERT(sizeof(OrbitBloom) == 56, "Bloom is 56 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitBloom, stats) == 16, "stats @16");
ORBIT_STATIC_ASSERT(offsetof(OrbitBloom, width) == 24, "width @24");
ORBIT_STATIC_ASSERT(offsetof(OrbitBloom, threshold) == 32, "threshold @32");
ORBIT_STATIC_ASSERT(offsetof(OrbitBloom, max_levels) == 44, "max_levels @44");
ORBIT_STATIC_ASSERT(offsetof(OrbitBloom, flags) == 48, "flags @48");
typedef struct OrbitPostStats { /* DEVICE, 16 B, cleared by the call (T5) */
    uint32_t pixels, nonfinite_pixels, bloom_pixels, _pad;
} OrbitPostStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitPostStats) == 16, "PostStats is 16 B");
typedef struct OrbitPostProcess { /* HOST block, 64 B; every pointer a DEVICE pointer */
    const float *color;    /* width * height * 4 floats, 16-B aligned */
    const uint32_t *bloom; /* NULL, or level 0 of orbit_bloom's mips */
    float *ldr;            /* NULL, or 4 floats per pixel, 16-B aligned */
    uint8_t *rgba8;        /* NULL, or 4 bytes per pixel, 4-B aligned */
    OrbitPostStats *stats; /* NULL, or the counters */
    float exposure, bloom_intensity;
    uint32_t render_mode; /* 0 or 8 */
    uint32_t width, height, flags;
} OrbitPostProcess;
ORBIT_STATIC_ASSERT(sizeof(OrbitPostProcess) == 64, "PostProcess is 64 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitPostProcess, stats) == 32, "stats @32");
ORBIT_STATIC_ASSERT(offsetof(OrbitPostProcess, exposure) == 40, "exposure @40");
ORBIT_STATIC_ASSERT(offsetof(OrbitPostProcess, render_mode) == 48, "render_mode @48");
ORBIT_STATIC_ASSERT(offsetof(OrbitPostProcess, flags) == 60, "flags @60");

/* B1's shape of a width x height target (host only; out->max_levels is read: 1..6, 0 = 6).  ORBIT_E_INVALID for a NULL
 * out, width or height 0 or above ORBIT_RASTER_MAX_DIM, max_levels above 6. */
int32_t orbit_bloom_layout(uint32_t width, uint32_t height, OrbitBloomLayout *out);
/* the reference's bloom chain of a colour plane into packed mips; see above */
int32_t orbit_bloom(OrbitCtx *ctx, const OrbitBloom *job, void *stream);
/* the reference's tone mapping and sRGB encoding of a colour plane; see above */
int32_t orbit_post_process(OrbitCtx *ctx, const OrbitPostProcess *job, void *stream);

/* ------------------------------------------------------------------------ */
/* orbit_ssao: the reference's screen-space ambient occlusion between its   */
/* depth prepass and its forward pass (app.rs:1151-1169;                    */
/* src/passes/ssao.rs, shaders/ssao/ssao.comp, shaders/ssao/ssao_blur.comp) */
/* and what forward.frag:335-338 reads of it per pixel.  It reads the depth */
/* plane orbit_raster_depth / orbit_visibility_resolve leave (floats,       */
/* reverse-z, 0 = uncovered) and the caller's two small tables.  ONE        */
/* definition for the device and the host mirror (orbit_host_ssao;          */
/* csrc/ssao_common.h); the two agree on every byte.  Arithmetic as in L /  */
/* B: fp32, every operation rounded on its own, never contracted, IEEE '/'  */
/* and sqrtf, GLSL max / clamp as x < y ? y : x; matrix x vector is R2's    */
/* left-to-right sums, dot is L's, normalize is F3's v / sqrtf(dot); cross, */
/* mix (a * (1 - t) + b * t) and smoothstep (t = clamp((x - e0) / (e1 -     */
/* e0), 0, 1); (t * t) * (3 - 2 * t)) are the GLSL specification's          */
/* formulas.                                                                */
/*  A1 positions (ssao.comp:51-71).  For a texel (px, py) of the ssao_w x   */
/*     ssao_h grid uv = (float(pixel) + 0.5f) * (1.0f / float(res)); depth  */
/*     = B3's LinearClamp sample of the full-size depth plane at uv;        */
/*     position = inverse_projection x (uv.x * 2 - 1, (1 - uv.y) * 2 - 1,   */
/*     depth, 1), xyz / w.  THE SHADER HOLDS pixel AS uvec2 (the binary     */
/*     converts it with OpConvertUToF in front of the + 0.5): the left      */
/*     neighbour of column 0 and the upper neighbour of row 0 are pixel     */
/*     0xFFFFFFFF, which converts to 2^32; its uv clamps to the far edge    */
/*     and its x / y are enormous.  THIS IS THE REFERENCE'S BEHAVIOUR AND   */
/*     IS KEPT: it decides the normal of column 0 and row 0.  Texels at or  */
/*     beyond res are positions like any other and write nothing.           */
/*  A2 the normal (:78-115).  With the centre p0 and the right, left, down, */
/*     up neighbours: horizontal = |right.z - p0.z| < |left.z - p0.z| ?     */
/*     right : left, vertical = |down.z - p0.z| < |up.z - p0.z| ? down : up */
/*     (a tie takes left / up); (p1, p2) = (right, up), (down, right), (up, */
/*     left) or (left, down) as the shader's four branches have them;       */
/*     normal = normalize(cross(p2 - p0, p1 - p0)).                         */
/*  A3 noise (:120-127), NearestRepeat: u = float(gid) / float(noise_size)  */
/*     per axis of the SSAO pixel gid; the texel is floor(u *               */
/*     float(noise_size)) wrapped into [0, noise_size); a snorm8 byte b     */
/*     reads as max(b / 127.0f, -1).  random_vec = normalize((n.x, n.y,     */
/*     0)); tangent = normalize(random_vec - normal * dot(random_vec,       */
/*     normal)); bitangent = cross(normal, tangent).  A (0, 0) noise texel  */
/*     makes them NaN, as in the shader; then every sample's proj is NaN    */
/*     and fails A5's range test, nothing is added and THE BYTE IS 255, NOT */
/*     0: the pixel does not count in nonfinite_pixels.                     */
/*  A4 per sample i (:134-141), independent of the pixel: fi = float(i) /   */
/*     float(sample_count); the 1-D NearestRepeat texel floor(fi *          */
/*     float(samples_size)) mod samples_size, as unorm8 / 255.0f, of which  */
/*     only .z is used; hammersley_2d as written (the bit reversal,         */
/*     float(bits) * 2.3283064365386963e-10f); hemispherepoint_uniform(fi,  */
/*     rdi): phi = (rdi * 2) * PI, cosTheta = 1 - fi, sinTheta = sqrtf(1 -  */
/*     cosTheta * cosTheta), (cos(phi) * sinTheta, sin(phi) * sinTheta,     */
/*     cosTheta) with H6's sine and cosine, whose domain [0, 2 pi] covers   */
/*     phi; radius = mix(min_radius, max_radius, z * z).                    */
/*  A5 the test (:140-154).  cone = (tangent * h.x + bitangent * h.y) +     */
/*     normal * h.z; sample_point = p0 - cone * radius; proj = projection x */
/*     (sample_point, 1); xyz /= w; xy = xy * (0.5, -0.5) + 0.5.  A sample  */
/*     is in range iff all three components equal their clamp to [0, 1]     */
/*     (NaN fails).  In-range samples read sample_depth by B3 at proj.xy;   */
/*     sample_depth_lin = 0.01f / sample_depth (the literal is the          */
/*     shader's, not the camera's near plane); range_check = smoothstep(0,  */
/*     1, min_radius / abs(sample_depth_lin - proj.w)); occlusion +=        */
/*     (sample_depth >= proj.z ? 1 : 0) * range_check, in sample order.     */
/*  A6 the store.  occlusion = 1 - occlusion / float(sample_count); the R8  */
/*     byte is uint8(clamp(c, 0, 1) * 255.0f + 0.5f), T4's byte rule.  NaN  */
/*     stores 0 and counts in nonfinite_pixels (it arises from range_check: */
/*     min_radius 0 and a sample at its own surface is 0 / 0); nothing else */
/*     non-finite can reach a byte.  VULKAN LEAVES THE CONVERSION'S LAST    */
/*     BIT TO THE IMPLEMENTATION: THIS IS THE PROJECT'S CHOICE.             */
/*  A7 the blur (ssao_blur.comp).  The four textureGather calls are at      */
/*     (float(pixel) + 0.5f - off) / float(size), off = (0, 0), (2, 0), (0, */
/*     2), (2, 2): a division, as written.  Each returns the four texels of */
/*     B3's footprint, i0 = floor(u * W - 0.5f), i0 and i0 + 1 clamped, in  */
/*     the order x = (i0, j1), y = (i1, j1), z = (i1, j0), w = (i0, j0);    */
/*     texels read as byte / 255.0f.  The sums are the two levels of dot(., */
/*     vec4(1)), left to right, then * 0.0625f, then A6's byte.  THE        */
/*     GATHERS SIT EXACTLY ON TEXEL CENTRES, WHERE A HARDWARE FOOTPRINT IS  */
/*     IMPLEMENTATION-DEFINED: fp32 AS WRITTEN, WITH THE floor IT YIELDS,   */
/*     IS THIS PROJECT'S CHOICE, as B3 is.                                  */
/*  A8 the fragment read (forward.frag:336-337).  ao_pixel[p] = B3's sample */
/*     of blurred (byte / 255.0f) at (float(x) + 0.5f, float(y) + 0.5f) /   */
/*     float(screen) for every screen pixel.  min with the material's ao is */
/*     the consumer's.                                                      */
/*  A9 stats (may be NULL) is cleared by the call: pixels = ssao_w *        */
/*     ssao_h, nonfinite_pixels, unoccluded_pixels (raw byte 255) and the   */
/*     64-bit samples_in_range.  Every output depends on its own pixel and  */
/*     the inputs only: independent of scheduling and of how the kernel     */
/*     tiles the target.                                                    */
/* Outputs: raw (ssao.comp's R8 image), blurred (ssao_blur.comp's, which    */
/* the frame uses), ao_pixel (A8); each may be NULL, not all; blurred needs */
/* raw and ao_pixel needs blurred: the call has no scratch.  Launches: one  */
/* that clears the counters, the SSAO launch (a workgroup takes a 16 x 16   */
/* tile and stages its bordered tile of positions and A4's table in LDS),   */
/* the blur and the fragment read, ordered by the stream.                   */
/* OUT OF SCOPE: the sky-light term (forward.frag:404) and render mode 6    */
/* (:561) that consume ao (cube maps, the BRDF table); the material's       */
/* occlusion texture; a hardware sampler's fixed-point weights and gather   */
/* footprint.                                                               */
/*   ORBIT_E_INVALID  (message prefix ssao:) depth, noise or samples NULL;  */
/*                    every output NULL; blurred without raw or ao_pixel    */
/*                    without blurred; depth, ao_pixel or samples not 4-B,  */
/*                    noise not 2-B, stats not 8-B aligned; a size 0 or     */
/*                    above ORBIT_RASTER_MAX_DIM, ssao above screen;        */
/*                    noise_size outside 1..64, samples_size outside        */
/*                    1..256, sample_count outside 1..64; a radius negative */
/*                    or not finite; flags not 0; an output equal to an     */
/*                    input or to another output.  As in the sibling calls  */
/*                    the check compares the pointers only: ranges that     */
/*                    overlap without starting at one address are the       */
/*                    caller's to avoid, and their result is undefined.     */
/* Kernel launches only: no allocation, no scratch, no host wait; a graph   */
/* captures the call on a fresh context's first call.                       */
/* ------------------------------------------------------------------------ */
#define ORBIT_SSAO_MAX_SAMPLES 64u       /* sample_count: the UI's range, ssao.rs:31 */
#define ORBIT_SSAO_MAX_NOISE_SIZE 64u    /* noise_size */
#define ORBIT_SSAO_MAX_SAMPLES_SIZE 256u /* samples_size */
typedef struct OrbitSsaoStats { /* DEVICE, 24 B, 8-B aligned, cleared by the call (A9) */
    uint32_t pixels, nonfinite_pixels, unoccluded_pixels, _pad;
    uint64_t samples_in_range;
} OrbitSsaoStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitSsaoStats) == 24, "SsaoStats is 24 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitSsaoStats, samples_in_range) == 16, "samples_in_range @16");
typedef struct OrbitSsao { /* HOST block, 224 B; every pointer a DEVICE pointer */
    const float *depth;     /* screen_w * screen_h floats, reverse-z, 0 = uncovered */
    const int8_t *noise;    /* noise_size * noise_size pairs (R8G8_SNORM), 2-B aligned */
    const uint8_t *samples; /* samples_size * 4 bytes (R8G8B8A8_UNORM), 4-B aligned */
    uint8_t *raw;           /* NULL, or ssao_w * ssao_h bytes */
    uint8_t *blurred;       /* NULL, or ssao_w * ssao_h bytes; needs raw */
    float *ao_pixel;        /* NULL, or screen_w * screen_h floats; needs blurred */
    OrbitSsaoStats *stats;  /* NULL, or the counters */
    float projection[16], inverse_projection[16]; /* column-major, GpuSSAOInfo's two (ssao.rs:50-53) */
    uint32_t screen_w, screen_h;
    uint32_t ssao_w, ssao_h; /* the screen's, or each / 2 (ssao.rs:93-97); any 1 <= ssao <= screen */
    uint32_t noise_size, samples_size, sample_count;
    float min_radius, max_radius; /* SsaoSettings, ssao.rs:9-25 */
    uint32_t flags;               /* 0 */
} OrbitSsao;
ORBIT_STATIC_ASSERT(sizeof(OrbitSsao) == 224, "Ssao is 224 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitSsao, raw) == 24, "raw @24");
ORBIT_STATIC_ASSERT(offsetof(OrbitSsao, stats) == 48, "stats @48");
ORBIT_STATIC_ASSERT(offsetof(OrbitSsao, projection) == 56, "projection @56");
ORBIT_STATIC_ASSERT(offsetof(OrbitSsao, inverse_projection) == 120, "inverse_projection @120");
ORBIT_STATIC_ASSERT(offsetof(OrbitSsao, screen_w) == 184, "screen_w @184");
ORBIT_STATIC_ASSERT(offsetof(OrbitSsao, noise_size) == 200, "noise_size @200");
ORBIT_STATIC_ASSERT(offsetof(OrbitSsao, min_radius) == 212, "min_radius @212");
ORBIT_STATIC_ASSERT(offsetof(OrbitSsao, flags) == 220, "flags @220");

/* the reference's SSAO, its blur and forward.frag's read of it per pixel; see above */
int32_t orbit_ssao(OrbitCtx *ctx, const OrbitSsao *job, void *stream);

/* ------------------------------------------------------------------------ */
/* orbit_env_map: the images the reference computes once at load time for   */
/* its sky light (src/passes/env_map_loader.rs, forward.rs:113-205): the    */
/* sky cube with its mip chain from an equirectangular panorama, the        */
/* irradiance cube, the prefiltered cube and the BRDF integration table.    */
/* orbit_env_sample is the cube sampler of rule E4 made public.  ONE        */
/* definition for the device and the host mirror (orbit_host_env_map,       */
/* orbit_host_env_sample; csrc/env_common.h); the two agree on every byte.  */
/* Arithmetic as in L / B / A: fp32, every operation rounded on its own, no */
/* contraction, IEEE / and sqrtf, normalize / cross / clamp by the GLSL     */
/* formulas, pow = B5's powc, log2 = L2's log2c.  DESIGN.md §4.30.          */
/*                                                                          */
/*  E0 storage.  A cube level is six faces of n x n texels of               */
/*     R16G16B16A16_SFLOAT (8 B), face-major, faces in Vulkan's layer order */
/*     +X -X +Y -Y +Z -Z, rows top to bottom.  Level m of a cube of size n  */
/*     has extent max(1, n >> m); levels are concatenated, level 0 first    */
/*     (orbit_env_map_layout).  The BRDF table is n x n texels of           */
/*     R16G16_SFLOAT (4 B).  fp32 -> fp16 rounds to nearest, ties to even   */
/*     (a project choice: Vulkan allows either); a finite value at or above */
/*     65520 in magnitude stores +-65504 (E10); a non-finite value stores   */
/*     +0 and its texel is counted (E8).  Alpha is 1.                       */
/*  E1 texel -> direction.  cx = (2.0f * (float(px) + 0.5f)) / float(n) -   */
/*     1.0f, cy = 1.0f - (2.0f * (float(py) + 0.5f)) / float(n), and        */
/*     in_local_pos = transpose(V) * (cx, cy, 1) of the layer's look_at_rh  */
/*     matrix V (the loader pushes the bare view matrix: w = 1, the draw is */
/*     orthographic, the clip removes view z < 0 and the viewport's height  */
/*     is negative), which is per layer                                     */
/*       0 (-1, cy, cx)   1 (1, cy, -cx)    2 (-cx, 1, cy)                  */
/*       3 (-cx, -1, -cy) 4 (-cx, cy, -1)   5 (cx, cy, 1)                   */
/*     Against Vulkan's face table this is the direction rotated by 180     */
/*     degrees about Y: the reference's behaviour, kept.                    */
/*  E2 equirect fetch (equirectangular_cube_map.frag).  v = normalize(      */
/*     in_local_pos); u.x = atan2c(v.z, v.x) * 0.1591f + 0.5f, u.y = 1.0f - */
/*     (asinc(v.y) * 0.3183f + 0.5f); LinearRepeat bilinear of level 0 of   */
/*     the caller's fp32 RGBA panorama: s = u * size - 0.5f, floor, the two */
/*     texel indices by integer remainder on both axes, B3's weights; then  */
/*     clamp(rgb, 0, 10000) by the GLSL formula (NaN stays NaN: E0).  The   */
/*     panorama's own mips are not read (a project choice).                 */
/*  E3 sky mips.  Level m + 1 texel = ((t00 + t10) + (t01 + t11)) * 0.25f   */
/*     of the 2 x 2 block of level m read back from its stored fp16, all    */
/*     four channels.  sky_size is a power of two in 1 .. 4096; the chain   */
/*     is full: log2(sky_size) + 1 levels.                                  */
/*  E4 the cube sampler.  A direction with a non-finite component or all    */
/*     three zero returns 0 and is counted.  The face is Vulkan's: z wins   */
/*     ties over y and x, y over x; sc, tc, ma by the specification's       */
/*     table; s = (0.5f * sc) / |ma| + 0.5f, t alike.  Per level of extent  */
/*     n: x = s * n - 0.5f, i0 = floor(x), f = x - i0, i1 = i0 + 1 (both in */
/*     -1 .. n), B3's expression (t00 * (1 - fx) + t10 * fx) * (1 - fy) +   */
/*     (t01 * (1 - fx) + t11 * fx) * fy.  Seamless: a tap outside the face  */
/*     in one axis is the texel of the adjoining face across that edge; a   */
/*     tap outside in both axes is ((own + across x) + across y) / 3.0f of  */
/*     the three corner texels.  lod: NaN and negative -> 0, above levels - */
/*     1 -> levels - 1; l = floor(lod), f = lod - l; f == 0 reads level l   */
/*     alone, else a * (1.0f - f) + b * f of levels l and l + 1.            */
/*  E5 irradiance (cubemap_convolution.frag) as written: the two float loop */
/*     counters advanced by fp32 += sample_delta against 2.0f * PI and 0.5f */
/*     * PI; sampleVec = (x * right + y * up) + z * in_local_pos, the       */
/*     unnormalised position; irradiance += (rgb * cos(theta)) * sin(theta);*/
/*     (PI * irradiance) * (1.0f / nrSamples).  The lod of every tap is one */
/*     constant per call, max(0, log2c(float(sky_size) / float(             */
/*     irradiance_size))) (a project choice).  At an odd size the texel at  */
/*     (0, +-1, 0) has a NaN frame: every tap is a bad direction by E4, the */
/*     texel stores 0 and bad_directions counts its taps.                   */
/*  E6 prefilter (environmental_map_prefilter.frag, functions.glsl) as      */
/*     written, level m of extent max(1, n >> m) at roughness float(m) /    */
/*     float(levels - 1) (0 when levels == 1): hammersley_2d,               */
/*     importance_sample_ggx with phi = (2.0f * PI) * Xi.x + random(        */
/*     normal.xz) * 0.1f, random's mod(dt, 3.14f) = dt - 3.14f * floor(dt / */
/*     3.14f) and fract(x) = x - floor(x); L = (2.0f * dot(V, H)) * H - V;  */
/*     pdf = (D * dotNH) / (4.0f * dotVH) + 0.0001f; omegaS = 1.0f / (float(*/
/*     sample_count) * pdf); omegaP = (4.0f * PI) / ((6.0f * dim) * dim)    */
/*     with dim = float(sky_size); mip = roughness == 0 ? 0 : max(0.5f *    */
/*     log2c(omegaS / omegaP) + 1.0f, 0); color / totalWeight (0 / 0 = NaN: */
/*     E0).  Sine and cosine are H6's routine, which holds on [-pi/4, 2 pi  */
/*     + pi/4] (phi reaches 2 pi + 0.1).                                    */
/*  E7 BRDF table (brdf_integration.frag) as written, with its own          */
/*     importance_sample_ggx and geometry_smith.  Texel (x, y) has in_uv =  */
/*     ((x + 0.5f) / n, (y + 0.5f) / n): blit.vert's uv.y = 1 - y and the   */
/*     negative viewport height cancel.  R = A, G = B.                      */
/*  E8 stats (may be NULL) is cleared by the call: per product the texels   */
/*     with a non-finite channel, and the bad directions of E4 over every   */
/*     tap of the call.                                                     */
/*  E9 ORBIT_E_INVALID (message prefix env_map: / env_sample:) for a NULL   */
/*     job; unknown flags; no product asked for; a product's size 0 or      */
/*     above ORBIT_ENV_MAX_SIZE; a sky size that is not a power of two;     */
/*     prefiltered_levels 0 or above ORBIT_ENV_MAX_LEVELS; sample_count or  */
/*     brdf_sample_count 0 or above ORBIT_ENV_MAX_SAMPLES where its product */
/*     is made; sample_delta non-finite or below 0.005f, which covers <= 0  */
/*     (a thread runs its texel's trips one after the other: 0.005 is 1 257 */
/*     x 315 of them, 25 times the reference's, and bounds the launch; a    */
/*     step below fp32's spacing at 2 pi would never end the loop);         */
/*     irradiance or prefiltered without a sky cube; an equirect of width   */
/*     or height 0 or above 65 536; a plane not aligned (equirect 16 B,     */
/*     cubes and stats 8 B, table 4 B); two of the call's buffers sharing a */
/*     byte, by the sizes the layout call gives (for the sample call: rgb   */
/*     or the counter sharing a byte with the cube, the directions, the     */
/*     lods or each other).  A NULL context.                                */
/* E10 a finite value beyond fp16's range stores the largest finite fp16.   */
/* E11 the distance of every product from the GLSL in float64 is measured,  */
/*     not bounded (tools/count_env_map.py, profiles/env_map_cpu.json).     */
/* E12 abs(N.z) < 0.999 compares against the fp32 literal 0.999f.           */
/*                                                                          */
/* Each product is optional (NULL: not made).  With equirect the sky cube   */
/* is written and then read by the later products; with equirect NULL the   */
/* caller's sky cube (all its levels, E0) is read.  Launches: one clears    */
/* the counters, one per sky face set, one per sky mip, one for the         */
/* irradiance cube, one per prefiltered level (a 256-thread workgroup takes */
/* a 16 x 16 tile of one face; what depends on the sample alone is staged   */
/* through LDS in chunks of 256 samples), one for the table.  No            */
/* allocation, no host sync: capturable on the first call.                  */
/* ------------------------------------------------------------------------ */
#define ORBIT_ENV_MAX_SIZE 4096u     /* every cube's and the table's largest size */
#define ORBIT_ENV_MAX_LEVELS 13u     /* log2(4096) + 1 */
#define ORBIT_ENV_MAX_SAMPLES 65536u /* sample_count, brdf_sample_count */
typedef struct OrbitEnvMapLayout { /* HOST, 264 B; sizes and offsets in texels */
    uint32_t sky_size, sky_levels, irradiance_size, prefiltered_size, prefiltered_levels, brdf_size;
    uint32_t sky_level_size[ORBIT_ENV_MAX_LEVELS], sky_level_offset[ORBIT_ENV_MAX_LEVELS]; /* 0 beyond sky_levels */
    uint32_t prefiltered_level_size[ORBIT_ENV_MAX_LEVELS], prefiltered_level_offset[ORBIT_ENV_MAX_LEVELS];
    uint64_t sky_texels, irradiance_texels, prefiltered_texels; /* 8-B texels */
    uint64_t brdf_texels;                                       /* 4-B texels */
} OrbitEnvMapLayout;
ORBIT_STATIC_ASSERT(sizeof(OrbitEnvMapLayout) == 264, "EnvMapLayout is 264 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, sky_size) == 0, "sky_size @0");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, sky_levels) == 4, "sky_levels @4");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, irradiance_size) == 8, "irradiance_size @8");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, prefiltered_size) == 12, "prefiltered_size @12");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, prefiltered_levels) == 16, "prefiltered_levels @16");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, brdf_size) == 20, "brdf_size @20");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, sky_level_size) == 24, "sky_level_size @24");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, sky_level_offset) == 76, "sky_level_offset @76");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, prefiltered_level_size) == 128, "prefiltered_level_size @128");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, prefiltered_level_offset) == 180, "prefiltered_level_offset @180");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, sky_texels) == 232, "sky_texels @232");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, irradiance_texels) == 240, "irradiance_texels @240");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, prefiltered_texels) == 248, "prefiltered_texels @248");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapLayout, brdf_texels) == 256, "brdf_texels @256");
typedef struct OrbitEnvMapStats { /* DEVICE, 48 B, 8-B aligned, cleared by the call (E8) */
    uint64_t sky_nonfinite, irradiance_nonfinite, prefiltered_nonfinite, brdf_nonfinite, bad_directions, _pad;
} OrbitEnvMapStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitEnvMapStats) == 48, "EnvMapStats is 48 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapStats, sky_nonfinite) == 0, "sky_nonfinite @0");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapStats, irradiance_nonfinite) == 8, "irradiance_nonfinite @8");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapStats, prefiltered_nonfinite) == 16, "prefiltered_nonfinite @16");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapStats, brdf_nonfinite) == 24, "brdf_nonfinite @24");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapStats, bad_directions) == 32, "bad_directions @32");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMapStats, _pad) == 40, "_pad @40");
typedef struct OrbitEnvMap { /* HOST block, 96 B; every pointer a DEVICE pointer */
    const float *equirect;   /* NULL (sky is the caller's), or equirect_w * equirect_h * 4 floats, 16-B aligned */
    uint16_t *sky;           /* NULL, or OrbitEnvMapLayout.sky_texels * 4 halves: written with equirect, else read */
    uint16_t *irradiance;    /* NULL, or irradiance_texels * 4 halves */
    uint16_t *prefiltered;   /* NULL, or prefiltered_texels * 4 halves */
    uint16_t *brdf;          /* NULL, or brdf_texels * 2 halves */
    OrbitEnvMapStats *stats; /* NULL, or the counters */
    uint32_t equirect_w, equirect_h;
    uint32_t sky_size, irradiance_size, prefiltered_size, prefiltered_levels, brdf_size; /* the layout call's */
    uint32_t sample_count;      /* E6; the reference: 4096 */
    float sample_delta;         /* E5; the reference: 0.025 */
    uint32_t brdf_sample_count; /* E7; the reference: 1024 */
    uint32_t flags, _pad;       /* 0 */
} OrbitEnvMap;
ORBIT_STATIC_ASSERT(sizeof(OrbitEnvMap) == 96, "EnvMap is 96 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, equirect) == 0, "equirect @0");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, sky) == 8, "sky @8");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, irradiance) == 16, "irradiance @16");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, prefiltered) == 24, "prefiltered @24");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, brdf) == 32, "brdf @32");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, stats) == 40, "stats @40");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, equirect_w) == 48, "equirect_w @48");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, equirect_h) == 52, "equirect_h @52");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, sky_size) == 56, "sky_size @56");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, irradiance_size) == 60, "irradiance_size @60");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, prefiltered_size) == 64, "prefiltered_size @64");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, prefiltered_levels) == 68, "prefiltered_levels @68");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, brdf_size) == 72, "brdf_size @72");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, sample_count) == 76, "sample_count @76");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, sample_delta) == 80, "sample_delta @80");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, brdf_sample_count) == 84, "brdf_sample_count @84");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, flags) == 88, "flags @88");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvMap, _pad) == 92, "_pad @92");
typedef struct OrbitEnvSample { /* HOST block, 56 B; every pointer a DEVICE pointer */
    const uint16_t *cube;     /* a cube in E0's layout, 8-B aligned */
    const float *directions;  /* n * 3 floats */
    const float *lods;        /* n floats */
    float *rgb;               /* n * 3 floats */
    uint64_t *bad_directions; /* NULL, or one counter, cleared by the call */
    uint32_t size, levels;    /* the cube's: level m has extent max(1, size >> m) */
    uint32_t n, flags;        /* flags: 0 */
} OrbitEnvSample;
ORBIT_STATIC_ASSERT(sizeof(OrbitEnvSample) == 56, "EnvSample is 56 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvSample, cube) == 0, "cube @0");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvSample, directions) == 8, "directions @8");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvSample, lods) == 16, "lods @16");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvSample, rgb) == 24, "rgb @24");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvSample, bad_directions) == 32, "bad_directions @32");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvSample, size) == 40, "size @40");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvSample, levels) == 44, "levels @44");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvSample, n) == 48, "n @48");
ORBIT_STATIC_ASSERT(offsetof(OrbitEnvSample, flags) == 52, "flags @52");

/* E0's shape (host only).  A size of 0 leaves its product out (its fields 0).  ORBIT_E_INVALID for a NULL out, a size
 * above ORBIT_ENV_MAX_SIZE, a sky size that is not a power of two, prefiltered_levels 0 (with a prefiltered size) or above
 * ORBIT_ENV_MAX_LEVELS. */
int32_t orbit_env_map_layout(uint32_t sky_size, uint32_t irradiance_size, uint32_t prefiltered_size, uint32_t prefiltered_levels,
                             uint32_t brdf_size, OrbitEnvMapLayout *out);
/* the sky cube, the irradiance cube, the prefiltered cube and the BRDF table; see above */
int32_t orbit_env_map(OrbitCtx *ctx, const OrbitEnvMap *job, void *stream);
/* E4 of n directions and lods of a cube in E0's layout (size 1 .. ORBIT_ENV_MAX_SIZE, levels 1 .. ORBIT_ENV_MAX_LEVELS);
 * n == 0 is a call that only clears the counter */
int32_t orbit_env_sample(OrbitCtx *ctx, const OrbitEnvSample *job, void *stream);

/* ------------------------------------------------------------------------ */
/* The sky light's term and the skybox.  orbit_fragments_shade_sky is       */
/* orbit_fragments_shade_shadowed with two additions: L5's SKY branch is    */
/* served (forward.frag:378-405) from the images orbit_env_map writes, and  */
/* the uncovered pixels are filled from the sky cube (skybox.vert /         */
/* skybox.frag, forward.rs:471-472, 629-682).  ONE definition for the       */
/* device and the host mirror (orbit_host_fragments_shade_sky,              */
/* csrc/sky_common.h); the two agree on every byte.  The job starts with an */
/* OrbitFragmentsShadeShadowed: same meaning, same checks.  Arithmetic as   */
/* in L: fp32, every operation rounded on its own, never contracted, IEEE   */
/* '/', GLSL max / min / clamp by their formulas, dot as L's left-to-right  */
/* sum.  The irradiance cube, the prefiltered cube and the BRDF table are   */
/* THE ENVIRONMENT: given together or not at all.  DESIGN.md §4.31.         */
/*  K1 which lights.  With the environment given, a SKY light of a pixel's  */
/*     walk is evaluated in list position, as often as it occurs, and no    */
/*     longer counts the pixel in unserved_pixels.  With the environment    */
/*     NULL it is skipped and counted exactly as by the shadowed call.  The */
/*     light's irradiance_map_index and prefiltered_map_index are not read: */
/*     a call has one environment, as the reference has one                 */
/*     environment_map.                                                     */
/*  K2 the reflection vector.  R = V - (2 * dot(N, V)) * N: GLSL            */
/*     reflect(view_direction, normal) with the view direction as the       */
/*     incident vector, the reference's expression, kept.  Then R.y = R.y * */
/*     -1.                                                                  */
/*  K3 Fresnel with roughness.  ndv0 = max(dot(N, V), 0); f0 is L6's; x =   */
/*     clamp(1 - ndv0, 0, 1); p5 = ((x * x) * (x * x)) * x (L6's choice for */
/*     pow(., 5)); kS_c = f0_c + (max(1 - roughness, f0_c) - f0_c) * p5;    */
/*     kD_c = (1 - kS_c) * (1 - metallic).                                  */
/*  K4 diffuse.  irr = E4's sample of the irradiance cube (one level) at N, */
/*     lod 0, the seamless fold and the corner mean included; diffuse_c =   */
/*     irr_c * base_c.                                                      */
/*  K5 reflection.  lod = roughness * float(prefiltered_levels - 1); refl = */
/*     E4's sample of the prefiltered cube at R and lod (E4 clamps NaN,     */
/*     negative and too-large lods).                                        */
/*  K6 the BRDF table.  env = table(ndv0, roughness) under the reference's  */
/*     default LinearClamp sampler: per axis s = u * n - 0.5, i0 = floor(s),*/
/*     f = s - i0, i1 = i0 + 1; both indices converted saturating with NaN  */
/*     -> 0 and clamped to [0, n - 1]; B3's expression (t00 * (1 - fx) +    */
/*     t10 * fx) * (1 - fy) + (t01 * (1 - fx) + t11 * fx) * fy on the       */
/*     stored fp16 pair.  u = ndv0 indexes a row's texels, v = roughness    */
/*     the rows (E7).                                                       */
/*  K7 the term.  spec_c = refl_c * (kS_c * env.x + env.y); term_c = ((kD_c */
/*     * diffuse_c + spec_c) * lc_c) * ao, lc = color * intensity as in L5; */
/*     light_sum_c = light_sum_c + term_c.                                  */
/*  K8 ambient occlusion.  ao = 1.0f with the plane NULL; otherwise min(    */
/*     1.0f, ao[p]) by GLSL's min (y < x ? y : x: NaN gives 1): what        */
/*     orbit_ssao writes as ao_pixel.  ao scales the sky term only, as in   */
/*     the shader.  Occlusion textures are not served and are counted in    */
/*     textured_pixels as before.                                           */
/*  K9 the skybox.  With sky given and render_mode 0, a pixel whose         */
/*     visibility word is 0 (the reference's EQUAL test against the cleared */
/*     reverse-z depth at gl_Position.z = 0) gets color[p] = (E4's sample   */
/*     of the sky cube at normalize(d) and skybox_lod, 1.0f), d = (cx *     */
/*     sky_x + cy * sky_y) + sky_z per component, cx = (2 * (x + 0.5)) /    */
/*     width - 1, cy = 1 - (2 * (y + 0.5)) / height (the sign follows the   */
/*     negative viewport height, as in E1).  The caller derives the basis   */
/*     from skybox_view_projection_matrix; for the reference's              */
/*     perspective_infinite_reverse_rh camera with orientation R: sky_x = R */
/*     e_x / P00, sky_y = R e_y / P11, sky_z = -R e_z                       */
/*     (orbit_host_skybox_basis).  TWO PROJECT CHOICES: the ray is          */
/*     evaluated at the pixel centre, and the lod is one constant per call  */
/*     where the shader's implicit lod depends on the driver's derivatives  */
/*     (E5's choice).  A bad direction (E4) stores 0 and is counted.        */
/*     Covered pixels are never touched by K9.  With sky NULL, or in        */
/*     render_mode 8, uncovered pixels are left as by the shadowed call.    */
/* K10 everything else.  L8 (no non-finite bytes), L9 and H1-H10 hold       */
/*     unchanged; every output depends on its own pixel only.  With the     */
/*     environment NULL and sky NULL, color, lights_walked, shadow_factor,  */
/*     cascade and all stats equal orbit_fragments_shade_shadowed's byte    */
/*     for byte.  In render_mode 8 nothing of K is evaluated.  sky_stats,   */
/*     cleared by the call: sky_evaluations = SKY lights evaluated over     */
/*     written pixels; sky_lit_pixels = written pixels with at least one;   */
/*     skybox_pixels = pixels K9 wrote; bad_directions = E4's bad           */
/*     directions over every cube sample of the call (K4, K5 and K9; those  */
/*     of K4 / K5 over written pixels).                                     */
/* OUT OF SCOPE: material textures, occlusion textures included; render     */
/* modes 1-7 and 9; MSAA and hdr_resolve; an orthographic camera's skybox;  */
/* more than one environment per call; a hardware sampler's fixed-point     */
/* weights; derivative-driven lod for the skybox.                           */
/*   ORBIT_E_INVALID  (message prefix fragments_shade_sky:) everything      */
/*                    orbit_fragments_shade_shadowed rejects; an            */
/*                    environment given only in part; a size of 0 or above  */
/*                    ORBIT_ENV_MAX_SIZE; prefiltered_levels or sky_levels  */
/*                    of 0 or above ORBIT_ENV_MAX_LEVELS; a cube or         */
/*                    sky_stats not 8-B aligned, the table or ao not 4-B    */
/*                    aligned; a non-finite skybox_lod; an output sharing a */
/*                    byte with an input, by the ranges the sizes give.     */
/*                    All checked before the context is looked at, by the   */
/*                    function the mirror uses.                             */
/* Kernel launches only: no allocation, no scratch, no host wait; a graph   */
/* captures the call on a fresh context's first call.                       */
/* ------------------------------------------------------------------------ */
typedef struct OrbitSkyStats { /* DEVICE, 32 B, 8-B aligned, cleared by the call (K10) */
    uint32_t sky_evaluations, sky_lit_pixels, skybox_pixels, _pad;
    uint64_t bad_directions, _pad2;
} OrbitSkyStats;
ORBIT_STATIC_ASSERT(sizeof(OrbitSkyStats) == 32, "SkyStats is 32 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitSkyStats, skybox_pixels) == 8, "skybox_pixels @8");
ORBIT_STATIC_ASSERT(offsetof(OrbitSkyStats, bad_directions) == 16, "bad_directions @16");
typedef struct OrbitFragmentsShadeSky { /* HOST block, 344 B; every pointer a DEVICE pointer */
    OrbitFragmentsShadeShadowed shadowed; /* as orbit_fragments_shade_shadowed takes it */
    const uint16_t *irradiance;           /* NULL, or level 0 of a cube in E0's layout, 8-B aligned */
    const uint16_t *prefiltered;          /* NULL, or prefiltered_levels levels in E0's layout, 8-B aligned */
    const uint16_t *brdf;                 /* NULL, or brdf_size^2 R16G16_SFLOAT texels, 4-B aligned */
    const uint16_t *sky;                  /* NULL (no skybox), or sky_levels levels in E0's layout, 8-B aligned */
    const float *ao;                      /* NULL, or 1 float per pixel (orbit_ssao's ao_pixel) */
    OrbitSkyStats *sky_stats;             /* NULL, or the counters */
    uint32_t irradiance_size, prefiltered_size, prefiltered_levels, brdf_size;
    uint32_t sky_size, sky_levels;
    float skybox_lod;
    float sky_x[3], sky_y[3], sky_z[3]; /* K9's ray basis */
} OrbitFragmentsShadeSky;
ORBIT_STATIC_ASSERT(sizeof(OrbitFragmentsShadeSky) == 344, "FragmentsShadeSky is 344 B");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeSky, irradiance) == 232, "irradiance @232");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeSky, sky) == 256, "sky @256");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeSky, sky_stats) == 272, "sky_stats @272");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeSky, irradiance_size) == 280, "irradiance_size @280");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeSky, sky_size) == 296, "sky_size @296");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeSky, skybox_lod) == 304, "skybox_lod @304");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeSky, sky_x) == 308, "sky_x @308");
ORBIT_STATIC_ASSERT(offsetof(OrbitFragmentsShadeSky, sky_z) == 332, "sky_z @332");

/* forward.frag's clustered lighting with shadows, the sky light's term and the skybox; see above */
int32_t orbit_fragments_shade_sky(OrbitCtx *ctx, const OrbitFragmentsShadeSky *job, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ORBIT_ABI_EXT_H */
