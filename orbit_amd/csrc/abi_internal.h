// abi_internal.h — what the translation units of the C ABI (abi_*.hip, include/orbit_abi.h) share: the context and
// meshlet-stream objects, the error reporting, and the helpers one unit defines and another calls.  Nothing declared
// here is exported from liborbit_cull.so (hidden visibility); the exported names are include/orbit_abi.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "block_pretest.h"
#include "kernels.h"

using namespace orbit;

#pragma GCC visibility push(hidden)

// orbit_meshlet_stream_*: derived arrays of meshlets [first, first + capacity) of the buffer at `source`
struct OrbitMeshletStream {
    int device = 0;
    uint64_t first = 0, capacity = 0;
    uint4 *sphere = nullptr;
    uint32_t *cone = nullptr;
    uint16_t *mat = nullptr;
    uint32_t *cmd = nullptr;
    uint16_t *cnt = nullptr;
    uint32_t *link = nullptr, *cls0 = nullptr, *cls1 = nullptr; // word 0 = meshlets (first & ~31) .. +31
    uint2 *base32 = nullptr;                                     // entry 0 = meshlet (first & ~31)
    BlockBound *blk = nullptr; // entry 0 = meshlets (first & ~31) .. +31: the block's bound (block_pretest.h), re-derived
                               // by every update for the blocks it touches; zero (not valid) where none was derived
    // A stream may be bound to several contexts, each with its own lock: its own state has its own.  The device-side
    // order of an update against the culls that read it is the caller's, like the order of the meshlet upload itself.
    std::mutex mu;
    const void *source = nullptr;          // Meshlet buffer of the updates so far (nullptr: never updated)
    uint64_t valid_lo = 0, valid_hi = 0;   // hull of the ranges derived from `source`: what a cull may read
    const void *materials = nullptr;       // orbit_meshlet_stream_set_materials: what the alpha classes mirror; read on
                                           // the DEVICE by every later update (the caller forgets it before freeing it)
    uint32_t material_count = 0;
    // "Some meshlet has class 3" (a material beyond the table, an alpha_mode > 2): written on the device by the launches
    // that derive classes, copied to pinned host memory behind them.  A cull reads the classes only once that copy has
    // landed and says no (hipEventQuery, never a wait); until then, and for streams with such meshlets, the
    // evaluation goes through the material indices, which is always right.
    uint32_t *d_other = nullptr, *h_other = nullptr;
    hipEvent_t other_event = nullptr;
    bool other_pending = false;  // a derivation is under way (or its outcome unknowable): do not trust the classes
    bool other_recorded = false; // other_event was recorded for the pending derivation (on a stream that really runs)
    std::atomic<int> bindings{0};          // contexts it is bound to (orbit_meshlet_stream_destroy refuses while > 0)
    // orbit_meshlet_stream_update_meshes: 32-B side entries of the meshes of `mesh_source` (kernels.h MeshSide);
    // allocated (zero-filled) by the first update, meshes [0, mesh_hi) may be read
    MeshSide *mesh_side = nullptr;
    uint32_t mesh_capacity = 0, mesh_hi = 0;
    const void *mesh_source = nullptr;
    uint64_t mesh_side_culls = 0;          // entity culls that were handed the table
};

struct OrbitCtx {
    int device = 0;
    uint32_t num_cus = 0;
    OrbitCaps caps{};
    std::mutex mu; // entry points are thread-safe per ctx (pass closures are Send + Sync, context.rs:617-620)
    // scratch (device)
    uint8_t *arena = nullptr;
    size_t arena_bytes = 0;
    OrbitMeshletDispatch *e_proto = nullptr;
    uint32_t *e_block_sums = nullptr, *e_total = nullptr;
    Payload *m_tile_payload = nullptr;
    uint32_t *m_tile_masks = nullptr, *m_chunk_sums = nullptr;
    uint32_t *m_tile_counts = nullptr, *m_tile_base = nullptr, *m_total = nullptr;
    uint32_t *s_block_sums = nullptr; // orbit_scene_update: {meshes, lights, shadow casters} per 256 entities
    uint32_t raster_blocks[kRasterVariants] = {};     // orbit_raster_depth: per variant, workgroups of its kernel resident at once
    uint32_t visibility_blocks[kRasterVariants] = {}; // orbit_raster_visibility: the same of its kernels
    float *b_mesh_slices = nullptr;  // orbit_mesh_bounds: 8 floats per range and slice, kMeshBoundsSlots of them
    uint32_t *x_block_pop = nullptr; // orbit_expand_visible_records: survivors per 1024 records of the list
    uint32_t *c_chunk = nullptr; // compact: its own chunk counts | the ones a counting mark launch left (c_chunk_words each)
    size_t c_chunk_words = 0;
    float4 *a_view_lights = nullptr, *a_coarse_lights = nullptr;
    uint32_t *a_light_flags = nullptr, *a_counts = nullptr, *a_block_sums = nullptr, *a_block_base = nullptr,
             *a_total = nullptr, *a_coarse = nullptr, *a_coarse_counts = nullptr, *a_hit_cache = nullptr;
    float *a_aabb = nullptr, *a_group_box = nullptr;
    uint32_t *a_group_order = nullptr;
    uint32_t a_coarse_seg = 0;
    uint32_t *m_tickets = nullptr, *m_list_sync = nullptr, *f_done = nullptr;
    uint32_t *f_sync = nullptr, *f_ent_flags = nullptr, *f_tile_flags = nullptr; // one-launch cull (cull_fused.hip)
    uint32_t *d_tickets = nullptr; // depth_reduce: one arrival counter per pyramid of a batch
    uint8_t *m_split = nullptr;    // dispatch_size 64 / 128: the caller's records as records of 32 (entity_cull.hip split_records_body)
    uint32_t rec_shift = 5;        // log2 of caps.dispatch_size
    uint64_t fused_culls = 0;                                                    // views culled by it so far
    uint64_t shard_culls = 0;                                                    // orbit_cull_shard calls that took ONE launch
    uint32_t *g_counts = nullptr; // gather_visible: per-rank command counts
    int32_t *status = nullptr;
    uint32_t debug_flags = 0;
    uint32_t scan_patience = 256; // meshlet_emit.hip emit_scan_wait (orbit_debug_set_scan_patience)
    unsigned long long *debug_cycles = nullptr;
    void *zero_page = nullptr;
    // measurement hook: HIP event pairs around the dominant kernel (meshlet_eval)
    uint32_t profiling = 0;   // 0 off, n: every n-th meshlet cull is timed
    uint32_t prof_calls = 0;
    std::vector<hipEvent_t> prof_events; // pairs, in record order
    size_t prof_used = 0;
    // orbit_cull_views: child contexts (own scan scratch) for views 1.., created on first use
    std::vector<OrbitCtx *> view_ctx;
    hipStream_t side_stream[2] = {nullptr, nullptr}; // orbit_frame_late: the chains beside the caller's stream
    hipEvent_t side_event[3] = {nullptr, nullptr, nullptr}; // fork, join of chain B, join of chain C
    OrbitMeshletStream *meshlet_stream = nullptr; // orbit_ctx_bind_meshlet_stream
    uint64_t stream_culls = 0;                          // meshlet culls launched from it
    uint64_t class_culls = 0;                           // ... of which with its alpha classes
    uint64_t block_culls = 0;                           // ... of which decided per block (meshlet_eval_blocks.hip)
    bool block_cull = true;                             // orbit_ctx_set_block_cull / ORBIT_BLOCK_CULL=0
    uint32_t block_cull_grid = 0;                       // orbit_ctx_set_block_cull_grid: workgroups at most (0 = no cap)
    uint32_t raster_grid = 0;                           // orbit_ctx_set_raster_grid: the same for every raster launch
    uint32_t fused_grid = 0;                            // orbit_ctx_set_fused_grid: the same for the one-launch cull's launches
    uint32_t visibility_grid = 0;                       // orbit_ctx_set_visibility_grid: the same for the buffer's readers and orbit_post_process
    char err[512] = {0};
};

// orbit_expand_visible_records: a list of up to kExpandBlocks * 1024 records (64 M) can be expanded
constexpr uint32_t kExpandBlocks = 65536;

// orbit_mesh_bounds: (range, slice) pairs one batch of launches works on
constexpr uint32_t kMeshBoundsSlots = 1024;

// ------------------------------------------------------------------- errors (abi_ctx.hip)
// The last error of the calling thread (orbit_last_error(NULL)); every failure also lands in its context's `err`.
extern thread_local char g_err[512];

int32_t fail(OrbitCtx *ctx, int32_t code, const char *fmt, ...);

inline int32_t hip_fail(OrbitCtx *ctx, hipError_t e, const char *what) {
    return fail(ctx, ORBIT_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// hipMemset of device memory returns before the fill has run (it is ordered on the null stream), and the streams the
// library is called on later need not wait for the null stream (hipStreamNonBlocking: torch's side streams are): a
// context's first cull could run while its scratch was still being cleared under it (found by
// tests/test_concurrent_gpu.py once the arena had grown by a gigabyte).  Every fill of memory that launches on OTHER
// streams will use is therefore waited for before the call that made it returns.
inline hipError_t memset_now(void *ptr, int value, size_t bytes) {
    hipError_t e = hipMemset(ptr, value, bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
}

inline uint32_t mip_levels_from_size(uint32_t max_size) { // src/math.rs:18-20
    uint32_t l = 0;
    while ((max_size >> (l + 1)) != 0) l++;
    return l + 1;
}

// The caps of a view's child context (orbit_cull_views' scratch for views 1..): the culls' scratch only — no cluster or
// light scratch, the bulk of a context's.
inline OrbitCaps view_child_caps(OrbitCaps child_caps) {
    child_caps.max_views = 0, child_caps.max_clusters = 0, child_caps.max_lights = 0;
    return child_caps;
}

// ------------------------------------------------------------ meshlet streams (per cull: inline)
// The stream's arrays based at global meshlet index 0, like meshlet_buffer itself, over the range derived so far.
inline MeshletStreamView stream_arrays(const OrbitMeshletStream *ms, uint64_t lo, uint64_t hi) {
    MeshletStreamView v{};
    v.sphere = ms->sphere - ms->first;
    v.cone = ms->cone - ms->first;
    v.mat = ms->mat - ms->first;
    v.cmd = ms->cmd - 3u * ms->first;
    v.cnt = ms->cnt - ms->first;
    v.link = ms->link - (ms->first >> 5);
    v.base32 = ms->base32 - (ms->first >> 5);
    v.cls0 = ms->cls0 - (ms->first >> 5);
    v.cls1 = ms->cls1 - (ms->first >> 5);
    v.first = (uint32_t)lo;
    v.count = (uint32_t)(hi - lo);
    return v;
}

// What a cull of `meshlet_buffer` (with `material_buffer`) may take from the stream bound to its context: nothing
// unless the stream mirrors that very buffer; the alpha classes only if they mirror that very material buffer.
inline MeshletStreamView stream_view_for(OrbitMeshletStream *ms, const void *meshlet_buffer, const void *material_buffer) {
    if (!ms) return MeshletStreamView{};
    std::lock_guard<std::mutex> lock(ms->mu);
    if (ms->source == nullptr || ms->source != meshlet_buffer || ms->valid_hi == ms->valid_lo) return MeshletStreamView{};
    MeshletStreamView v = stream_arrays(ms, ms->valid_lo, ms->valid_hi);
    bool classes = ms->materials != nullptr && ms->materials == material_buffer;
    // (no query while the flag's read-back was only captured into a graph, not run: other_recorded is false then)
    if (classes && ms->other_pending && ms->other_recorded && hipEventQuery(ms->other_event) == hipSuccess)
        ms->other_pending = false;
    if (classes && (ms->other_pending || *ms->h_other != 0u)) classes = false;
    if (!classes) v.cls0 = v.cls1 = nullptr;
    return v;
}

// The stream's block bounds based at block 0, for a launch whose parameter block reads this stream (p.ms of stream_view_for)
inline const BlockBound *stream_block_bounds(const OrbitMeshletStream *ms) { return ms->blk - (ms->first >> 5); }

// ------------------------------------------------------------------ culls (abi_cull.hip)
// One orbit_cull_views call, validated and laid out, not yet enqueued (orbit_frame_late validates all its groups before
// it forks anything).  Scratch: view i runs on scratch set `scratch_base + i` (0 = the context itself, k = child k - 1).
struct PreparedCullViews {
    EntityCullViews ev{};
    MeshletCullViews mv{};
    FusedCullViews fv{};
    SplitRecordsViews sv{}; // dispatch_size 64 / 128: entry k serves mv.v[k]
    uint32_t draws[ORBIT_MAX_CULL_VIEWS] = {};
    uint32_t count = 0, n_mesh = 0, max_draws = 0;
    bool fused = false;
};

// Caller holds ctx->mu.  Allocates missing scratch sets (the only allocation an enqueue call can ever make).
int32_t prepare_cull_views(OrbitCtx *ctx, const OrbitCullView *views, uint32_t count, uint32_t scratch_base,
                           PreparedCullViews &pc);
int32_t launch_prepared_cull_views(OrbitCtx *ctx, const PreparedCullViews &pc, hipStream_t s);

#pragma GCC visibility pop
