// raster_walk.h — the compute rasteriser of DESIGN.md §4.12 / §4.13, the one owner of its walker: a template on the SINK
// that takes an inside sample, with the clear kernel and the launch that every raster call shares.  raster_depth.hip and
// raster_visibility.hip add a sink and a one-line kernel each.  The arithmetic is raster_common.h's, shared with the
// host mirror, which is the pin.
//
// A grid of as many wave64s as are resident at once (or fewer); a wave takes one command (= one meshlet of one entity) at a time.
//   phase 1  the wave checks the command's ranges (R9, and the sink's triangle limit) — nothing is read before its index
//            is known to be in range —, computes mvp = view_proj x model, and its lanes transform the <= 255 vertices into
//            LDS: snapped X, Y, z / w and the clip / guard flags, 16 B per vertex
//   phase 2  a lane per triangle (chunks of 64): setup and the rejects of R3-R5, counted per lane and summed once per
//            wave when it runs out of commands
//   phase 3  a triangle whose pixel box holds at most kLaneBox samples is walked by its own lane (most are: two thirds
//            of the front faces of the test scene cover no sample at all); a larger one is taken by the whole wave, one
//            at a time (ballot, the corners broadcast, every lane repeats the setup, lanes take the 8 x 8 tiles of the
//            box).  Edge functions are stepped in int64, the same integers as evaluating them per sample.
// Behind ORBIT_RASTER_WIDE_GUARD (RasterVariant::Wide, R4w) a triangle with a vertex beyond R4's band is taken by the whole wave as well,
// but not box by box: walk_wide rejects 64 x 64 blocks, then 8 x 8 tiles, and evaluates samples only in the tiles left.
// A sink has
//   static constexpr uint32_t kMaxTriangles   a command with more triangles is a range error (V3); ~0u: no limit
//   bool write(const Setup &, x, y, width, id) const   R7 + the merge of one inside sample -> it is a fragment (d > 0);
//                                                      and the same for a SetupW (R7w)
// where id = (id_base + the command's position) << 8 | triangle index.  Both sinks merge by atomicMax: the result does
// not depend on scheduling or command order.
#pragma once
#include "kernels.h"
#include "orbit_device.h"
#include "raster_common.h"

// A##B after both are expanded: a raster unit names its kernel from its ORBIT_RASTER_VARIANT with it
#define ORBIT_RASTER_PASTE_(a, b) a##b
#define ORBIT_RASTER_PASTE(a, b) ORBIT_RASTER_PASTE_(a, b)

namespace orbit {
namespace raster {

constexpr uint32_t kRasterThreads = 256, kRasterWaves = kRasterThreads / 64;
constexpr uint32_t kMaxVertices = 256; // vcount <= 255 (R9)
constexpr int32_t kLaneBox = 16; // samples: a box no larger is walked by the triangle's own lane (not yet tuned)

struct RasterParams { // what the walker reads; the target belongs to the sink
    const uint32_t *commands; // {count; 7 words per command}
    const uint32_t *meshlet_data;
    const uint8_t *vertices;
    const float *entity_data; // 32 floats per entity, the model matrix first
    uint32_t *stats;
    uint64_t meshlet_data_words, vertex_count;
    uint32_t max_commands, entity_count, vertex_stride, position_offset, width, height, flags;
    float view_proj[16];
    int32_t *status;
};

// (OrbitRasterDepth and OrbitRasterVisibility name these fields alike)
template <class Job>
inline void fill_raster_params(RasterParams &p, const Job &job, int32_t *status) {
    p.commands = (const uint32_t *)job.draw_commands;
    p.meshlet_data = job.meshlet_data;
    p.vertices = (const uint8_t *)job.vertices;
    p.entity_data = (const float *)job.entity_data;
    p.stats = (uint32_t *)job.stats;
    p.meshlet_data_words = job.meshlet_data_words, p.vertex_count = job.vertex_count;
    p.max_commands = job.max_commands, p.entity_count = job.entity_count;
    p.vertex_stride = job.vertex_stride, p.position_offset = job.position_offset;
    p.width = job.width, p.height = job.height, p.flags = job.flags;
    for (int k = 0; k < 16; k++) p.view_proj[k] = job.view_proj[k];
    p.status = status;
}

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ Vertex lds_vertex(const int4 *verts, uint32_t i) {
    const int4 w = verts[i];
    Vertex v;
    v.X = w.x, v.Y = w.y, v.d = __int_as_float(w.z), v.flags = (uint32_t)w.w;
    return v;
}

__device__ __forceinline__ Vertex readlane_vertex(const Vertex &v, uint32_t src) {
    Vertex out;
    out.X = __builtin_amdgcn_readlane(v.X, (int)src), out.Y = __builtin_amdgcn_readlane(v.Y, (int)src);
    out.d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.d), (int)src));
    out.flags = (uint32_t)__builtin_amdgcn_readlane((int)v.flags, (int)src);
    return out;
}

// The wave's mvp beyond phase 1: the pieces form of phase 2 reads it again; the plain form has nothing to keep
template <bool kKeep>
struct KeptMvp {
    float m[16];
    __device__ __forceinline__ void keep(const float *mvp) {
        for (int k = 0; k < 16; k++) m[k] = mvp[k];
    }
};
template <>
struct KeptMvp<false> {
    __device__ __forceinline__ void keep(const float *) {}
};

// The samples (x_lo + x0 + k * step_x, y_lo + y0 + j * step_y) of the triangle's box: the lane path takes all of them
// (x0 = y0 = 0, steps of 1), a lane of the wave path its own sample of every 8 x 8 tile.  -> inside samples; fragments
// are added to `fragments`.
template <class Sink>
__device__ __forceinline__ uint32_t walk(const Sink &sink, uint32_t width, const Setup &s, int32_t x0, int32_t y0,
                                         int32_t step, uint32_t id, uint32_t &fragments) {
    uint32_t inside = 0;
    const int64_t sx0 = -(int64_t)s.dy[0] * 256 * step, sx1 = -(int64_t)s.dy[1] * 256 * step,
                  sx2 = -(int64_t)s.dy[2] * 256 * step; // E(px + 256 step) - E(px)
    for (int32_t y = s.y_lo + y0; y <= s.y_hi; y += step) {
        const int32_t x = s.x_lo + x0, py = 256 * y + 128;
        int64_t e0 = edge_at(s, 0, 256 * x + 128, py), e1 = edge_at(s, 1, 256 * x + 128, py),
                e2 = edge_at(s, 2, 256 * x + 128, py);
        for (int32_t xx = x; xx <= s.x_hi; xx += step) {
            if ((e0 | e1 | e2) >= 0) {
                inside++;
                fragments += sink.write(s, xx, y, width, id) ? 1u : 0u;
            }
            e0 += sx0, e1 += sx1, e2 += sx2;
        }
    }
    return inside;
}

// R6w-R7w of one wide triangle by the whole wave (`s` is wave-uniform).  A near-cut triangle has a box that is most of
// the target and a coverage that is a wedge of it, so the box is not stepped: a lane takes a 64 x 64 block of it (on the
// target's grid) and asks rect_outside_wide; of each block that stays a lane takes an 8 x 8 tile and asks again; of each
// tile that stays a lane takes a sample.  The rectangle test is exact in the direction used (raster_common.h), so the
// samples found inside are the samples inside.  -> this lane's inside samples.
template <class Sink>
__device__ __forceinline__ uint32_t walk_wide(const Sink &sink, uint32_t width, const SetupW &s, uint32_t lane, uint32_t id,
                                              uint32_t &fragments) {
    uint32_t inside = 0;
    const int32_t bx0 = s.x_lo >> 6, by0 = s.y_lo >> 6;
    const uint32_t blocks_x = (uint32_t)((s.x_hi >> 6) - bx0 + 1), blocks = blocks_x * (uint32_t)((s.y_hi >> 6) - by0 + 1); // <= 512^2
    for (uint32_t first = 0; first < blocks; first += 64u) {
        const uint32_t b = first + lane;
        int32_t ox = 0, oy = 0; // the block's first pixel
        bool live = false;
        if (b < blocks) { // (every block of the range holds pixels of the box)
            ox = (bx0 + (int32_t)(b % blocks_x)) << 6, oy = (by0 + (int32_t)(b / blocks_x)) << 6;
            live = !rect_outside_wide(s, imax(ox, s.x_lo), imax(oy, s.y_lo), imin(ox + 63, s.x_hi), imin(oy + 63, s.y_hi));
        }
        uint64_t live_blocks = __ballot(live);
        while (live_blocks != 0ull) {
            const uint32_t src = (uint32_t)__builtin_ctzll(live_blocks);
            live_blocks &= live_blocks - 1ull;
            const int32_t wx = __builtin_amdgcn_readlane(ox, (int)src), wy = __builtin_amdgcn_readlane(oy, (int)src);
            const int32_t tx = wx + 8 * (int32_t)(lane & 7u), ty = wy + 8 * (int32_t)(lane >> 3);
            const int32_t x0 = imax(tx, s.x_lo), y0 = imax(ty, s.y_lo), x1 = imin(tx + 7, s.x_hi), y1 = imin(ty + 7, s.y_hi);
            uint64_t live_tiles = __ballot(x0 <= x1 && y0 <= y1 && !rect_outside_wide(s, x0, y0, x1, y1));
            while (live_tiles != 0ull) {
                const uint32_t tile = (uint32_t)__builtin_ctzll(live_tiles);
                live_tiles &= live_tiles - 1ull;
                const int32_t x = wx + 8 * (int32_t)(tile & 7u) + (int32_t)(lane & 7u);
                const int32_t y = wy + 8 * (int32_t)(tile >> 3) + (int32_t)(lane >> 3);
                // (inside the box: inside the target)
                if (x >= s.x_lo && x <= s.x_hi && y >= s.y_lo && y <= s.y_hi && inside_wide(s, x, y)) {
                    inside++;
                    fragments += sink.write(s, x, y, width, id) ? 1u : 0u;
                }
            }
        }
    }
    return inside;
}

// The body of a raster kernel: a resident grid of wave64s striding over the command list, in the phases named at the
// top.  `id_base` is added to the command's position in the list before it goes into the sample's id.
//
// V (kernels.h) picks one of two forms of phase 2, and what phase 1 keeps for it:
//   Plain     a lane sets up its triangle from LDS and counts the outcome directly; the wave walk reads the corners
//             from LDS again.  The code as it was before either flag existed: it holds fewer registers than the pieces
//             form, which is why it stays a form of its own.
//   ClipNear  (ORBIT_RASTER_CLIP_NEAR, R3c) the pieces form: a lane whose triangle R3 rejects with a vertex in reads the
//             three positions again through the index words phase 1 checked, recomputes their clip coordinates from the
//             wave's mvp and builds its pieces in registers (raster_common.h); each piece then takes the routes above,
//             and the triangle is counted once, under the best outcome of its pieces.  The wave walk broadcasts a piece's
//             three Vertex records from the owning lane, as its vertices are not in LDS.
//   Wide      (ORBIT_RASTER_WIDE_GUARD, R4w; with or without CLIP_NEAR) phase 1 keeps a guard-failing vertex's xf, yf in
//             its LDS record; phase 2 is the pieces form with ORBIT_RASTER_CLIP_NEAR read from the flag word and three
//             additions under `if constexpr`: a piece with every vertex narrow takes the routes above unchanged, one with
//             a vertex out of band is guard_skipped, and a wide one (is_wide_triangle) is taken by the whole wave
//             (walk_wide), its three Vertex records broadcast from the owning lane and its setup wave-uniform.
template <RasterVariant V, class Sink>
__device__ __forceinline__ void raster_commands(const RasterParams &p, const Sink &sink, uint32_t id_base) {
    constexpr bool kWide = V == RasterVariant::Wide;
    __shared__ int4 lds_verts[kRasterWaves][kMaxVertices];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int4 *verts = lds_verts[wave];
    const uint8_t *data_bytes = (const uint8_t *)p.meshlet_data;
    const uint32_t listed = p.commands[0];
    const uint32_t count = listed < p.max_commands ? listed : p.max_commands;
    const bool cull_none = (p.flags & ORBIT_RASTER_CULL_NONE) != 0u;
    const float w_f = (float)p.width, h_f = (float)p.height;
    // this lane's share of the counters, OrbitRasterStats' order
    uint32_t n_commands = 0, n_triangles = 0, n_outcome[5] = {0, 0, 0, 0, 0}, n_fragments = 0, n_range = 0;
    const uint32_t stride = gridDim.x * kRasterWaves;
    if (blockIdx.x * kRasterWaves + wave >= count) return; // (wave-uniform) no command for this wave: nothing to add
    for (uint32_t i = blockIdx.x * kRasterWaves + wave; i < count; i += stride) {
        const uint32_t *cmd = p.commands + 1u + 7u * (size_t)i;
        const uint32_t index_count = cmd[0], first_index = cmd[2], index_base = cmd[3], entity = cmd[4];
        const uint64_t vertex_base = cmd[5];
        const uint32_t nt = index_count / 3u, first_word = first_index / 4u;
        const uint32_t vcount = first_word - index_base; // (meaningful once first_word >= index_base)
        if (lane == 0u) n_commands++;
        // R9 (and V3's triangle limit), the wave-uniform part: the index words [index_base, first_word) and the corner
        // bytes lie in meshlet_data
        bool bad = first_word < index_base || vcount > 255u || (uint64_t)first_word > p.meshlet_data_words ||
                   ((uint64_t)first_index + 3ull * nt + 3ull) / 4ull > p.meshlet_data_words || entity >= p.entity_count ||
                   nt > Sink::kMaxTriangles;
        KeptMvp<V != RasterVariant::Plain> kept; // (set when !bad)
        if (!bad) {
            float mvp[16];
            {
                const float *model = p.entity_data + 32u * (size_t)entity;
                float m[16];
                for (int k = 0; k < 16; k++) m[k] = model[k];
                mat4_mul(p.view_proj, m, mvp);
                kept.keep(mvp);
            }
            bool lane_bad = false;
            for (uint32_t v = lane; v < vcount; v += 64u) {
                const uint64_t g = vertex_base + p.meshlet_data[index_base + v];
                Vertex out;
                out.X = out.Y = 0, out.d = 0.f, out.flags = kClipFail;
                if (g < p.vertex_count) {
                    const float *src = (const float *)(p.vertices + g * p.vertex_stride + p.position_offset);
                    out = transform_vertex(mvp, src[0], src[1], src[2], w_f, h_f, kWide);
                } else {
                    lane_bad = true;
                }
                verts[v] = make_int4(out.X, out.Y, __float_as_int(out.d), (int)out.flags);
            }
            for (uint32_t t = lane; t < nt; t += 64u) {
                const uint8_t *c = data_bytes + (size_t)first_index + 3u * (size_t)t;
                if (c[0] >= vcount || c[1] >= vcount || c[2] >= vcount) lane_bad = true;
            }
            bad = __ballot(lane_bad) != 0ull;
        }
        if (bad) { // the command is skipped whole
            if (lane == 0u) {
                n_range++;
                latch_status(p.status, ORBIT_E_RANGE);
            }
            continue;
        }
        if (lane == 0u) n_triangles += nt;
        const uint32_t command_id = (id_base + i) << 8;
        wave_lds_sync();
        if constexpr (V == RasterVariant::Plain) {
            for (uint32_t base = 0; base < nt; base += 64u) {
                const uint32_t t = base + lane;
                Setup s;
                uint32_t corners = 0;
                bool draw = false;
                if (t < nt) {
                    const uint8_t *c = data_bytes + (size_t)first_index + 3u * (size_t)t;
                    corners = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16;
                    const uint32_t outcome = setup_triangle(lds_vertex(verts, c[0]), lds_vertex(verts, c[1]),
                                                            lds_vertex(verts, c[2]), p.width, p.height, cull_none, s);
                    for (uint32_t k = 1; k < 5u; k++) n_outcome[k] += outcome == k ? 1u : 0u;
                    draw = outcome == kDraw;
                }
                // (boxes are at most 32768^2 samples: the product fits)
                const bool small = draw && (s.x_hi - s.x_lo + 1) * (s.y_hi - s.y_lo + 1) <= kLaneBox;
                if (small && walk(sink, p.width, s, 0, 0, 1, command_id | t, n_fragments) == 0u) n_outcome[kNoCoverage]++;
                uint64_t large = __ballot(draw && !small);
                while (large != 0ull) {
                    const uint32_t src = (uint32_t)__builtin_ctzll(large);
                    large &= large - 1ull;
                    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)corners, (int)src);
                    Setup ws;
                    (void)setup_triangle(lds_vertex(verts, c & 0xFFu), lds_vertex(verts, (c >> 8) & 0xFFu),
                                         lds_vertex(verts, c >> 16), p.width, p.height, cull_none, ws);
                    const uint32_t inside = walk(sink, p.width, ws, (int32_t)(lane & 7u), (int32_t)(lane >> 3), 8,
                                                 command_id | (base + src), n_fragments);
                    if (__ballot(inside != 0u) == 0ull && lane == 0u) n_outcome[kNoCoverage]++;
                }
            }
        } else {
            // (Wide: a wave-uniform branch, so the flag pair costs two kernels, not four)
            const bool clip_near = V == RasterVariant::ClipNear || (p.flags & ORBIT_RASTER_CLIP_NEAR) != 0u;
            for (uint32_t base = 0; base < nt; base += 64u) {
                const uint32_t t = base + lane;
                Pieces pc;
                pc.count = 0u;
                for (int k = 0; k < 4; k++) pc.u[k].X = pc.u[k].Y = 0, pc.u[k].d = 0.f, pc.u[k].flags = 0u;
                if (t < nt) {
                    const uint8_t *c = data_bytes + (size_t)first_index + 3u * (size_t)t;
                    pc.u[0] = lds_vertex(verts, c[0]), pc.u[1] = lds_vertex(verts, c[1]), pc.u[2] = lds_vertex(verts, c[2]);
                    pc.u[3] = pc.u[2];
                    const uint32_t any_out = (pc.u[0].flags | pc.u[1].flags | pc.u[2].flags) & kClipFail;
                    const uint32_t all_out = pc.u[0].flags & pc.u[1].flags & pc.u[2].flags & kClipFail;
                    if (any_out == 0u) {
                        pc.count = 1u;
                    } else if (clip_near && all_out == 0u) { // R3c: a vertex in, a vertex out
                        Clip cc[3];
                        for (int k = 0; k < 3; k++) {
                            const uint64_t g = vertex_base + p.meshlet_data[index_base + c[k]]; // in range: phase 1
                            const float *src = (const float *)(p.vertices + g * p.vertex_stride + p.position_offset);
                            cc[k] = clip_position(kept.m, src[0], src[1], src[2]);
                        }
                        clip_near_pieces(cc[0], cc[1], cc[2], w_f, h_f, pc, kWide);
                    }
                    if (pc.count == 0u) n_outcome[kClipSkipped]++;
                }
                uint32_t best = kNoCoverage; // of this lane's pieces; counted once below
                const uint32_t rounds = __ballot(pc.count > 1u) != 0ull ? 2u : 1u;
#pragma nounroll
                for (uint32_t q = 0; q < rounds; q++) {
                    Vertex v0, v1, v2;
                    piece_vertices(pc, q, v0, v1, v2);
                    Setup s;
                    bool draw = false, wide = false;
                    if (q < pc.count) {
                        if constexpr (kWide) wide = is_wide_triangle(v0, v1, v2);
                        if (!wide) { // all narrow, or a vertex out of band: guard_skipped
                            const uint32_t outcome = setup_triangle(v0, v1, v2, p.width, p.height, cull_none, s);
                            draw = outcome == kDraw;
                            if (!draw) best = better_outcome(best, outcome);
                        }
                    }
                    const bool small = draw && (s.x_hi - s.x_lo + 1) * (s.y_hi - s.y_lo + 1) <= kLaneBox;
                    if (small && walk(sink, p.width, s, 0, 0, 1, command_id | t, n_fragments) != 0u) best = kDraw;
                    uint64_t large = __ballot(draw && !small);
                    while (large != 0ull) {
                        const uint32_t src = (uint32_t)__builtin_ctzll(large);
                        large &= large - 1ull;
                        const Vertex b0 = readlane_vertex(v0, src), b1 = readlane_vertex(v1, src), b2 = readlane_vertex(v2, src);
                        Setup ws;
                        (void)setup_triangle(b0, b1, b2, p.width, p.height, cull_none, ws);
                        const uint32_t inside = walk(sink, p.width, ws, (int32_t)(lane & 7u), (int32_t)(lane >> 3), 8,
                                                     command_id | (base + src), n_fragments);
                        if (__ballot(inside != 0u) != 0ull && lane == src) best = kDraw;
                    }
                    if constexpr (kWide) {
                        uint64_t wides = __ballot(wide);
                        while (wides != 0ull) {
                            const uint32_t src = (uint32_t)__builtin_ctzll(wides);
                            wides &= wides - 1ull;
                            const Vertex b0 = readlane_vertex(v0, src), b1 = readlane_vertex(v1, src), b2 = readlane_vertex(v2, src);
                            SetupW ws;
                            const uint32_t outcome = setup_triangle_wide(b0, b1, b2, p.width, p.height, cull_none, ws); // (wave-uniform)
                            uint32_t inside = 0;
                            if (outcome == kDraw) inside = walk_wide(sink, p.width, ws, lane, command_id | (base + src), n_fragments);
                            const bool covered = __ballot(inside != 0u) != 0ull;
                            if (lane == src) best = covered ? (uint32_t)kDraw : better_outcome(best, outcome == kDraw ? (uint32_t)kNoCoverage : outcome);
                        }
                    }
                }
                if (pc.count != 0u && best != kDraw) n_outcome[best]++;
            }
        }
        wave_lds_sync(); // the next command overwrites the wave's vertices
    }
    if (!p.stats) return;
    uint32_t sums[8] = {n_commands,           n_triangles,           n_outcome[kClipSkipped], n_outcome[kGuardSkipped],
                        n_outcome[kBackFacing], n_outcome[kNoCoverage], n_fragments,            n_range};
    for (uint32_t k = 0; k < 8u; k++) {
        uint32_t v = sums[k];
        for (uint32_t d = 1; d < 64u; d <<= 1) v += (uint32_t)__shfl_xor((int)v, (int)d, 64);
        if (lane == 0u && v != 0u) atomicAdd(&p.stats[k], v);
    }
}

// target[0, words) = 0 and, if given, the eight counters = 0
template <class Word>
__global__ __launch_bounds__(kRasterThreads) void raster_clear_kernel(Word *target, uint64_t words, uint32_t *stats) {
    const uint64_t stride = (uint64_t)gridDim.x * kRasterThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kRasterThreads + threadIdx.x; i < words; i += stride) target[i] = 0;
    if (stats && blockIdx.x == 0u && threadIdx.x < 8u) stats[threadIdx.x] = 0u;
}

// A raster call on the stream: one launch clears `target` (ORBIT_RASTER_CLEAR) and the counters, the next is `kernel`
// over (the job's RasterParams, args...).  LoadOp::Clear(0.0) and the counters' clear are a launch, not memset nodes: a
// captured call then consists of kernel nodes only, whose arguments a replay carries by value.
template <class Job, class Word, class... Args>
inline hipError_t launch_raster(void (*kernel)(RasterParams, Args...), const Job &job, Word *target, uint32_t resident_blocks,
                                int32_t *status, hipStream_t s, Args... args) {
    const uint64_t clear_words = (job.flags & ORBIT_RASTER_CLEAR) ? (uint64_t)job.width * job.height : 0ull;
    const uint64_t cap = resident_blocks ? resident_blocks : 512u;
    if (clear_words != 0ull || job.stats) {
        const uint64_t need = (clear_words + kRasterThreads * 4ull - 1ull) / (kRasterThreads * 4ull);
        const uint32_t blocks = (uint32_t)(need < 1ull ? 1ull : need < cap ? need : cap);
        hipLaunchKernelGGL(raster_clear_kernel<Word>, dim3(blocks), dim3(kRasterThreads), 0, s, target, clear_words,
                           (uint32_t *)job.stats);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (job.max_commands == 0u) return hipSuccess;
    RasterParams p;
    fill_raster_params(p, job, status);
    // the count is the device's: the grid covers max_commands, up to as many workgroups as are resident at once (the
    // kernel's registers decide how many per CU), which stride over the list
    const uint64_t need = ((uint64_t)job.max_commands + kRasterWaves - 1u) / kRasterWaves;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)(need < cap ? need : cap)), dim3(kRasterThreads), 0, s, p, args...);
    return hipGetLastError();
}

} // namespace raster
} // namespace orbit
