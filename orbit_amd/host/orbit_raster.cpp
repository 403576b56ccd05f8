// orbit_raster.cpp — see orbit_raster.hpp.
#include "orbit_raster.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../csrc/raster_common.h"
#include "../csrc/surface_common.h"
#include "../csrc/fragment_common.h"
#include "../csrc/shade_common.h"
#include "../csrc/shadow_common.h"
#include "../csrc/sky_common.h"
#include "orbit_host.hpp"

namespace orbit {
namespace raster {

namespace {

struct DepthSink { // R8: max on the u32 view
    static constexpr uint32_t kMaxTriangles = ~0u;
    float *depth;
    void clear(size_t pixels) const { std::memset(depth, 0, pixels * sizeof(float)); }
    void write(size_t pixel, uint32_t bits, uint32_t) const {
        uint32_t old;
        std::memcpy(&old, depth + pixel, 4);
        if (bits > old) std::memcpy(depth + pixel, &bits, 4);
    }
};

struct VisibilitySink { // V2: max on the u64 view of depth bits << 32 | id
    static constexpr uint32_t kMaxTriangles = 256u; // V3
    uint64_t *visibility;
    void clear(size_t pixels) const { std::memset(visibility, 0, pixels * sizeof(uint64_t)); }
    void write(size_t pixel, uint32_t bits, uint32_t id) const {
        const uint64_t word = (uint64_t)bits << 32 | id;
        if (word > visibility[pixel]) visibility[pixel] = word;
    }
};

// the one sequential walk of both calls; id = (id_base + the command's position) << 8 | triangle
template <class Sink>
void raster_into(const HostJob &j, const Sink &sink, bool has_target, uint32_t id_base, OrbitRasterStats *stats,
                 int32_t *command_error) {
    if (!j.draw_commands || !j.meshlet_data || !j.vertices || !j.entity_data || !has_target || !j.view_proj)
        throw Panic("raster_depth: NULL argument");
    if ((uint64_t)j.vertex_stride < (uint64_t)j.position_offset + 12u || (j.vertex_stride & 3u) || (j.position_offset & 3u))
        throw Panic("raster_depth: vertex_stride / position_offset");
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        throw Panic("raster_depth: target size");
    if (j.flags & ~(ORBIT_RASTER_CLEAR | ORBIT_RASTER_CULL_NONE | ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD)) throw Panic("raster_depth: unknown flags");
    if (j.flags & ORBIT_RASTER_CLEAR) sink.clear((size_t)j.width * j.height);
    OrbitRasterStats st{};
    const bool cull_none = (j.flags & ORBIT_RASTER_CULL_NONE) != 0u, clip_near = (j.flags & ORBIT_RASTER_CLIP_NEAR) != 0u;
    const bool wide = (j.flags & ORBIT_RASTER_WIDE_GUARD) != 0u; // R4w
    const uint8_t *data_bytes = reinterpret_cast<const uint8_t *>(j.meshlet_data);
    const uint32_t count = j.draw_commands[0] < j.max_commands ? j.draw_commands[0] : j.max_commands;
    const float w_f = (float)j.width, h_f = (float)j.height;
    Vertex verts[256];
    Clip clips[256]; // R3c reads them; a Vertex does not keep them
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t *cmd = j.draw_commands + 1u + 7u * (size_t)i;
        const uint32_t index_count = cmd[0], first_index = cmd[2], index_base = cmd[3], entity = cmd[4];
        const uint64_t vertex_base = cmd[5];
        const uint32_t nt = index_count / 3u, first_word = first_index / 4u;
        const uint32_t vcount = first_word - index_base;
        st.commands++;
        if (command_error) command_error[i] = 1;
        // R9, V3
        bool bad = first_word < index_base || vcount > 255u || (uint64_t)first_word > j.meshlet_data_words ||
                   ((uint64_t)first_index + 3ull * nt + 3ull) / 4ull > j.meshlet_data_words || entity >= j.entity_count ||
                   nt > Sink::kMaxTriangles;
        for (uint32_t v = 0; v < vcount && !bad; v++) bad = vertex_base + j.meshlet_data[index_base + v] >= j.vertex_count;
        for (uint64_t b = 0; b < 3ull * nt && !bad; b++) bad = data_bytes[first_index + b] >= vcount;
        if (bad) {
            st.range_errors++;
            continue;
        }
        if (command_error) command_error[i] = 0;
        st.triangles += nt;
        float mvp[16];
        mat4_mul(j.view_proj, j.entity_data[entity].model_matrix, mvp);
        for (uint32_t v = 0; v < vcount; v++) {
            float pos[3];
            std::memcpy(pos, j.vertices + (vertex_base + j.meshlet_data[index_base + v]) * j.vertex_stride + j.position_offset, 12);
            clips[v] = clip_position(mvp, pos[0], pos[1], pos[2]);
            verts[v] = vertex_from_clip(clips[v], w_f, h_f, false, wide);
        }
        for (uint32_t t = 0; t < nt; t++) {
            const uint8_t *c = data_bytes + (size_t)first_index + 3u * (size_t)t;
            // the triangle itself, or with ORBIT_RASTER_CLIP_NEAR the pieces of one that R3 rejects (R3c)
            Pieces pc;
            pc.u[0] = verts[c[0]], pc.u[1] = verts[c[1]], pc.u[2] = pc.u[3] = verts[c[2]];
            pc.count = 1u;
            if (clip_near && ((pc.u[0].flags | pc.u[1].flags | pc.u[2].flags) & kClipFail))
                clip_near_pieces(clips[c[0]], clips[c[1]], clips[c[2]], w_f, h_f, pc, wide);
            // R7 (a Setup) or R7w (a SetupW) of one inside sample: a fragment if d > 0
            const auto emit = [&](const auto &setup, int32_t x, int32_t y) {
                const float d = depth_at(setup, 256 * x + 128, 256 * y + 128);
                if (!(d > 0.0f)) return;
                st.fragments++;
                uint32_t bits;
                std::memcpy(&bits, &d, 4);
                sink.write((size_t)y * j.width + (uint32_t)x, bits, (id_base + i) << 8 | t);
            };
            uint32_t best = kNoCoverage; // counted once, under the best outcome of the pieces
            for (uint32_t q = 0; q < pc.count; q++) {
                Vertex v0, v1, v2;
                piece_vertices(pc, q, v0, v1, v2);
                if (wide && is_wide_triangle(v0, v1, v2)) { // R5w-R7w: 8 x 8 tiles of the box, those no edge rules out sample by sample
                    SetupW ws;
                    const uint32_t outcome = setup_triangle_wide(v0, v1, v2, j.width, j.height, cull_none, ws);
                    if (outcome != kDraw) {
                        best = better_outcome(best, outcome);
                        continue;
                    }
                    uint64_t inside = 0;
                    for (int32_t ty = ws.y_lo; ty <= ws.y_hi; ty += 8)
                        for (int32_t tx = ws.x_lo; tx <= ws.x_hi; tx += 8) {
                            const int32_t x1 = imin(tx + 7, ws.x_hi), y1 = imin(ty + 7, ws.y_hi);
                            if (rect_outside_wide(ws, tx, ty, x1, y1)) continue;
                            for (int32_t y = ty; y <= y1; y++)
                                for (int32_t x = tx; x <= x1; x++) {
                                    if (!inside_wide(ws, x, y)) continue;
                                    inside++;
                                    emit(ws, x, y);
                                }
                        }
                    if (inside != 0) best = kDraw;
                    continue;
                }
                Setup s;
                const uint32_t outcome = setup_triangle(v0, v1, v2, j.width, j.height, cull_none, s);
                if (outcome != kDraw) {
                    best = better_outcome(best, outcome);
                    continue;
                }
                uint64_t inside = 0;
                for (int32_t y = s.y_lo; y <= s.y_hi; y++)
                    for (int32_t x = s.x_lo; x <= s.x_hi; x++) {
                        const int32_t px = 256 * x + 128, py = 256 * y + 128;
                        if (edge_at(s, 0, px, py) < 0 || edge_at(s, 1, px, py) < 0 || edge_at(s, 2, px, py) < 0) continue;
                        inside++;
                        emit(s, x, y);
                    }
                if (inside != 0) best = kDraw;
            }
            if (pc.count == 0u) best = kClipSkipped;
            switch (best) {
            case kClipSkipped: st.clip_skipped++; break;
            case kGuardSkipped: st.guard_skipped++; break;
            case kBackFacing: st.back_facing++; break;
            case kNoCoverage: st.no_coverage++; break;
            default: break;
            }
        }
    }
    if (stats) *stats = st;
}

} // namespace

void raster_depth(const HostJob &j, OrbitRasterStats *stats, int32_t *command_error) {
    raster_into(j, DepthSink{j.depth}, j.depth != nullptr, 0u, stats, command_error);
}

void raster_visibility(const HostJob &j, uint64_t *visibility, uint32_t command_base, OrbitRasterStats *stats,
                       int32_t *command_error) {
    if ((uint64_t)command_base + j.max_commands > ORBIT_VIS_MAX_COMMANDS) throw Panic("raster_visibility: command_base + max_commands");
    raster_into(j, VisibilitySink{visibility}, visibility != nullptr, command_base, stats, command_error);
}

void visibility_resolve(const uint64_t *visibility, uint32_t width, uint32_t height, uint32_t command_base,
                        uint32_t max_commands, float *depth, uint32_t *command_pixels, OrbitVisibilityStats *stats) {
    if (!visibility) throw Panic("visibility_resolve: NULL argument");
    if (!depth && !command_pixels && !stats) throw Panic("visibility_resolve: no output");
    if (width == 0 || height == 0 || width > ORBIT_RASTER_MAX_DIM || height > ORBIT_RASTER_MAX_DIM)
        throw Panic("visibility_resolve: target size");
    if ((uint64_t)command_base + max_commands > ORBIT_VIS_MAX_COMMANDS) throw Panic("visibility_resolve: command_base + max_commands");
    OrbitVisibilityStats st{};
    if (command_pixels) std::memset(command_pixels, 0, (size_t)max_commands * 4);
    for (size_t p = 0; p < (size_t)width * height; p++) {
        const uint64_t word = visibility[p];
        if (depth) {
            const uint32_t bits = (uint32_t)(word >> 32);
            std::memcpy(depth + p, &bits, 4);
        }
        if (word == 0) continue;
        st.covered_pixels++;
        const uint32_t id = (uint32_t)(word >> 8) & 0xFFFFFFu;
        if (id < command_base || id - command_base >= max_commands) {
            st.foreign_pixels++;
        } else if (command_pixels && command_pixels[id - command_base]++ == 0) {
            st.visible_commands++;
        }
    }
    if (stats) *stats = st;
}

void visibility_compact(const OrbitVisibilityCompact &j, int32_t *status) {
    const bool cut = (j.flags & ORBIT_COMPACT_TRIANGLES) != 0u;
    if (j.flags & ~ORBIT_COMPACT_TRIANGLES) throw Panic("visibility_compact: unknown flags");
    if (!j.visibility || !j.draw_commands || !j.triangle_masks || !j.visible_commands) throw Panic("visibility_compact: NULL argument");
    if (cut && (!j.meshlet_data || !j.visible_data)) throw Panic("visibility_compact: ORBIT_COMPACT_TRIANGLES without meshlet_data or visible_data");
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        throw Panic("visibility_compact: target size");
    if ((uint64_t)j.command_base + j.max_commands > ORBIT_VIS_MAX_COMMANDS) throw Panic("visibility_compact: command_base + max_commands");
    if (j.visible_data_words > (1u << 30)) throw Panic("visibility_compact: visible_data_words");
    const uint32_t *commands = static_cast<const uint32_t *>(j.draw_commands);
    uint32_t *out = static_cast<uint32_t *>(j.visible_commands);
    const uint32_t n = commands[0] < j.max_commands ? commands[0] : j.max_commands;
    OrbitVisibilityCompactStats st{};
    int32_t latched = ORBIT_OK;
    // C1
    std::memset(j.triangle_masks, 0, (size_t)j.max_commands * 32);
    for (size_t p = 0; p < (size_t)j.width * j.height; p++) {
        const uint64_t word = j.visibility[p];
        if (word == 0) continue;
        st.covered_pixels++;
        const uint32_t id = (uint32_t)(word >> 8) & 0xFFFFFFu, t = (uint32_t)word & 255u;
        if (id < j.command_base || id - j.command_base >= n) {
            st.foreign_pixels++;
            continue;
        }
        j.triangle_masks[8u * (size_t)(id - j.command_base) + (t >> 5)] |= 1u << (t & 31u);
    }
    // C2-C5, command after command
    const uint8_t *data_bytes = reinterpret_cast<const uint8_t *>(j.meshlet_data);
    uint64_t next_word = 0; // base of the next visible consistent command
    bool dropping = false;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t *mask = j.triangle_masks + 8u * (size_t)k, *cmd = commands + 1u + 7u * (size_t)k;
        const uint32_t nt = cmd[0] / 3u, first_index = cmd[2], index_base = cmd[3], first_word = first_index / 4u;
        uint32_t m = 0;
        bool beyond = false;
        for (uint32_t t = 0; t < 256u; t++)
            if (mask[t >> 5] >> (t & 31u) & 1u) {
                m++;
                if (t >= nt) beyond = true;
            }
        if (m == 0) continue;
        bool consistent = nt <= 256u && !beyond;
        const uint32_t vcount = first_word - index_base;
        if (cut && (first_word < index_base || vcount > 255u || (uint64_t)first_word > j.meshlet_data_words ||
                    ((uint64_t)first_index + 3ull * nt + 3ull) / 4ull > j.meshlet_data_words))
            consistent = false;
        if (!consistent) {
            st.range_errors++;
            latched = ORBIT_E_RANGE;
            continue;
        }
        const uint32_t jv = st.visible_commands++;
        st.visible_triangles += m;
        const uint32_t size = cut ? vcount + (3u * m + 3u) / 4u : 0u;
        const uint64_t base = next_word;
        next_word += size;
        if (dropping || jv >= j.visible_capacity || (cut && base + size > j.visible_data_words)) {
            dropping = true; // (base + size only grows: nothing behind a dropped command fits)
            st.dropped_commands++;
            continue;
        }
        st.written_commands++;
        uint32_t *dst = out + 1u + 7u * (size_t)jv;
        std::memcpy(dst, cmd, 28);
        if (j.visible_ids) j.visible_ids[jv] = j.command_base + k;
        if (!cut) continue;
        uint32_t *region = j.visible_data + base;
        dst[0] = 3u * m, dst[2] = 4u * ((uint32_t)base + vcount), dst[3] = (uint32_t)base;
        std::memcpy(region, j.meshlet_data + index_base, (size_t)vcount * 4);
        uint8_t *corners = reinterpret_cast<uint8_t *>(region + vcount);
        std::memset(corners, 0, (size_t)(size - vcount) * 4);
        for (uint32_t t = 0, r = 0; t < nt; t++)
            if (mask[t >> 5] >> (t & 31u) & 1u) std::memcpy(corners + 3u * (size_t)r++, data_bytes + (size_t)first_index + 3u * (size_t)t, 3);
    }
    out[0] = st.written_commands;
    st.data_words_needed = next_word > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)next_word;
    if (st.dropped_commands != 0 && latched == ORBIT_OK) latched = ORBIT_E_CAPACITY;
    if (j.stats) *j.stats = st;
    if (status) *status = latched;
}

void visibility_surface(const OrbitVisibilitySurface &j, int32_t *status) {
    if (j.flags & ~ORBIT_SURFACE_CLEAR) throw Panic("visibility_surface: unknown flags");
    if (!j.visibility || !j.draw_commands || !j.meshlet_data || !j.vertices || !j.entity_data) throw Panic("visibility_surface: NULL argument");
    if (!j.bary && !j.grad && !j.triangle) throw Panic("visibility_surface: no output");
    if ((uint64_t)j.vertex_stride < (uint64_t)j.position_offset + 12u || (j.vertex_stride & 3u) || (j.position_offset & 3u))
        throw Panic("visibility_surface: vertex_stride / position_offset");
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        throw Panic("visibility_surface: target size");
    if ((uint64_t)j.command_base + j.max_commands > ORBIT_VIS_MAX_COMMANDS) throw Panic("visibility_surface: command_base + max_commands");
    if (j.triangle && j.vertex_count > (1ull << 32)) throw Panic("visibility_surface: triangle with vertex_count > 2^32");
    const size_t pixels = (size_t)j.width * j.height;
    if (j.flags & ORBIT_SURFACE_CLEAR) { // S7
        if (j.bary) std::memset(j.bary, 0, pixels * 8);
        if (j.grad) std::memset(j.grad, 0, pixels * 16);
        if (j.triangle) std::memset(j.triangle, 0xFF, pixels * 16);
    }
    const uint32_t *commands = static_cast<const uint32_t *>(j.draw_commands);
    const uint32_t n = commands[0] < j.max_commands ? commands[0] : j.max_commands;
    OrbitSurfaceStats st{};
    for (size_t p = 0; p < pixels; p++) {
        const uint64_t word = j.visibility[p];
        if (word == 0) continue;
        st.covered_pixels++;
        const uint32_t id = (uint32_t)(word >> 8) & 0xFFFFFFu, t = (uint32_t)word & 255u;
        if (id < j.command_base || id - j.command_base >= n) { // S1
            st.foreign_pixels++;
            continue;
        }
        const uint32_t k = id - j.command_base;
        const SurfaceCommand cmd = surface_command(j, k);
        bool command_ok = cmd.in_range; // R9, V3: the command whole, as the drawing call asked
        for (uint32_t v = 0; v < cmd.vcount && command_ok; v++) command_ok = surface_index_word_ok(j, cmd, v);
        for (uint32_t b = 0; b < 3u * cmd.nt && command_ok; b++) command_ok = surface_corner_byte_ok(j, cmd, b);
        SurfaceTriangle tri;
        surface_triangle(j, k, t, command_ok, tri);
        float out[6];
        bool degenerate;
        const uint32_t verdict = surface_pixel(tri, (int32_t)(p % j.width), (int32_t)(p / j.width), (uint32_t)(word >> 32), out, degenerate);
        if (verdict == kSurfaceUnsupported) st.unsupported_pixels++;
        if (verdict == kSurfaceStale) st.stale_pixels++;
        if (verdict != kSurfaceWritten) continue;
        st.written_pixels++;
        if (degenerate) st.degenerate_pixels++;
        if (j.bary) std::memcpy(j.bary + 2 * p, out, 8);
        if (j.grad) std::memcpy(j.grad + 4 * p, out + 2, 16);
        if (j.triangle) std::memcpy(j.triangle + 4 * p, tri.ids, 16);
    }
    if (j.stats) *j.stats = st;
    if (status) *status = st.stale_pixels != 0 ? ORBIT_E_RANGE : ORBIT_OK;
}

void visibility_surface_drawn(const OrbitVisibilitySurface &j, uint32_t raster_flags, int32_t *status) {
    if (raster_flags & ~(ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD)) throw Panic("visibility_surface_drawn: unknown raster_flags");
    if (j.flags & ~ORBIT_SURFACE_CLEAR) throw Panic("visibility_surface_drawn: unknown flags");
    if (!j.visibility || !j.draw_commands || !j.meshlet_data || !j.vertices || !j.entity_data) throw Panic("visibility_surface_drawn: NULL argument");
    if (!j.bary && !j.grad && !j.triangle) throw Panic("visibility_surface_drawn: no output");
    if ((uint64_t)j.vertex_stride < (uint64_t)j.position_offset + 12u || (j.vertex_stride & 3u) || (j.position_offset & 3u))
        throw Panic("visibility_surface_drawn: vertex_stride / position_offset");
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        throw Panic("visibility_surface_drawn: target size");
    if ((uint64_t)j.command_base + j.max_commands > ORBIT_VIS_MAX_COMMANDS) throw Panic("visibility_surface_drawn: command_base + max_commands");
    if (j.triangle && j.vertex_count > (1ull << 32)) throw Panic("visibility_surface_drawn: triangle with vertex_count > 2^32");
    const size_t pixels = (size_t)j.width * j.height;
    if (j.flags & ORBIT_SURFACE_CLEAR) { // S7
        if (j.bary) std::memset(j.bary, 0, pixels * 8);
        if (j.grad) std::memset(j.grad, 0, pixels * 16);
        if (j.triangle) std::memset(j.triangle, 0xFF, pixels * 16);
    }
    const uint32_t *commands = static_cast<const uint32_t *>(j.draw_commands);
    const uint32_t n = commands[0] < j.max_commands ? commands[0] : j.max_commands;
    OrbitSurfaceStats st{};
    for (size_t p = 0; p < pixels; p++) {
        const uint64_t word = j.visibility[p];
        if (word == 0) continue;
        st.covered_pixels++;
        const uint32_t id = (uint32_t)(word >> 8) & 0xFFFFFFu, t = (uint32_t)word & 255u;
        if (id < j.command_base || id - j.command_base >= n) { // S1
            st.foreign_pixels++;
            continue;
        }
        const uint32_t k = id - j.command_base;
        const SurfaceCommand cmd = surface_command(j, k);
        bool command_ok = cmd.in_range; // R9, V3
        for (uint32_t v = 0; v < cmd.vcount && command_ok; v++) command_ok = surface_index_word_ok(j, cmd, v);
        for (uint32_t b = 0; b < 3u * cmd.nt && command_ok; b++) command_ok = surface_corner_byte_ok(j, cmd, b);
        SurfaceTriangle tri;
        SurfaceSlow slow;
        surface_triangle_drawn(j, k, t, command_ok, raster_flags, tri, slow); // S2d
        float out[6];
        bool degenerate;
        uint32_t cand_flags;
        const uint32_t verdict = surface_pixel_drawn(tri, slow, (int32_t)(p % j.width), (int32_t)(p / j.width), (uint32_t)(word >> 32), out,
                                                     degenerate, cand_flags);
        if (verdict == kSurfaceUnsupported) st.unsupported_pixels++;
        if (verdict == kSurfaceStale) st.stale_pixels++;
        if (verdict != kSurfaceWritten) continue;
        st.written_pixels++;
        if (degenerate) st.degenerate_pixels++;
        if (cand_flags & kCandCut) st.cut_pixels++;
        if (cand_flags & kCandWide) st.wide_pixels++;
        if (j.bary) std::memcpy(j.bary + 2 * p, out, 8);
        if (j.grad) std::memcpy(j.grad + 4 * p, out + 2, 16);
        if (j.triangle) std::memcpy(j.triangle + 4 * p, tri.ids, 16);
    }
    if (j.stats) *j.stats = st;
    if (status) *status = st.stale_pixels != 0 ? ORBIT_E_RANGE : ORBIT_OK;
}

void surface_fragments(const OrbitSurfaceFragments &j, int32_t *status) {
    if (j.flags & ~ORBIT_FRAGMENTS_CLEAR) throw Panic("surface_fragments: unknown flags");
    if (!j.visibility || !j.draw_commands || !j.meshlets || !j.bary || !j.triangle || !j.vertices || !j.entity_data)
        throw Panic("surface_fragments: NULL argument");
    if (!j.world_pos && !j.normal && !j.tangent && !j.uv && !j.uv_grad && !j.material) throw Panic("surface_fragments: no output");
    if (j.uv_grad && !j.grad) throw Panic("surface_fragments: uv_grad needs grad");
    if ((j.vertex_stride | j.position_offset | j.normal_offset | j.uv_offset | j.tangent_offset) & 3u)
        throw Panic("surface_fragments: vertex_stride / offsets no multiples of 4");
    if ((uint64_t)j.vertex_stride < (uint64_t)j.position_offset + 12u || (uint64_t)j.vertex_stride < (uint64_t)j.normal_offset + 4u ||
        (uint64_t)j.vertex_stride < (uint64_t)j.uv_offset + 8u || (uint64_t)j.vertex_stride < (uint64_t)j.tangent_offset + 4u)
        throw Panic("surface_fragments: vertex_stride below an attribute's end");
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        throw Panic("surface_fragments: target size");
    if ((uint64_t)j.command_base + j.max_commands > ORBIT_VIS_MAX_COMMANDS) throw Panic("surface_fragments: command_base + max_commands");
    if (j.vertex_count > (1ull << 32)) throw Panic("surface_fragments: vertex_count > 2^32");
    const size_t pixels = (size_t)j.width * j.height;
    if (j.flags & ORBIT_FRAGMENTS_CLEAR) { // F8
        if (j.world_pos) std::memset(j.world_pos, 0, pixels * 16);
        if (j.normal) std::memset(j.normal, 0, pixels * 12);
        if (j.tangent) std::memset(j.tangent, 0, pixels * 16);
        if (j.uv) std::memset(j.uv, 0, pixels * 8);
        if (j.uv_grad) std::memset(j.uv_grad, 0, pixels * 16);
        if (j.material) std::memset(j.material, 0xFF, pixels * 4);
    }
    const uint32_t *commands = static_cast<const uint32_t *>(j.draw_commands);
    const uint32_t n = commands[0] < j.max_commands ? commands[0] : j.max_commands;
    OrbitFragmentStats st{};
    for (size_t p = 0; p < pixels; p++) {
        const uint64_t word = j.visibility[p];
        if (word == 0) continue;
        st.covered_pixels++;
        const uint32_t id = (uint32_t)(word >> 8) & 0xFFFFFFu;
        if (id < j.command_base || id - j.command_base >= n) { // F1
            st.foreign_pixels++;
            continue;
        }
        float out[kFragmentFloats];
        uint32_t material;
        bool degenerate;
        const uint32_t verdict = fragment_pixel(j, id - j.command_base, p, out, material, degenerate);
        if (verdict == kFragmentUnshaded) st.unshaded_pixels++;
        if (verdict == kFragmentStale) st.stale_pixels++;
        if (verdict != kFragmentWritten) continue;
        st.written_pixels++;
        if (degenerate) st.degenerate_pixels++;
        if (j.world_pos) std::memcpy(j.world_pos + 4 * p, out, 16);
        if (j.normal) std::memcpy(j.normal + 3 * p, out + 4, 12);
        if (j.tangent) std::memcpy(j.tangent + 4 * p, out + 7, 16);
        if (j.uv) std::memcpy(j.uv + 2 * p, out + 11, 8);
        if (j.uv_grad) std::memcpy(j.uv_grad + 4 * p, out + 13, 16);
        if (j.material) j.material[p] = material;
    }
    if (j.stats) *j.stats = st;
    if (status) *status = st.stale_pixels != 0 ? ORBIT_E_RANGE : ORBIT_OK;
}

// what both shade mirrors throw for the base job
static void check_fragments_shade(const OrbitFragmentsShade &j) {
    const uint32_t known = ORBIT_SHADE_CLEAR | ORBIT_SHADE_FORCE_PER_LANE | ORBIT_SHADE_FORCE_STAGED;
    if (j.flags & ~known) throw Panic("fragments_shade: unknown flags");
    if ((j.flags & ORBIT_SHADE_FORCE_PER_LANE) && (j.flags & ORBIT_SHADE_FORCE_STAGED)) throw Panic("fragments_shade: both forms forced");
    if (j.render_mode != 0u && j.render_mode != 8u) throw Panic("fragments_shade: render_mode");
    if (j.width == 0 || j.height == 0 || j.width > ORBIT_RASTER_MAX_DIM || j.height > ORBIT_RASTER_MAX_DIM)
        throw Panic("fragments_shade: target size");
    if (j.cluster_count[0] == 0 || j.cluster_count[1] == 0 || j.cluster_count[2] == 0 || j.tile_size_px == 0)
        throw Panic("fragments_shade: a zero in cluster_count or tile_size_px");
    if (j.cluster_count[2] > 32u) throw Panic("fragments_shade: cluster_count[2] > 32");
    if ((uint64_t)j.cluster_count[0] * j.cluster_count[1] > (1ull << 31) / j.cluster_count[2]) throw Panic("fragments_shade: clusters > 2^31");
    if ((j.flags & ORBIT_SHADE_FORCE_STAGED) && j.tile_size_px % 8u != 0u) throw Panic("fragments_shade: staged needs tile_size_px % 8 == 0");
    if (!j.visibility || !j.world_pos || !j.normal || !j.material || !j.materials || !j.lights || !j.cluster_offset_image ||
        !j.light_index_buffer || !j.color)
        throw Panic("fragments_shade: NULL argument");
}

// The three shade mirrors' loop (L1-L9 with what the tier adds) is shade_mirror; a tier's host half is the overloads in
// front of it: the planes L9 / H10 fill, what a written pixel counts and stores beside the base job's, the stats blocks.
namespace {
struct ShadeTally {
    OrbitShadeStats st{};
    OrbitShadowStats sh{};
    OrbitSkyStats sky{};
};
struct SkyCounting { // sky_common.h's and the sampler's census hook: counts into the tests' block, or nowhere
    uint64_t *census;
    void operator()(uint32_t index) const {
        if (census) census[index]++;
    }
};

void mirror_clear(const OrbitFragmentsShade &, size_t) {}
void mirror_clear(const OrbitFragmentsShadeShadowed &j, size_t pixels) { // H10
    if (j.shadow_factor) std::fill(j.shadow_factor, j.shadow_factor + pixels, 1.0f);
    if (j.cascade) std::fill(j.cascade, j.cascade + pixels, kNone);
}
void mirror_clear(const OrbitFragmentsShadeSky &j, size_t pixels) { mirror_clear(j.shadowed, pixels); }

void mirror_written(const OrbitFragmentsShade &, size_t, const ShadeTier::Extra &, ShadeTally &) {}
void mirror_written(const OrbitFragmentsShadeShadowed &j, size_t p, const ShadowPixel &sp, ShadeTally &t) {
    if (sp.marks & kShadowEvaluated) t.sh.shadowed_pixels++;
    if (sp.marks & kShadowOutOfCascades) t.sh.no_cascade_pixels++;
    if (sp.marks & kShadowEarlyOut) t.sh.early_out_pixels++;
    t.sh.shadow_evaluations += sp.evaluations;
    if (j.shadow_factor) j.shadow_factor[p] = sp.factor;
    if (j.cascade) j.cascade[p] = sp.cascade;
}
void mirror_written(const OrbitFragmentsShadeSky &j, size_t p, const SkyExtra &e, ShadeTally &t) {
    mirror_written(j.shadowed, p, e.sp, t);
    if (e.k.evaluations != 0u) t.sky.sky_lit_pixels++;
    t.sky.sky_evaluations += e.k.evaluations;
    t.sky.bad_directions += e.k.bad;
}

void mirror_stats(const OrbitFragmentsShade &j, const ShadeTally &t) {
    if (j.stats) *j.stats = t.st;
}
void mirror_stats(const OrbitFragmentsShadeShadowed &j, const ShadeTally &t) {
    mirror_stats(j.shade, t);
    if (j.shadow_stats) *j.shadow_stats = t.sh;
}
void mirror_stats(const OrbitFragmentsShadeSky &j, const ShadeTally &t) {
    mirror_stats(j.shadowed, t);
    if (j.sky_stats) *j.sky_stats = t.sky;
}

// uncovered(x, y, p, tally): what the call does with a pixel whose visibility word is 0
template <class Tier, class Uncovered>
void shade_mirror(const Tier &tier, const typename Tier::Job &j, int32_t *status, Uncovered uncovered) {
    const OrbitFragmentsShade &b = Tier::base(j);
    const size_t pixels = (size_t)b.width * b.height;
    if (b.flags & ORBIT_SHADE_CLEAR) { // L9
        std::memset(b.color, 0, pixels * 16);
        if (b.lights_walked) std::memset(b.lights_walked, 0, pixels * 4);
        mirror_clear(j, pixels);
    }
    ShadeTally t;
    for (size_t p = 0; p < pixels; p++) {
        const uint64_t word = b.visibility[p];
        const uint32_t x = (uint32_t)(p % b.width), y = (uint32_t)(p / b.width);
        if (word == 0) {
            uncovered(x, y, p, t);
            continue;
        }
        t.st.covered_pixels++;
        const uint32_t slice = shade_slice_canonical(b.z_near, bits_float((int32_t)(uint32_t)(word >> 32)), b.z_scale, b.z_bias); // L2
        float color[4];
        uint32_t n, marks;
        typename Tier::Extra e;
        Tier::reset(e);
        const uint32_t verdict = shade_walk_pixel(tier, j, x, y, p, slice, color, n, marks, e);
        if (verdict == kShadeUnshaded) t.st.unshaded_pixels++;
        if (verdict == kShadeStale) t.st.stale_pixels++;
        if (verdict != kShadeWritten) continue;
        t.st.written_pixels++;
        if (marks & kShadeOutside) t.st.outside_pixels++;
        if (marks & kShadeDegenerate) t.st.degenerate_pixels++;
        if (marks & kShadeTextured) t.st.textured_pixels++;
        if (marks & kShadeUnserved) t.st.unserved_pixels++;
        std::memcpy(b.color + 4 * p, color, 16);
        if (b.lights_walked) b.lights_walked[p] = n;
        mirror_written(j, p, e, t);
    }
    mirror_stats(j, t);
    if (status) *status = t.st.stale_pixels != 0 ? ORBIT_E_RANGE : ORBIT_OK;
}
const auto kUncoveredStays = [](uint32_t, uint32_t, size_t, ShadeTally &) {};
} // namespace

void fragments_shade(const OrbitFragmentsShade &j, int32_t *status) {
    check_fragments_shade(j);
    shade_mirror(ShadeTier{}, j, status, kUncoveredStays);
}

void fragments_shade_shadowed(const OrbitFragmentsShadeShadowed &j, int32_t *status) {
    check_fragments_shade(j.shade);
    if (j.shadow_count > 0u) {
        if (!j.shadows || !j.shadow_maps) throw Panic("fragments_shade_shadowed: shadow_count > 0 with shadows or shadow_maps NULL");
        if (j.shadow_resolution == 0u || j.shadow_resolution > ORBIT_RASTER_MAX_DIM) throw Panic("fragments_shade_shadowed: shadow_resolution");
        if ((uint64_t)j.shadow_map_count * j.shadow_resolution * j.shadow_resolution > (1ull << 31))
            throw Panic("fragments_shade_shadowed: shadow maps > 2^31 floats");
    }
    shade_mirror(ShadowedTier{}, j, status, kUncoveredStays);
}

void fragments_shade_sky(const OrbitFragmentsShadeSky &js, int32_t *status, uint64_t *census) {
    if (const char *wrong = sky_check(js)) throw Panic(std::string("fragments_shade_sky: ") + wrong);
    const SkyCounting counting{census};
    const bool box = sky_box_given(js);
    shade_mirror(SkyTier<true, SkyCounting>{counting}, js, status, [&](uint32_t x, uint32_t y, size_t p, ShadeTally &t) { // K9
        if (!box) return;
        float color[4];
        if (!sky_box_pixel(js, x, y, color, counting)) t.sky.bad_directions++;
        t.sky.skybox_pixels++;
        std::memcpy(js.shadowed.shade.color + 4 * p, color, 16);
    });
}

void shadow_rotation(uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, float *theta, float *sine, float *cosine) {
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) {
            const size_t i = (size_t)y * width + x;
            theta[i] = shadow_theta(x0 + x, y0 + y);
            shadow_sincos(theta[i], sine[i], cosine[i]);
        }
}

} // namespace raster
} // namespace orbit
