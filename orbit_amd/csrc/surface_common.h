// surface_common.h — the arithmetic of orbit_visibility_surface (include/orbit_abi_ext.h S2-S6), written
// once for the device kernel (visibility_surface.hip) and the host mirror (orbit_amd/host/orbit_raster.cpp).  Three steps:
// surface_command with its two content checks is R9 and V3 of a command; surface_triangle is S2's work per (command,
// triangle) — R1-R5 through raster_common.h, what S3 needs of the result — and surface_pixel is the work per pixel: R6's
// inside test, R7's depth against the word, S3-S5.  The device runs the first on a wave per distinct command of a tile,
// the second on a lane per distinct key and the third on a lane per pixel; the host runs all three per pixel.  Equal
// inputs, equal functions: equal bytes.
#pragma once
#include "../../include/orbit_abi_ext.h"
#include "raster_common.h"

namespace orbit {
namespace raster {

enum SurfaceVerdict : uint32_t { kSurfaceWritten = 0, kSurfaceUnsupported = 1, kSurfaceStale = 2 }; // of an owned pixel
constexpr uint32_t kSurfaceVerdictMask = 3u, kSurfaceSwapped = 4u; // SurfaceTriangle::flags

struct SurfaceTriangle { // what a pixel needs of its triangle: 17 words
    int32_t ax[3], ay[3]; // R5's normalised vertices, snapped
    float iw[3];          // S3's 1 / w of the same
    float d0, gx, gy;     // R7's plane
    uint32_t flags;       // the verdict so far | kSurfaceSwapped
    uint32_t ids[4];      // S6
};

struct SurfaceCommand { // R1's decode of one command and the checks of R9 and V3 that read nothing but its seven words
    uint32_t nt, first_index, index_base, vcount, entity;
    uint64_t vertex_base;
    bool in_range;
};

ORBIT_RASTER_FN SurfaceCommand surface_command(const OrbitVisibilitySurface &j, uint32_t k) {
    const uint32_t *cmd = (const uint32_t *)j.draw_commands + 1u + 7u * (size_t)k;
    SurfaceCommand c;
    const uint32_t index_count = cmd[0], first_word = cmd[2] / 4u;
    c.first_index = cmd[2], c.index_base = cmd[3], c.entity = cmd[4], c.vertex_base = cmd[5];
    c.nt = index_count / 3u;
    c.vcount = first_word - c.index_base; // (meaningful once first_word >= index_base)
    c.in_range = !(first_word < c.index_base || c.vcount > 255u || (uint64_t)first_word > j.meshlet_data_words ||
                   ((uint64_t)c.first_index + 3ull * c.nt + 3ull) / 4ull > j.meshlet_data_words || c.entity >= j.entity_count ||
                   c.nt > 256u);
    return c;
}

// R9's checks of the contents, one at a time (c.in_range holds): index word v < vcount, corner byte b < 3 * nt.  The host
// asks them in turn, the device a lane each.
ORBIT_RASTER_FN bool surface_index_word_ok(const OrbitVisibilitySurface &j, const SurfaceCommand &c, uint32_t v) {
    return c.vertex_base + j.meshlet_data[(size_t)c.index_base + v] < j.vertex_count;
}
ORBIT_RASTER_FN bool surface_corner_byte_ok(const OrbitVisibilitySurface &j, const SurfaceCommand &c, uint32_t b) {
    return ((const uint8_t *)j.meshlet_data)[(size_t)c.first_index + b] < c.vcount;
}

// S2 of triangle t of command k < n, up to the setup.  command_ok: the command passed R9 and V3 whole (surface_command's
// in_range and every index word and corner byte); without it nothing the command names is read.
ORBIT_RASTER_FN void surface_triangle(const OrbitVisibilitySurface &j, uint32_t k, uint32_t t, bool command_ok, SurfaceTriangle &out) {
    for (int i = 0; i < 3; i++) out.ax[i] = out.ay[i] = 0, out.iw[i] = 0.0f;
    out.d0 = out.gx = out.gy = 0.0f;
    for (int i = 0; i < 4; i++) out.ids[i] = 0u;
    out.flags = kSurfaceStale;
    if (!command_ok) return;
    const SurfaceCommand cmd = surface_command(j, k);
    if (t >= cmd.nt) return;
    const uint32_t entity = cmd.entity;
    const uint8_t *c = (const uint8_t *)j.meshlet_data + (size_t)cmd.first_index + 3u * (size_t)t;
    const uint64_t g0 = cmd.vertex_base + j.meshlet_data[(size_t)cmd.index_base + c[0]],
                   g1 = cmd.vertex_base + j.meshlet_data[(size_t)cmd.index_base + c[1]],
                   g2 = cmd.vertex_base + j.meshlet_data[(size_t)cmd.index_base + c[2]];
    out.ids[0] = entity, out.ids[1] = (uint32_t)g0, out.ids[2] = (uint32_t)g1, out.ids[3] = (uint32_t)g2;
    float mvp[16];
    mat4_mul(j.view_proj, j.entity_data[entity].model_matrix, mvp);
    const float w_f = (float)j.width, h_f = (float)j.height;
    const uint64_t g[3] = {g0, g1, g2};
    Clip clip[3];
    Vertex v[3];
    for (int i = 0; i < 3; i++) {
        float pos[3];
        __builtin_memcpy(pos, (const uint8_t *)j.vertices + g[i] * j.vertex_stride + j.position_offset, 12);
        clip[i] = clip_position(mvp, pos[0], pos[1], pos[2]);
        v[i] = vertex_from_clip(clip[i], w_f, h_f, false, false);
    }
    if ((v[0].flags | v[1].flags | v[2].flags) & (kClipFail | kGuardFail)) {
        out.flags = kSurfaceUnsupported;
        return;
    }
    Setup s;
    if (setup_triangle(v[0], v[1], v[2], j.width, j.height, true, s) != kDraw) return;
    const bool swapped = s.ax[1] != v[1].X || s.ay[1] != v[1].Y; // A != 0: vertices 1 and 2 differ
    for (int i = 0; i < 3; i++) out.ax[i] = s.ax[i], out.ay[i] = s.ay[i];
    out.iw[0] = 1.0f / clip[0].w, out.iw[1] = 1.0f / (swapped ? clip[2].w : clip[1].w), out.iw[2] = 1.0f / (swapped ? clip[1].w : clip[2].w);
    out.d0 = s.d0, out.gx = s.gx, out.gy = s.gy;
    out.flags = kSurfaceWritten | (swapped ? kSurfaceSwapped : 0u);
}

struct Bary { // S3 at one sample
    float l1, l2;
    bool positive; // s > 0
};

// S3: B(px, py) of the normalised setup; exchanged back to meshlet_data's corner order
ORBIT_RASTER_FN Bary bary_at(const Setup &s, const float *iw, bool swapped, int32_t px, int32_t py) {
    float e[3];
    for (int k = 0; k < 3; k++)
        e[k] = (float)(double)((int64_t)s.dx[k] * (int64_t)(py - s.ay[k]) - (int64_t)s.dy[k] * (int64_t)(px - s.ax[k]));
    const float q0 = e[1] * iw[0], q1 = e[2] * iw[1], q2 = e[0] * iw[2];
    const float sum = (q0 + q1) + q2;
    const float l1 = q1 / sum, l2 = q2 / sum;
    Bary b;
    b.l1 = swapped ? l2 : l1, b.l2 = swapped ? l1 : l2, b.positive = sum > 0.0f;
    return b;
}

ORBIT_RASTER_FN bool finite_or_zero(float &f) { // S5 of one float -> it was finite
    const bool finite = fabsf(f) < INFINITY; // false for NaN
    if (!finite) f = 0.0f;
    return finite;
}

// The rest of S2 and S3-S5 of pixel (x, y), whose word's high half is depth_bits -> the verdict; kSurfaceWritten:
// out[0..1] = bary, out[2..5] = grad, degenerate = S5's count of the pixel
ORBIT_RASTER_FN uint32_t surface_pixel(const SurfaceTriangle &t, int32_t x, int32_t y, uint32_t depth_bits, float *out, bool &degenerate) {
    degenerate = false;
    const uint32_t verdict = t.flags & kSurfaceVerdictMask;
    if (verdict != kSurfaceWritten) return verdict;
    Setup s;
    for (int k = 0; k < 3; k++) s.ax[k] = t.ax[k], s.ay[k] = t.ay[k];
    for (int k = 0; k < 3; k++) { // setup_triangle's expressions
        const int n = k == 2 ? 0 : k + 1;
        s.dx[k] = s.ax[n] - s.ax[k], s.dy[k] = s.ay[n] - s.ay[k];
        s.nb[k] = (s.dy[k] < 0 || (s.dy[k] == 0 && s.dx[k] > 0)) ? 0 : 1;
    }
    s.x_lo = s.x_hi = s.y_lo = s.y_hi = 0; // (not read)
    s.d0 = t.d0, s.gx = t.gx, s.gy = t.gy;
    const int32_t px = 256 * x + 128, py = 256 * y + 128;
    if (edge_at(s, 0, px, py) < 0 || edge_at(s, 1, px, py) < 0 || edge_at(s, 2, px, py) < 0) return kSurfaceStale;
    const float d = depth_at(s, px, py);
    if (!(d > 0.0f) || (uint32_t)float_bits(d) != depth_bits) return kSurfaceStale;
    const bool swapped = (t.flags & kSurfaceSwapped) != 0u;
    const Bary b = bary_at(s, t.iw, swapped, px, py), bx = bary_at(s, t.iw, swapped, px + 256, py), by = bary_at(s, t.iw, swapped, px, py + 256);
    out[0] = b.l1, out[1] = b.l2;
    out[2] = bx.positive ? bx.l1 - b.l1 : 0.0f, out[3] = bx.positive ? bx.l2 - b.l2 : 0.0f;
    out[4] = by.positive ? by.l1 - b.l1 : 0.0f, out[5] = by.positive ? by.l2 - b.l2 : 0.0f;
    bool all_finite = true;
    for (int i = 0; i < 6; i++) all_finite = finite_or_zero(out[i]) && all_finite;
    degenerate = !all_finite || !bx.positive || !by.positive;
    return kSurfaceWritten;
}

} // namespace raster
} // namespace orbit
