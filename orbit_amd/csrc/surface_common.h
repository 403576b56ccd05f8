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

// ---- orbit_visibility_surface_drawn (S2d, S3c, S3w): the keys S2 leaves out -------------------------
// A key of class (b) or (c) whose flags are given has one or two CANDIDATES: the wide triangle itself, or the pieces of
// R3c.  surface_triangle_drawn is S2d per (command, triangle): surface_triangle's work for class (a), whose bytes it
// must give, so its head and tail are restated here rather than shared (surface_triangle stays the code it was), and
// the candidates otherwise.  surface_candidate_pixel is the work per pixel and candidate: R6 / R6w, R7 / R7w, S3w, S3c.
constexpr uint32_t kSurfaceSlow = 3u; // SurfaceTriangle::flags' verdict of a key with candidates: ask them
constexpr uint32_t kCandDraws = 1u, kCandSwapped = 2u, kCandWide = 4u, kCandCut = 8u; // SurfaceCandidate::flags

struct SurfaceCandidate { // what a pixel needs of a candidate: 28 words
    int64_t x[3], y[3]; // R5's or R5w's normalised vertices
    float iw[3];        // 1 / w of the same
    float t[3];         // S3c's t of P_0, P_1, P_2 (piece_vertices' order); 0 for an original corner
    uint32_t io;        // S3c's i | o << 2 of P_q at bits 4 q; i == o for an original corner
    uint32_t plane[6];  // R7's d0, gx, gy as three floats, or R7w's as three doubles
    uint32_t flags;
};

struct SurfaceSlow {
    SurfaceCandidate c[2];
    uint32_t count; // 1 or 2
    uint32_t miss;  // the verdict of a pixel that no candidate owns: kSurfaceStale or kSurfaceUnsupported
};

ORBIT_RASTER_FN void candidate_none(SurfaceCandidate &c) {
    for (int i = 0; i < 3; i++) c.x[i] = c.y[i] = 0, c.iw[i] = c.t[i] = 0.0f;
    for (int i = 0; i < 6; i++) c.plane[i] = 0u;
    c.io = c.flags = 0u;
}

// R3c's t and the w of N(i, o), which clip_new_vertex computes and drops: its expressions, its roundings
ORBIT_RASTER_FN void clip_new_vertex_tw(const Clip &i, const Clip &o, float &t, float &w) {
    const float b_i = i.w - i.z, b_o = o.w - o.z;
    const float den = b_i - b_o;
    t = b_i / den;
    w = i.w + t * (o.w - i.w);
}

// the candidate of the vertices (v0, v1, v2), none out of band, none failing R3, of clip w (w0, w1, w2)
ORBIT_RASTER_FN void surface_candidate(const Vertex &v0, const Vertex &v1, const Vertex &v2, float w0, float w1, float w2,
                                       uint32_t width, uint32_t height, uint32_t cut_flag, SurfaceCandidate &c) {
    bool swapped;
    if (is_wide_triangle(v0, v1, v2)) {
        SetupW s;
        if (setup_triangle_wide(v0, v1, v2, width, height, true, s) != kDraw) return;
        swapped = s.ax[1] != wide_coord(v1, v1.X) || s.ay[1] != wide_coord(v1, v1.Y);
        for (int i = 0; i < 3; i++) c.x[i] = s.ax[i], c.y[i] = s.ay[i];
        __builtin_memcpy(&c.plane[0], &s.d0, 8), __builtin_memcpy(&c.plane[2], &s.gx, 8), __builtin_memcpy(&c.plane[4], &s.gy, 8);
        c.flags = kCandDraws | kCandWide | cut_flag;
    } else {
        Setup s;
        if (setup_triangle(v0, v1, v2, width, height, true, s) != kDraw) return;
        swapped = s.ax[1] != v1.X || s.ay[1] != v1.Y;
        for (int i = 0; i < 3; i++) c.x[i] = s.ax[i], c.y[i] = s.ay[i];
        c.plane[0] = (uint32_t)float_bits(s.d0), c.plane[1] = (uint32_t)float_bits(s.gx), c.plane[2] = (uint32_t)float_bits(s.gy);
        c.flags = kCandDraws | cut_flag;
    }
    c.iw[0] = 1.0f / w0, c.iw[1] = 1.0f / (swapped ? w2 : w1), c.iw[2] = 1.0f / (swapped ? w1 : w2);
    if (swapped) c.flags |= kCandSwapped;
}

// piece q of pc as a candidate, of clip w (w0, w1, w2) -> it was left out as not covered by the flags.  (t and io of a
// candidate that does not draw are not read.)
ORBIT_RASTER_FN bool surface_piece(const Pieces &pc, uint32_t q, bool wide, float w0, float w1, float w2, uint32_t width,
                                   uint32_t height, SurfaceCandidate &c) {
    Vertex p0, p1, p2;
    piece_vertices(pc, q, p0, p1, p2);
    const uint32_t pflags = p0.flags | p1.flags | p2.flags;
    if (pflags & kOutOfBand) return false; // left out
    if ((pflags & kGuardFail) && !wide) return true;
    surface_candidate(p0, p1, p2, w0, w1, w2, width, height, kCandCut, c);
    return false;
}

// S2d of triangle t of command k < n, up to the setups -> the key has candidates (out.flags = kSurfaceSlow, `slow` is
// made); otherwise out is surface_triangle's, with the verdict of the classes that need no candidate
ORBIT_RASTER_FN bool surface_triangle_drawn(const OrbitVisibilitySurface &j, uint32_t k, uint32_t t, bool command_ok,
                                            uint32_t raster_flags, SurfaceTriangle &out, SurfaceSlow &slow) {
    for (int i = 0; i < 3; i++) out.ax[i] = out.ay[i] = 0, out.iw[i] = 0.0f;
    out.d0 = out.gx = out.gy = 0.0f;
    for (int i = 0; i < 4; i++) out.ids[i] = 0u;
    out.flags = kSurfaceStale;
    if (!command_ok) return false;
    const SurfaceCommand cmd = surface_command(j, k);
    if (t >= cmd.nt) return false;
    const uint32_t entity = cmd.entity;
    const uint8_t *c = (const uint8_t *)j.meshlet_data + (size_t)cmd.first_index + 3u * (size_t)t;
    const uint64_t g0 = cmd.vertex_base + j.meshlet_data[(size_t)cmd.index_base + c[0]],
                   g1 = cmd.vertex_base + j.meshlet_data[(size_t)cmd.index_base + c[1]],
                   g2 = cmd.vertex_base + j.meshlet_data[(size_t)cmd.index_base + c[2]];
    out.ids[0] = entity, out.ids[1] = (uint32_t)g0, out.ids[2] = (uint32_t)g1, out.ids[3] = (uint32_t)g2;
    float mvp[16];
    mat4_mul(j.view_proj, j.entity_data[entity].model_matrix, mvp);
    const float w_f = (float)j.width, h_f = (float)j.height;
    const bool clip_near = (raster_flags & ORBIT_RASTER_CLIP_NEAR) != 0u, wide = (raster_flags & ORBIT_RASTER_WIDE_GUARD) != 0u;
    const uint64_t g[3] = {g0, g1, g2};
    Clip clip[3];
    Vertex v[3];
    for (int i = 0; i < 3; i++) {
        float pos[3];
        __builtin_memcpy(pos, (const uint8_t *)j.vertices + g[i] * j.vertex_stride + j.position_offset, 12);
        clip[i] = clip_position(mvp, pos[0], pos[1], pos[2]);
        v[i] = vertex_from_clip(clip[i], w_f, h_f, false, wide);
    }
    const uint32_t vflags = v[0].flags | v[1].flags | v[2].flags;
    if (!(vflags & (kClipFail | kGuardFail))) { // (a): surface_triangle's tail
        Setup s;
        if (setup_triangle(v[0], v[1], v[2], j.width, j.height, true, s) != kDraw) return false;
        const bool swapped = s.ax[1] != v[1].X || s.ay[1] != v[1].Y;
        for (int i = 0; i < 3; i++) out.ax[i] = s.ax[i], out.ay[i] = s.ay[i];
        out.iw[0] = 1.0f / clip[0].w, out.iw[1] = 1.0f / (swapped ? clip[2].w : clip[1].w), out.iw[2] = 1.0f / (swapped ? clip[1].w : clip[2].w);
        out.d0 = s.d0, out.gx = s.gx, out.gy = s.gy;
        out.flags = kSurfaceWritten | (swapped ? kSurfaceSwapped : 0u);
        return false;
    }
    candidate_none(slow.c[0]), candidate_none(slow.c[1]);
    slow.count = 1u, slow.miss = kSurfaceStale;
    if (!(vflags & kClipFail)) { // (b)
        if (!wide) {
            out.flags = kSurfaceUnsupported;
            return false;
        }
        if (vflags & kOutOfBand) return false; // the raster guard_skipped it
        surface_candidate(v[0], v[1], v[2], clip[0].w, clip[1].w, clip[2].w, j.width, j.height, 0u, slow.c[0]);
        slow.c[0].io = 0u | 0u << 2 | (1u | 1u << 2) << 4 | (2u | 2u << 2) << 8; // (not read: no kCandCut)
        out.flags = kSurfaceSlow;
        return true;
    }
    // (c)
    if (!clip_near) {
        out.flags = kSurfaceUnsupported;
        return false;
    }
    Pieces pc;
    clip_near_pieces(clip[0], clip[1], clip[2], w_f, h_f, pc, wide);
    if (pc.count == 0u) return false;
    // clip_near_pieces' rotation, as corner numbers: a = lone, b = lone + 1, c = lone + 2
    const bool in0 = clip_in(clip[0]), in1 = clip_in(clip[1]);
    const bool one_in = pc.count == 1u;
    const bool lone0 = in0 == one_in, lone1 = !lone0 && in1 == one_in;
    const uint32_t ia = lone0 ? 0u : lone1 ? 1u : 2u, ib = ia == 2u ? 0u : ia + 1u, ic = ib == 2u ? 0u : ib + 1u;
    const Clip ca = select_clip(lone0, clip[0], select_clip(lone1, clip[1], clip[2]));
    const Clip cb = select_clip(lone0, clip[1], select_clip(lone1, clip[2], clip[0]));
    const Clip cc = select_clip(lone0, clip[2], select_clip(lone1, clip[0], clip[1]));
    // u[0..3] of the fan: its corner pairs (i, o), its t and its w
    float tn0, wn0, tn1, wn1; // of n0 and n1
    clip_new_vertex_tw(select_clip(one_in, ca, cc), select_clip(one_in, cb, ca), tn0, wn0);
    clip_new_vertex_tw(select_clip(one_in, ca, cb), select_clip(one_in, cc, ca), tn1, wn1);
    const uint32_t io_n0 = one_in ? (ia | ib << 2) : (ic | ia << 2), io_n1 = one_in ? (ia | ic << 2) : (ib | ia << 2);
    const uint32_t io_u0 = one_in ? (ia | ia << 2) : (ib | ib << 2), io_u1 = one_in ? io_n0 : (ic | ic << 2);
    const float w_u0 = one_in ? ca.w : cb.w, w_u1 = one_in ? wn0 : cc.w, t_u1 = one_in ? tn0 : 0.0f;
    // one in: u = (a, n0, n1, n1); one out: u = (b, c, n0, n1)
    const uint32_t io_u2 = one_in ? io_n1 : io_n0, io_u3 = io_n1;
    const float w_u2 = one_in ? wn1 : wn0, t_u2 = one_in ? tn1 : tn0, w_u3 = wn1, t_u3 = tn1;
    slow.count = pc.count;
    // piece 0 = (u0, u1, u2), piece 1 = (u0, u2, u3); each written out, so that no record is indexed by a variable
    if (surface_piece(pc, 0u, wide, w_u0, w_u1, w_u2, j.width, j.height, slow.c[0])) slow.miss = kSurfaceUnsupported;
    slow.c[0].t[0] = 0.0f, slow.c[0].t[1] = t_u1, slow.c[0].t[2] = t_u2;
    slow.c[0].io = io_u0 | io_u1 << 4 | io_u2 << 8;
    if (pc.count > 1u) {
        if (surface_piece(pc, 1u, wide, w_u0, w_u2, w_u3, j.width, j.height, slow.c[1])) slow.miss = kSurfaceUnsupported;
        slow.c[1].t[0] = 0.0f, slow.c[1].t[1] = t_u2, slow.c[1].t[2] = t_u3;
        slow.c[1].io = io_u0 | io_u2 << 4 | io_u3 << 8;
    }
    out.flags = kSurfaceSlow;
    return true;
}

// S3w's e_j of a 128-bit edge value: R7w's conversion, then one rounding to float
ORBIT_RASTER_FN float edge_float_wide(int128_t e) {
    return (float)((double)(int64_t)(e >> 64) * 18446744073709551616.0 + (double)(uint64_t)e);
}

// S3c's weight of original corner c in the piece vertex with the pair io and the float t
ORBIT_RASTER_FN float piece_weight(uint32_t io, float t, uint32_t c) {
    const uint32_t i = io & 3u, o = io >> 2 & 3u;
    return c == i ? 1.0f - t : c == o ? t : 0.0f;
}

// S3, S3w or S3c from the three e_j of the candidate's normalised setup
ORBIT_RASTER_FN Bary bary_of_candidate(const SurfaceCandidate &c, const float *e) {
    const float q0 = e[1] * c.iw[0], q1 = e[2] * c.iw[1], q2 = e[0] * c.iw[2];
    const bool swapped = (c.flags & kCandSwapped) != 0u;
    Bary b;
    if (!(c.flags & kCandCut)) { // S3 as bary_at has it
        const float sum = (q0 + q1) + q2;
        const float l1 = q1 / sum, l2 = q2 / sum;
        b.l1 = swapped ? l2 : l1, b.l2 = swapped ? l1 : l2, b.positive = sum > 0.0f;
        return b;
    }
    const float Q0 = q0, Q1 = swapped ? q2 : q1, Q2 = swapped ? q1 : q2; // R5's swap undone: Q_i belongs to P_i
    float n[3];
    for (uint32_t k = 0; k < 3u; k++)
        n[k] = (Q0 * piece_weight(c.io & 15u, c.t[0], k) + Q1 * piece_weight(c.io >> 4 & 15u, c.t[1], k)) +
               Q2 * piece_weight(c.io >> 8 & 15u, c.t[2], k);
    const float sum = (n[0] + n[1]) + n[2];
    b.l1 = n[1] / sum, b.l2 = n[2] / sum, b.positive = sum > 0.0f;
    return b;
}

ORBIT_RASTER_FN Bary bary_at_candidate(const SurfaceCandidate &c, const Setup &s, int32_t px, int32_t py) {
    float e[3];
    for (int k = 0; k < 3; k++)
        e[k] = (float)(double)((int64_t)s.dx[k] * (int64_t)(py - s.ay[k]) - (int64_t)s.dy[k] * (int64_t)(px - s.ax[k]));
    return bary_of_candidate(c, e);
}
ORBIT_RASTER_FN Bary bary_at_candidate(const SurfaceCandidate &c, const SetupW &s, int32_t px, int32_t py) {
    float e[3];
    for (int k = 0; k < 3; k++)
        e[k] = edge_float_wide((int128_t)s.dx[k] * (int128_t)((int64_t)py - s.ay[k]) - (int128_t)s.dy[k] * (int128_t)((int64_t)px - s.ax[k]));
    return bary_of_candidate(c, e);
}

// S4, S5 of one owned sample of the candidate's setup (a Setup or a SetupW): surface_pixel's end
template <class AnySetup>
ORBIT_RASTER_FN void candidate_outputs(const SurfaceCandidate &c, const AnySetup &s, int32_t px, int32_t py, float *out, bool &degenerate) {
    const Bary b = bary_at_candidate(c, s, px, py), bx = bary_at_candidate(c, s, px + 256, py), by = bary_at_candidate(c, s, px, py + 256);
    out[0] = b.l1, out[1] = b.l2;
    out[2] = bx.positive ? bx.l1 - b.l1 : 0.0f, out[3] = bx.positive ? bx.l2 - b.l2 : 0.0f;
    out[4] = by.positive ? by.l1 - b.l1 : 0.0f, out[5] = by.positive ? by.l2 - b.l2 : 0.0f;
    bool all_finite = true;
    for (int i = 0; i < 6; i++) all_finite = finite_or_zero(out[i]) && all_finite;
    degenerate = !all_finite || !bx.positive || !by.positive;
}

// S2d's ownership of pixel (x, y), whose word's high half is depth_bits, by one candidate -> owned: out and degenerate as
// surface_pixel's.  The 128-bit arithmetic runs only for a wide candidate.
ORBIT_RASTER_FN bool surface_candidate_pixel(const SurfaceCandidate &c, int32_t x, int32_t y, uint32_t depth_bits, float *out, bool &degenerate) {
    degenerate = false;
    if (!(c.flags & kCandDraws)) return false;
    const int32_t px = 256 * x + 128, py = 256 * y + 128;
    if (c.flags & kCandWide) {
        SetupW s;
        for (int k = 0; k < 3; k++) s.ax[k] = c.x[k], s.ay[k] = c.y[k];
        for (int k = 0; k < 3; k++) { // setup_triangle_wide's expressions
            const int n = k == 2 ? 0 : k + 1;
            s.dx[k] = s.ax[n] - s.ax[k], s.dy[k] = s.ay[n] - s.ay[k];
            s.nb[k] = (s.dy[k] < 0 || (s.dy[k] == 0 && s.dx[k] > 0)) ? 0 : 1;
        }
        s.x_lo = s.x_hi = s.y_lo = s.y_hi = 0; // (not read)
        __builtin_memcpy(&s.d0, &c.plane[0], 8), __builtin_memcpy(&s.gx, &c.plane[2], 8), __builtin_memcpy(&s.gy, &c.plane[4], 8);
        if (!inside_wide(s, x, y)) return false;
        const float d = depth_at(s, px, py);
        if (!(d > 0.0f) || (uint32_t)float_bits(d) != depth_bits) return false;
        candidate_outputs(c, s, px, py, out, degenerate);
        return true;
    }
    Setup s;
    for (int k = 0; k < 3; k++) s.ax[k] = (int32_t)c.x[k], s.ay[k] = (int32_t)c.y[k];
    for (int k = 0; k < 3; k++) { // setup_triangle's expressions
        const int n = k == 2 ? 0 : k + 1;
        s.dx[k] = s.ax[n] - s.ax[k], s.dy[k] = s.ay[n] - s.ay[k];
        s.nb[k] = (s.dy[k] < 0 || (s.dy[k] == 0 && s.dx[k] > 0)) ? 0 : 1;
    }
    s.x_lo = s.x_hi = s.y_lo = s.y_hi = 0; // (not read)
    s.d0 = bits_float((int32_t)c.plane[0]), s.gx = bits_float((int32_t)c.plane[1]), s.gy = bits_float((int32_t)c.plane[2]);
    if (edge_at(s, 0, px, py) < 0 || edge_at(s, 1, px, py) < 0 || edge_at(s, 2, px, py) < 0) return false;
    const float d = depth_at(s, px, py);
    if (!(d > 0.0f) || (uint32_t)float_bits(d) != depth_bits) return false;
    candidate_outputs(c, s, px, py, out, degenerate);
    return true;
}

// S2d of an owned pixel whose key's lane made (t, slow) -> the verdict; *cand_flags: the owning candidate's flags
// (kCandCut, kCandWide count in cut_pixels, wide_pixels), 0 for class (a)
ORBIT_RASTER_FN uint32_t surface_pixel_drawn(const SurfaceTriangle &t, const SurfaceSlow &slow, int32_t x, int32_t y, uint32_t depth_bits,
                                             float *out, bool &degenerate, uint32_t &cand_flags) {
    cand_flags = 0u;
    const uint32_t verdict = surface_pixel(t, x, y, depth_bits, out, degenerate);
    if (verdict != kSurfaceSlow) return verdict;
    for (uint32_t q = 0; q < 2u; q++) {
        if (q >= slow.count) break;
        if (surface_candidate_pixel(slow.c[q], x, y, depth_bits, out, degenerate)) {
            cand_flags = slow.c[q].flags;
            return kSurfaceWritten;
        }
    }
    return slow.miss;
}

} // namespace raster
} // namespace orbit
