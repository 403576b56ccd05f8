// raster_common.h — the arithmetic of orbit_raster_depth (include/orbit_abi_ext.h R2-R7), written once
// for the device kernels (raster_walk.h) and the host mirror (orbit_amd/host/orbit_raster.cpp): the vertex transform
// and snap, the triangle setup with its rejects, the edge functions and the depth plane.  Both translation units are
// built with -ffp-contract=off and correctly rounded divides; every product and sum below is rounded on its own, in
// the order written.  What the two sides do NOT share is how they walk the pixels: the host evaluates every edge
// function at every sample of the box directly, the device steps them — equal integers either way.
// Behind ORBIT_RASTER_WIDE_GUARD (R4w-R7w, at the end of this file) the same expressions stand a second time on int64
// coordinates, 128-bit edge values and a double depth plane, with the rectangle test both sides use to skip tiles.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIP__
#define ORBIT_RASTER_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define ORBIT_RASTER_FN inline
#endif

namespace orbit {
namespace raster {

constexpr uint32_t kClipFail = 1u, kGuardFail = 2u; // Vertex::flags
constexpr uint32_t kOutOfBand = 4u; // R4w only, beside kGuardFail: not even below 2^60 (or NaN)

struct Vertex { // R3, R4: one transformed vertex
    int32_t X, Y;   // 8 sub-pixel bits; 0 when the guard failed (R4w: then the float bits of xs * 256, ys * 256)
    float d;        // z / w
    uint32_t flags; // kClipFail | kGuardFail | kOutOfBand
};

ORBIT_RASTER_FN int32_t float_bits(float f) {
    int32_t b;
    __builtin_memcpy(&b, &f, 4);
    return b;
}
ORBIT_RASTER_FN float bits_float(int32_t b) {
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}

// R2: out = a x b, column by column (OpMatrixTimesMatrix: mat4_mul_col of orbit_device.h, canonical profile)
ORBIT_RASTER_FN void mat4_mul(const float *a, const float *b, float *out) {
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++)
            out[4 * c + r] = ((a[r] * b[4 * c] + a[4 + r] * b[4 * c + 1]) + a[8 + r] * b[4 * c + 2]) + a[12 + r] * b[4 * c + 3];
}

struct Clip { // R2: the clip coordinates of one position
    float x, y, z, w;
};

// R2 of one position
ORBIT_RASTER_FN Clip clip_position(const float *mvp, float px, float py, float pz) {
    float clip[4];
    for (int r = 0; r < 4; r++) clip[r] = ((mvp[r] * px + mvp[4 + r] * py) + mvp[8 + r] * pz) + mvp[12 + r] * 1.0f;
    Clip c;
    c.x = clip[0], c.y = clip[1], c.z = clip[2], c.w = clip[3];
    return c;
}

// R3: w > 0 && z >= 0 && z <= w (false for NaN)
ORBIT_RASTER_FN bool clip_in(const Clip &c) { return c.w > 0.0f && c.z >= 0.0f && c.z <= c.w; }

// R3, R4 of clip coordinates.  on_near_plane (R3c's new vertices): the depth is 1 exactly, c.z is not read and R3 is
// not asked; X, Y and the guard flag are R4's all the same.  wide (R4w): a vertex that fails the guard keeps xf, yf as
// float bits in X, Y (both, so that wide_coord() reads either alike) and is kOutOfBand unless both are below 2^60.
ORBIT_RASTER_FN Vertex vertex_from_clip(const Clip &c, float w_f, float h_f, bool on_near_plane = false, bool wide = false) {
    const float x = c.x, y = c.y, z = c.z, w = c.w;
    Vertex v;
    v.flags = on_near_plane ? 0u : (w > 0.0f && z >= 0.0f && z <= w) ? 0u : kClipFail;
    const float nx = x / w, ny = y / w;
    v.d = on_near_plane ? 1.0f : z / w;
    const float xs = (nx * 0.5f + 0.5f) * w_f, ys = (ny * -0.5f + 0.5f) * h_f;
    const float xf = xs * 256.0f, yf = ys * 256.0f;
    const bool in_guard = fabsf(xf) < 8388608.0f && fabsf(yf) < 8388608.0f; // false for NaN
    if (!in_guard) v.flags |= kGuardFail;
    v.X = in_guard ? (int32_t)rintf(xf) : 0;
    v.Y = in_guard ? (int32_t)rintf(yf) : 0;
    if (wide && !in_guard) {
        const bool in_band = fabsf(xf) < 1152921504606846976.0f && fabsf(yf) < 1152921504606846976.0f; // 2^60; false for NaN
        if (!in_band) v.flags |= kOutOfBand;
        v.X = float_bits(xf), v.Y = float_bits(yf);
    }
    return v;
}

// R2-R4 of one position
ORBIT_RASTER_FN Vertex transform_vertex(const float *mvp, float px, float py, float pz, float w_f, float h_f, bool wide = false) {
    return vertex_from_clip(clip_position(mvp, px, py, pz), w_f, h_f, false, wide);
}

enum Outcome : uint32_t { kDraw = 0, kClipSkipped = 1, kGuardSkipped = 2, kBackFacing = 3, kNoCoverage = 4 };

struct Setup { // R5-R7: a triangle that may cover samples, orientation normalised to A > 0
    int32_t ax[3], ay[3], dx[3], dy[3]; // edge k runs from (ax, ay) by (dx, dy): v0->v1, v1->v2, v2->v0
    int32_t nb[3];                      // 0 for a top-left edge, else 1: inside <=> E - nb >= 0 on all three
    int32_t x_lo, x_hi, y_lo, y_hi;     // pixels whose centre lies in the snapped box, clamped to the target
    float d0, gx, gy;
};

ORBIT_RASTER_FN int32_t imin(int32_t a, int32_t b) { return a < b ? a : b; }
ORBIT_RASTER_FN int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }

ORBIT_RASTER_FN uint32_t setup_triangle(const Vertex &v0, Vertex v1, Vertex v2, uint32_t width, uint32_t height,
                                        bool cull_none, Setup &s) {
    const uint32_t flags = v0.flags | v1.flags | v2.flags;
    if (flags & kClipFail) return kClipSkipped;
    if (flags & kGuardFail) return kGuardSkipped;
    int64_t area = (int64_t)(v1.X - v0.X) * (int64_t)(v2.Y - v0.Y) - (int64_t)(v2.X - v0.X) * (int64_t)(v1.Y - v0.Y);
    if (area == 0) return kNoCoverage;
    if (area > 0 && !cull_none) return kBackFacing; // front <=> A < 0
    if (area < 0) {
        const Vertex t = v1;
        v1 = v2, v2 = t;
        area = -area;
    }
    const int32_t min_x = imin(v0.X, imin(v1.X, v2.X)), max_x = imax(v0.X, imax(v1.X, v2.X));
    const int32_t min_y = imin(v0.Y, imin(v1.Y, v2.Y)), max_y = imax(v0.Y, imax(v1.Y, v2.Y));
    // centre 256 x + 128 in [min, max]  <=>  x in [ceil((min - 128) / 256), floor((max - 128) / 256)] (>> floors)
    s.x_lo = imax((min_x - 128 + 255) >> 8, 0), s.x_hi = imin((max_x - 128) >> 8, (int32_t)width - 1);
    s.y_lo = imax((min_y - 128 + 255) >> 8, 0), s.y_hi = imin((max_y - 128) >> 8, (int32_t)height - 1);
    if (s.x_lo > s.x_hi || s.y_lo > s.y_hi) return kNoCoverage;
    s.ax[0] = v0.X, s.ax[1] = v1.X, s.ax[2] = v2.X;
    s.ay[0] = v0.Y, s.ay[1] = v1.Y, s.ay[2] = v2.Y;
    for (int k = 0; k < 3; k++) {
        const int n = k == 2 ? 0 : k + 1;
        s.dx[k] = s.ax[n] - s.ax[k], s.dy[k] = s.ay[n] - s.ay[k];
        s.nb[k] = (s.dy[k] < 0 || (s.dy[k] == 0 && s.dx[k] > 0)) ? 0 : 1;
    }
    const float area_f = (float)(double)area;
    const float d10 = v1.d - v0.d, d20 = v2.d - v0.d;
    s.d0 = v0.d;
    s.gx = (d10 * (float)(v2.Y - v0.Y) - d20 * (float)(v1.Y - v0.Y)) / area_f;
    s.gy = (d20 * (float)(v1.X - v0.X) - d10 * (float)(v2.X - v0.X)) / area_f;
    return kDraw;
}

// R6: edge k at the sample (px, py), less its top-left bias: the sample is inside iff all three are >= 0
ORBIT_RASTER_FN int64_t edge_at(const Setup &s, int k, int32_t px, int32_t py) {
    return (int64_t)s.dx[k] * (int64_t)(py - s.ay[k]) - (int64_t)s.dy[k] * (int64_t)(px - s.ax[k]) - (int64_t)s.nb[k];
}

// R7 at the sample (px, py); the caller writes it iff the result is > 0
ORBIT_RASTER_FN float depth_at(const Setup &s, int32_t px, int32_t py) {
    const float d = (s.d0 + s.gx * (float)(px - s.ax[0])) + s.gy * (float)(py - s.ay[0]);
    return 1.0f < d ? 1.0f : d; // GLSL min(d, 1): a NaN stays a NaN
}

// ---- R3c (ORBIT_RASTER_CLIP_NEAR): a triangle R3 rejects, cut at the near plane z = w -----------------------------
// The pieces as a fan of up to four vertices: piece 0 = (u[0], u[1], u[2]), piece 1 = (u[0], u[2], u[3]).  Both keep
// the triangle's orientation; the diagonal u[0]-u[2] is shared with identical snapped ends.
struct Pieces {
    Vertex u[4];
    uint32_t count; // 0: the triangle stays clip_skipped
};

ORBIT_RASTER_FN Clip select_clip(bool first, const Clip &a, const Clip &b) {
    Clip c;
    c.x = first ? a.x : b.x, c.y = first ? a.y : b.y, c.z = first ? a.z : b.z, c.w = first ? a.w : b.w;
    return c;
}

ORBIT_RASTER_FN bool clip_finite(const Clip &c) {
    return fabsf(c.x) < INFINITY && fabsf(c.y) < INFINITY && fabsf(c.z) < INFINITY && fabsf(c.w) < INFINITY; // false for NaN
}

// N(i, o): the new vertex on the edge from the in vertex i to the out vertex o — a function of the ordered pair
// only, so two triangles sharing the edge get the same vertex.  -> false: the whole triangle is clip_skipped.
ORBIT_RASTER_FN bool clip_new_vertex(const Clip &i, const Clip &o, float w_f, float h_f, Vertex &n, bool wide = false) {
    const float b_i = i.w - i.z, b_o = o.w - o.z;
    const float den = b_i - b_o;
    if (!(den > 0.0f)) return false;
    const float t = b_i / den;
    Clip c; // on the near plane; its z is not computed
    c.x = i.x + t * (o.x - i.x), c.y = i.y + t * (o.y - i.y), c.z = 0.0f, c.w = i.w + t * (o.w - i.w);
    if (!(c.w > 0.0f)) return false;
    n = vertex_from_clip(c, w_f, h_f, true, wide);
    return true;
}

// The pieces of a triangle with at least one vertex failing R3.  The rotation to (a, b, c), a the lone vertex, is
// made of selects: no indexed array.  wide: the pieces' vertices are R4w's.
ORBIT_RASTER_FN void clip_near_pieces(const Clip &c0, const Clip &c1, const Clip &c2, float w_f, float h_f, Pieces &p,
                                      bool wide = false) {
    p.count = 0u;
    const bool in0 = clip_in(c0), in1 = clip_in(c1), in2 = clip_in(c2);
    const uint32_t n_in = (in0 ? 1u : 0u) + (in1 ? 1u : 0u) + (in2 ? 1u : 0u);
    if (n_in == 0u || n_in == 3u) return;
    if (!(clip_finite(c0) && clip_finite(c1) && clip_finite(c2))) return;
    if (!(c0.z >= 0.0f && c1.z >= 0.0f && c2.z >= 0.0f)) return;
    const bool one_in = n_in == 1u;
    // the lone vertex is the one whose test differs from the other two
    const bool lone0 = in0 == one_in, lone1 = !lone0 && in1 == one_in;
    const Clip a = select_clip(lone0, c0, select_clip(lone1, c1, c2));
    const Clip b = select_clip(lone0, c1, select_clip(lone1, c2, c0));
    const Clip c = select_clip(lone0, c2, select_clip(lone1, c0, c1));
    // one in: N(a, b), N(a, c); one out: Q = N(c, a), P = N(b, a)
    Vertex n0, n1;
    if (!clip_new_vertex(select_clip(one_in, a, c), select_clip(one_in, b, a), w_f, h_f, n0, wide)) return;
    if (!clip_new_vertex(select_clip(one_in, a, b), select_clip(one_in, c, a), w_f, h_f, n1, wide)) return;
    if (one_in) { // (a, N(a,b), N(a,c))
        p.u[0] = vertex_from_clip(a, w_f, h_f, false, wide), p.u[1] = n0, p.u[2] = n1, p.u[3] = n1;
        p.count = 1u;
    } else { // (b, c, Q), (b, Q, P)
        p.u[0] = vertex_from_clip(b, w_f, h_f, false, wide), p.u[1] = vertex_from_clip(c, w_f, h_f, false, wide), p.u[2] = n0, p.u[3] = n1;
        p.count = 2u;
    }
}

// piece q of p
ORBIT_RASTER_FN void piece_vertices(const Pieces &p, uint32_t q, Vertex &v0, Vertex &v1, Vertex &v2) {
    v0 = p.u[0];
    v1 = q ? p.u[2] : p.u[1];
    v2 = q ? p.u[3] : p.u[2];
}

// A clipped triangle is counted once, under the best outcome of its pieces: drawn, guard_skipped, back_facing,
// no_coverage — the order of the Outcome values.
ORBIT_RASTER_FN uint32_t better_outcome(uint32_t a, uint32_t b) { return a < b ? a : b; }

// ---- R4w-R7w (ORBIT_RASTER_WIDE_GUARD): a triangle with a vertex outside R4's band and none out of band -----------
// The same expressions as R5-R7 on int64 coordinates, with 128-bit areas and edge values and a double depth plane.
// |X|, |Y| < 2^60, so a difference is below 2^61, a product below 2^122 and an area or edge value below 2^123.
typedef __int128 int128_t;

// R4w's integer of a coordinate slot: the int32 of a narrow vertex, or the float a guard-failing one keeps as bits
// (an integer already, as every float of 2^23 or more is; a narrow coordinate beside a wide one rounds as R4 does)
ORBIT_RASTER_FN int64_t wide_coord(const Vertex &v, int32_t slot) {
    return (v.flags & kGuardFail) ? (int64_t)rintf(bits_float(slot)) : (int64_t)slot;
}

// a wide triangle: all three vertices in band, at least one of them wide
ORBIT_RASTER_FN bool is_wide_triangle(const Vertex &v0, const Vertex &v1, const Vertex &v2) {
    const uint32_t flags = v0.flags | v1.flags | v2.flags;
    return (flags & (kClipFail | kGuardFail | kOutOfBand)) == kGuardFail;
}

struct SetupW { // R5w-R7w: Setup on wide integers
    int64_t ax[3], ay[3], dx[3], dy[3];
    int32_t nb[3];
    int32_t x_lo, x_hi, y_lo, y_hi; // clamped to the target: these fit
    double d0, gx, gy;
};

ORBIT_RASTER_FN int64_t lmin(int64_t a, int64_t b) { return a < b ? a : b; }
ORBIT_RASTER_FN int64_t lmax(int64_t a, int64_t b) { return a > b ? a : b; }

// of a wide triangle (is_wide_triangle): kDraw, kBackFacing or kNoCoverage
ORBIT_RASTER_FN uint32_t setup_triangle_wide(const Vertex &v0, const Vertex &v1, const Vertex &v2, uint32_t width,
                                             uint32_t height, bool cull_none, SetupW &s) {
    const int64_t X0 = wide_coord(v0, v0.X), Y0 = wide_coord(v0, v0.Y);
    int64_t X1 = wide_coord(v1, v1.X), Y1 = wide_coord(v1, v1.Y), X2 = wide_coord(v2, v2.X), Y2 = wide_coord(v2, v2.Y);
    float d1 = v1.d, d2 = v2.d;
    int128_t area = (int128_t)(X1 - X0) * (int128_t)(Y2 - Y0) - (int128_t)(X2 - X0) * (int128_t)(Y1 - Y0);
    if (area == 0) return kNoCoverage;
    if (area > 0 && !cull_none) return kBackFacing;
    if (area < 0) {
        int64_t t = X1;
        X1 = X2, X2 = t;
        t = Y1, Y1 = Y2, Y2 = t;
        const float f = d1;
        d1 = d2, d2 = f;
        area = -area;
    }
    const int64_t min_x = lmin(X0, lmin(X1, X2)), max_x = lmax(X0, lmax(X1, X2));
    const int64_t min_y = lmin(Y0, lmin(Y1, Y2)), max_y = lmax(Y0, lmax(Y1, Y2));
    const int64_t x_lo = lmax((min_x - 128 + 255) >> 8, 0), x_hi = lmin((max_x - 128) >> 8, (int64_t)width - 1);
    const int64_t y_lo = lmax((min_y - 128 + 255) >> 8, 0), y_hi = lmin((max_y - 128) >> 8, (int64_t)height - 1);
    if (x_lo > x_hi || y_lo > y_hi) return kNoCoverage;
    s.x_lo = (int32_t)x_lo, s.x_hi = (int32_t)x_hi, s.y_lo = (int32_t)y_lo, s.y_hi = (int32_t)y_hi;
    s.ax[0] = X0, s.ax[1] = X1, s.ax[2] = X2;
    s.ay[0] = Y0, s.ay[1] = Y1, s.ay[2] = Y2;
    for (int k = 0; k < 3; k++) {
        const int n = k == 2 ? 0 : k + 1;
        s.dx[k] = s.ax[n] - s.ax[k], s.dy[k] = s.ay[n] - s.ay[k];
        s.nb[k] = (s.dy[k] < 0 || (s.dy[k] == 0 && s.dx[k] > 0)) ? 0 : 1;
    }
    // (no int128 -> double conversion on the device: the two halves, each exact, then one rounded sum)
    const double area_d = (double)(int64_t)(area >> 64) * 18446744073709551616.0 + (double)(uint64_t)area;
    const double d10 = (double)d1 - (double)v0.d, d20 = (double)d2 - (double)v0.d;
    s.d0 = (double)v0.d;
    s.gx = (d10 * (double)(Y2 - Y0) - d20 * (double)(Y1 - Y0)) / area_d;
    s.gy = (d20 * (double)(X1 - X0) - d10 * (double)(X2 - X0)) / area_d;
    return kDraw;
}

// R6w: edge_at on wide integers
ORBIT_RASTER_FN int128_t edge_at_wide(const SetupW &s, int k, int32_t px, int32_t py) {
    return (int128_t)s.dx[k] * (int128_t)((int64_t)py - s.ay[k]) - (int128_t)s.dy[k] * (int128_t)((int64_t)px - s.ax[k]) -
           (int128_t)s.nb[k];
}

// R6w: the sample (256 x + 128, 256 y + 128) is inside
ORBIT_RASTER_FN bool inside_wide(const SetupW &s, int32_t x, int32_t y) {
    const int32_t px = 256 * x + 128, py = 256 * y + 128;
    return edge_at_wide(s, 0, px, py) >= 0 && edge_at_wide(s, 1, px, py) >= 0 && edge_at_wide(s, 2, px, py) >= 0;
}

// No sample of the pixels [x0, x1] x [y0, y1] is inside: an edge function is affine, so over the rectangle it is largest
// at the corner its gradient (-dy, dx) points to; negative there (after the bias), it is negative at every sample.
// Exact in this direction; `false` promises nothing (the three half planes may still miss each other inside).
ORBIT_RASTER_FN bool rect_outside_wide(const SetupW &s, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
    bool out = false;
    for (int k = 0; k < 3; k++) {
        const int32_t x = s.dy[k] > 0 ? x0 : x1, y = s.dx[k] > 0 ? y1 : y0;
        out = out || edge_at_wide(s, k, 256 * x + 128, 256 * y + 128) < 0;
    }
    return out;
}

// R7w at the sample (px, py); the caller writes it iff the result is > 0
ORBIT_RASTER_FN float depth_at(const SetupW &s, int32_t px, int32_t py) {
    const double dd = (s.d0 + s.gx * (double)((int64_t)px - s.ax[0])) + s.gy * (double)((int64_t)py - s.ay[0]);
    const float d = (float)dd;
    return 1.0f < d ? 1.0f : d;
}

} // namespace raster
} // namespace orbit
