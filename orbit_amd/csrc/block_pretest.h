// block_pretest.h — the per-block pre-test of the pass-0 evaluation (meshlet_eval_blocks.hip): the bound of a block of
// 32 meshlets (meshlet_stream.hip derives it), what a dispatch record precomputes from it, and the per-meshlet test that
// decides the cone verdict (shaders/meshlet_cull.comp:148-158 of the reference repo) from the 4-byte cone word alone
// wherever that verdict is certain.  Compiles for the device and for the host (liborbit_host exports it:
// tests/test_block_pretest_cpu.py holds it against the oracle).  The pre-test is NOT the reference's arithmetic — it only
// has to be right about "certain" — so it uses fma freely; every fma is written out (the units are built with
// -ffp-contract=off), which makes the host and the device compute the same bits.
//
// The bound (DESIGN.md 4.2 has the derivation).  u = 2^-24.  With p = M (c, 1) the meshlet's view-space centre, L = mat3(M),
// a_f / cutoff_f the decoded cone and rs = radius x scale, the reference culls iff fl(p . L a_f) >= fl(cutoff_f |p| + rs).
// For a block with |c - C| <= Rc and radius <= r_max:  p = d + e, d = M (C, 1), |e| <= sigma Rc, sigma >= ||L||_2, so the exact
//     E = p . L a_f - cutoff_f |p| - rs   lies in   [S0 - W - r', S0 + W],
//     S0 = g . a_f - cutoff_f D,  g = L^T d,  D = |d|,  W = sigma Rc (sigma |a_f| + |cutoff_f|),  r' = r_max x scale.
// Rounding: the reference's two sides are off their exact values by at most 20 u (Ap + D + Rc') (sigma |a_f|_1 + |cutoff_f|)
// + 2.1 u r' + 2^-149 (Ap: the largest sum of absolute terms of a component of p), the pre-test's own S0 by at most
// 10 u D (sigma |a_f|_1 + |cutoff_f|), and d itself by 7 u Ap.  All of it is covered by kBlkEps = 64 u on the magnitudes,
// a factor 1 + 2^-10 on the band, and kBlkTiny for underflow.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ORBIT_BLK_FN __host__ __device__ inline
#else
#define ORBIT_BLK_FN inline
#endif

namespace orbit {

ORBIT_BLK_FN uint32_t blk_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
ORBIT_BLK_FN float blk_float(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
// a finite x >= 0 rounded up to a float whose lower 16 bits are zero, as those upper 16 bits
ORBIT_BLK_FN uint32_t blk_up16(float x) { return (blk_bits(x) + 0xFFFFu) >> 16; }

// One entry per 32-aligned block of global meshlet indices (addressed like MeshletStreamView::base32).
struct BlockBound {
    float cx, cy, cz; // model-space centre C
    // what the evaluation reads besides the centre, so that a record's bound is ONE 16-byte load into four registers:
    // rc and r_max rounded UP to their upper 16 bits, rc in the upper half; 0 = not valid (a valid rc is never 0)
    uint32_t packed;
    float rc;         // |c_i - C| <= rc for every meshlet of the block that the stream's arrays hold
    float r_max;      // radius_i <= r_max
    uint32_t valid;   // 0: some centre or radius is not finite, a radius is negative, or the block was never derived
    uint32_t pad_;
};
static_assert(sizeof(BlockBound) == 32, "BlockBound layout");

// the bound as the evaluation sees it: {centre, packed} -> rc, r_max (each at most 2^-7 above the entry's), valid
ORBIT_BLK_FN BlockBound block_bound_unpack(float cx, float cy, float cz, uint32_t packed) {
    BlockBound b;
    b.cx = cx, b.cy = cy, b.cz = cz, b.packed = packed;
    b.rc = blk_float(packed & 0xFFFF0000u);
    b.r_max = blk_float(packed << 16);
    b.valid = (packed >> 16) != 0u ? 1u : 0u;
    b.pad_ = 0u;
    return b;
}

// What the rows read of a sparse record (wave tile slab): everything in units of 127 (the cone's integer bytes are used
// as they are: a_f = a_i k_f (1 + <= u), k_f the reference's rounded 1 / 127).
struct BlockRecord {
    float gx, gy, gz, dk; // k_f g, k_f D
    float sigma;          // >= ||L||_2
    float bk;             // k_f (Rc' + kBlkEps (Ap + D + Rc')) (1 + 2^-10)
    float rr;             // r' (1 + 2^-10) + kBlkTiny
    uint32_t flags;       // kBlkSparse | kBlkInside
};
static_assert(sizeof(BlockRecord) == 32, "BlockRecord layout");
constexpr uint32_t kBlkSparse = 1u; // the record's lanes take the pre-test
constexpr uint32_t kBlkInside = 2u; // every meshlet of the block is certainly inside every cull plane

constexpr float kBlkEps = 0x1p-18f;    // 64 u
constexpr float kBlkSlack = 1.0f + 0x1p-10f;
constexpr float kBlkUp = 1.0f + 0x1p-20f; // rounds a correctly rounded result up past its exact value
constexpr float kBlkTiny = 0x1p-80f;
constexpr float kBlkHuge = 0x1p60f;    // magnitudes beyond it (sigma: beyond 2^40): the record stays dense.  Below, nothing
                                       // overflows, and what underflows (2^-149 per operation, times these) stays below kBlkTiny
// A record is sparse only if the block is small against its distance from the camera, D > ORBIT_BLK_RATIO Rc': the share of
// lanes whose verdict stays open is about Rc' / D times a small factor, and an open lane costs a gathered literal evaluation.
#ifndef ORBIT_BLK_RATIO
#define ORBIT_BLK_RATIO 8.0f
#endif

ORBIT_BLK_FN float blk_max(float a, float b) { return a > b ? a : b; }

// The bound of n <= 32 spheres {x, y, z, radius} around a given centre (the derivation picks the middle of their box).
// Distances are rounded up by kBlkUp (the float distance is within 4 u of the exact one) plus 2^-60 for squares that
// underflow; r_max is an exact maximum.
ORBIT_BLK_FN BlockBound block_bound_finish(float cx, float cy, float cz, float dist_max, float r_max, float r_min, bool finite) {
    BlockBound b;
    b.cx = cx, b.cy = cy, b.cz = cz;
    b.rc = dist_max * kBlkUp + 0x1p-60f;
    b.r_max = r_max;
    const bool ok = finite && r_min >= 0.0f && b.rc < kBlkHuge && r_max < kBlkHuge && fabsf(cx) < kBlkHuge &&
                    fabsf(cy) < kBlkHuge && fabsf(cz) < kBlkHuge;
    b.valid = ok ? 1u : 0u;
    b.packed = ok ? (blk_up16(b.rc) << 16 | blk_up16(r_max)) : 0u;
    b.pad_ = 0u;
    return b;
}
ORBIT_BLK_FN float block_dist(float cx, float cy, float cz, float x, float y, float z) {
    const float dx = x - cx, dy = y - cy, dz = z - cz;
    return sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}

// The bound of n <= 32 spheres {x, y, z, radius}, as the derivation launch computes it (meshlet_stream.hip: the same
// operations, there across the lanes of half a wave).
ORBIT_BLK_FN BlockBound block_bound_of(const float *spheres, uint32_t n) {
    const float inf = INFINITY;
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf}, r_max = 0.0f, r_min = 0.0f;
    bool finite = true;
    for (uint32_t i = 0; i < n; i++) {
        const float *s = spheres + 4 * i;
        for (int k = 0; k < 3; k++) lo[k] = fminf(lo[k], s[k]), hi[k] = fmaxf(hi[k], s[k]);
        r_max = fmaxf(r_max, s[3]), r_min = fminf(r_min, s[3]);
        finite = finite && isfinite(s[0]) && isfinite(s[1]) && isfinite(s[2]) && isfinite(s[3]);
    }
    const float cx = 0.5f * lo[0] + 0.5f * hi[0], cy = 0.5f * lo[1] + 0.5f * hi[1], cz = 0.5f * lo[2] + 0.5f * hi[2];
    float dist = 0.0f;
    for (uint32_t i = 0; i < n; i++) dist = fmaxf(dist, block_dist(cx, cy, cz, spheres[4 * i], spheres[4 * i + 1], spheres[4 * i + 2]));
    return block_bound_finish(cx, cy, cz, dist, r_max, r_min, finite);
}

// What the plane loop below needs of a plane alone, not of the record: |n| rounded up.  The evaluation computes it once
// per workgroup and plane (meshlet_eval_blocks.hip plane_nn), not once per record and plane.
ORBIT_BLK_FN float block_plane_norm(float nx, float ny, float nz) {
    return sqrtf(fmaf(nz, nz, fmaf(ny, ny, nx * nx))) * kBlkUp + kBlkTiny;
}

// A record's precomputation.  m = view x model, column-major (m[4 c + r]); affine: its last row is 0 0 0 1 and its
// translation finite (WaveTileLds::affine_rows); scale: the slab's largest column norm; planes: n_planes x {nx, ny, nz, w};
// covered: the record starts on a multiple of 32 and the stream holds all its meshlets; ratio: the record is sparse only
// if D > ratio Rc' (the evaluation's ORBIT_BLK_RATIO — a matter of speed: the bounds hold for any ratio >= 0).
ORBIT_BLK_FN BlockRecord block_record_setup(const float *m, bool affine, float scale, const BlockBound &b, bool covered,
                                            const float *planes, uint32_t n_planes, float ratio = ORBIT_BLK_RATIO) {
    BlockRecord o;
    const float Cx = b.cx, Cy = b.cy, Cz = b.cz;
    // d = M (C, 1) and the largest sum of absolute terms of a component of any p of the block
    const float dx = fmaf(m[8], Cz, fmaf(m[4], Cy, fmaf(m[0], Cx, m[12])));
    const float dy = fmaf(m[9], Cz, fmaf(m[5], Cy, fmaf(m[1], Cx, m[13])));
    const float dz = fmaf(m[10], Cz, fmaf(m[6], Cy, fmaf(m[2], Cx, m[14])));
    const float aCx = fabsf(Cx), aCy = fabsf(Cy), aCz = fabsf(Cz);
    const float apx = fmaf(fabsf(m[8]), aCz, fmaf(fabsf(m[4]), aCy, fmaf(fabsf(m[0]), aCx, fabsf(m[12]))));
    const float apy = fmaf(fabsf(m[9]), aCz, fmaf(fabsf(m[5]), aCy, fmaf(fabsf(m[1]), aCx, fabsf(m[13]))));
    const float apz = fmaf(fabsf(m[10]), aCz, fmaf(fabsf(m[6]), aCy, fmaf(fabsf(m[2]), aCx, fabsf(m[14]))));
    // sigma^2 >= the largest eigenvalue of L^T L (Gershgorin on the Gram matrix: exact for orthogonal columns)
    const float g00 = fmaf(m[2], m[2], fmaf(m[1], m[1], m[0] * m[0]));
    const float g11 = fmaf(m[6], m[6], fmaf(m[5], m[5], m[4] * m[4]));
    const float g22 = fmaf(m[10], m[10], fmaf(m[9], m[9], m[8] * m[8]));
    const float g01 = fabsf(fmaf(m[2], m[6], fmaf(m[1], m[5], m[0] * m[4])));
    const float g02 = fabsf(fmaf(m[2], m[10], fmaf(m[1], m[9], m[0] * m[8])));
    const float g12 = fabsf(fmaf(m[6], m[10], fmaf(m[5], m[9], m[4] * m[8])));
    const float s2 = blk_max(g00 + g01 + g02, blk_max(g11 + g01 + g12, g22 + g02 + g12));
    // (the Gram entries carry 3 u of their absolute sums, which s2 bounds: 2^-16 covers them and the square root)
    const float sigma = sqrtf(s2) * (1.0f + 0x1p-16f) + 0x1p-60f; // (+ 2^-60: entries whose squares underflow)
    const float ap = (blk_max(apx, blk_max(apy, apz)) + 2.0f * sigma * b.rc) * kBlkUp;
    const float rcp = fmaf(kBlkEps, ap, sigma * b.rc * kBlkUp); // Rc': sigma Rc, plus what d is off by
    const float D = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
    const float gx = fmaf(m[2], dz, fmaf(m[1], dy, m[0] * dx));
    const float gy = fmaf(m[6], dz, fmaf(m[5], dy, m[4] * dx));
    const float gz = fmaf(m[10], dz, fmaf(m[9], dy, m[8] * dx));
    const float kf = 0x1.020408p-7f; // the reference's 1 / 127 (orbit_device.h snorm8)
    const float mag = ap + D + rcp;
    o.gx = gx * kf, o.gy = gy * kf, o.gz = gz * kf, o.dk = D * kf;
    o.sigma = sigma;
    o.bk = kf * fmaf(kBlkEps, mag, rcp) * kBlkSlack;
    o.rr = b.r_max * scale * kBlkSlack + kBlkTiny;
    // every comparison is false for a NaN: a record with a non-finite intermediate stays dense
    bool sparse = affine && covered && b.valid != 0u && D > ratio * rcp && D > 0x1p-40f && mag < kBlkHuge &&
                  sigma < 0x1p40f && o.rr < kBlkHuge && scale >= 0.0f;
    bool inside = sparse;
    for (uint32_t i = 0; i < n_planes; i++) {
        const float nx = planes[4 * i], ny = planes[4 * i + 1], nz = planes[4 * i + 2], w = planes[4 * i + 3];
        const float nn = block_plane_norm(nx, ny, nz);
        const float dist = fmaf(nz, dz, fmaf(ny, dy, fmaf(nx, dx, w))) - nn * rcp;
        const float margin = fmaf(kBlkEps, fmaf(nn, mag, fabsf(w)), kBlkTiny);
        inside = inside && dist > margin; // then fl(n . p + w) > 0 >= -radius x scale for every meshlet of the block
    }
    o.flags = (sparse ? kBlkSparse : 0u) | (inside ? kBlkInside : 0u);
    return o;
}

// The same precomputation on FOUR lanes per record (the evaluation's blk_setup: lane k = lane & 3 of record lane >> 2).
// Every value that reaches the BlockRecord is computed by the expression tree block_record_setup computes it by — the
// same operations on the same operands in the same order — only by another lane, so the two forms agree in every bit
// (tests/test_block_setup_quad_cpu.py) and no bound above needs deriving again: nothing is summed across lanes.
//   lane k reads row k of m and two of its columns, A = column {0, 1, 2, 0}[k] and B = column {1, 2, 2, 2}[k], and
//   computes d_k and ap_k (k < 3), the Gram diagonal of A (k < 3: g00, g11, g22) and |A . B| (k = 0, 1, 3: g01, g12, g02);
//   the quad exchanges these twelve (BlockQuadSums); every lane runs the scalar tail (BlockQuadTail), lane k < 3 adds
//   component k of g = L^T d from its column A, lane 3 has D; plane i goes to lane i & 3, and the record is inside if
//   every lane's planes say so.
ORBIT_BLK_FN int block_quad_col_a(int k) { return k == 3 ? 0 : k; }
ORBIT_BLK_FN int block_quad_col_b(int k) { return k < 2 ? k + 1 : 2; }
struct BlockQuadShare {
    float d, ap, gd, go;
};
ORBIT_BLK_FN BlockQuadShare block_quad_share(const float row[4], const float a[3], const float b[3], float Cx, float Cy, float Cz) {
    BlockQuadShare s;
    s.d = fmaf(row[2], Cz, fmaf(row[1], Cy, fmaf(row[0], Cx, row[3])));
    s.ap = fmaf(fabsf(row[2]), fabsf(Cz), fmaf(fabsf(row[1]), fabsf(Cy), fmaf(fabsf(row[0]), fabsf(Cx), fabsf(row[3]))));
    s.gd = fmaf(a[2], a[2], fmaf(a[1], a[1], a[0] * a[0]));
    s.go = fabsf(fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])));
    return s;
}
struct BlockQuadSums { // lane:
    float dx, dy, dz;     // d of 0, 1, 2
    float apx, apy, apz;  // ap of 0, 1, 2
    float g00, g11, g22;  // gd of 0, 1, 2
    float g01, g12, g02;  // go of 0, 1, 3
};
struct BlockQuadTail {
    float sigma, rcp, D, mag, bk, rr;
    bool sparse;
};
constexpr float kBlkKf = 0x1.020408p-7f; // the reference's 1 / 127 (orbit_device.h snorm8)
ORBIT_BLK_FN BlockQuadTail block_quad_tail(const BlockQuadSums &q, bool affine, float scale, const BlockBound &b, bool covered,
                                           float ratio) {
    BlockQuadTail t;
    const float s2 = blk_max(q.g00 + q.g01 + q.g02, blk_max(q.g11 + q.g01 + q.g12, q.g22 + q.g02 + q.g12));
    t.sigma = sqrtf(s2) * (1.0f + 0x1p-16f) + 0x1p-60f;
    const float ap = (blk_max(q.apx, blk_max(q.apy, q.apz)) + 2.0f * t.sigma * b.rc) * kBlkUp;
    t.rcp = fmaf(kBlkEps, ap, t.sigma * b.rc * kBlkUp);
    t.D = sqrtf(fmaf(q.dz, q.dz, fmaf(q.dy, q.dy, q.dx * q.dx)));
    t.mag = ap + t.D + t.rcp;
    t.bk = kBlkKf * fmaf(kBlkEps, t.mag, t.rcp) * kBlkSlack;
    t.rr = b.r_max * scale * kBlkSlack + kBlkTiny;
    t.sparse = affine && covered && b.valid != 0u && t.D > ratio * t.rcp && t.D > 0x1p-40f && t.mag < kBlkHuge &&
               t.sigma < 0x1p40f && t.rr < kBlkHuge && scale >= 0.0f;
    return t;
}
// lane k < 3: k_f g_k from its column A (column k); lane 3: k_f D — the record's first four floats, one per lane
ORBIT_BLK_FN float block_quad_out(int k, const float a[3], const BlockQuadSums &q, const BlockQuadTail &t) {
    const float g = fmaf(a[2], q.dz, fmaf(a[1], q.dy, a[0] * q.dx));
    return (k == 3 ? t.D : g) * kBlkKf;
}
// one plane {nx, ny, nz, w} with nn = block_plane_norm(nx, ny, nz): the block is certainly inside it
ORBIT_BLK_FN bool block_quad_plane(const float pl[4], float nn, const BlockQuadSums &q, const BlockQuadTail &t) {
    const float dist = fmaf(pl[2], q.dz, fmaf(pl[1], q.dy, fmaf(pl[0], q.dx, pl[3]))) - nn * t.rcp;
    const float margin = fmaf(kBlkEps, fmaf(nn, t.mag, fabsf(pl[3])), kBlkTiny);
    return dist > margin;
}
// The quad form with arrays of four where the device has four lanes and an exchange (plane_nn[i]: block_plane_norm of
// plane i, as the evaluation's workgroup holds it).
ORBIT_BLK_FN BlockRecord block_record_setup_quad(const float *m, bool affine, float scale, const BlockBound &b, bool covered,
                                                 const float *planes, const float *plane_nn, uint32_t n_planes,
                                                 float ratio = ORBIT_BLK_RATIO) {
    BlockQuadShare s[4];
    for (int k = 0; k < 4; k++) {
        const float row[4] = {m[k], m[4 + k], m[8 + k], m[12 + k]};
        s[k] = block_quad_share(row, m + 4 * block_quad_col_a(k), m + 4 * block_quad_col_b(k), b.cx, b.cy, b.cz);
    }
    const BlockQuadSums q = {s[0].d,  s[1].d,  s[2].d,  s[0].ap, s[1].ap, s[2].ap,
                             s[0].gd, s[1].gd, s[2].gd, s[0].go, s[1].go, s[3].go};
    float out[4];
    BlockQuadTail t[4];
    bool pass = true;
    for (int k = 0; k < 4; k++) {
        t[k] = block_quad_tail(q, affine, scale, b, covered, ratio);
        out[k] = block_quad_out(k, m + 4 * block_quad_col_a(k), q, t[k]);
        for (uint32_t i = (uint32_t)k; i < n_planes; i += 4u) pass = block_quad_plane(planes + 4 * i, plane_nn[i], q, t[k]) && pass;
    }
    BlockRecord o;
    o.gx = out[0], o.gy = out[1], o.gz = out[2], o.dk = out[3];
    o.sigma = t[0].sigma, o.bk = t[0].bk, o.rr = t[0].rr;
    o.flags = (t[0].sparse ? kBlkSparse : 0u) | (t[0].sparse && pass ? kBlkInside : 0u);
    return o;
}

// The per-meshlet pre-test from the cone word (cone_axis bytes | cone_cutoff << 24): s0 and the half-width of the band
// around zero inside which the verdict stays open.
ORBIT_BLK_FN void block_pretest_terms(const BlockRecord &r, uint32_t cone, float &s0, float &band) {
    const float ax = (float)(int)(int8_t)(cone & 0xFFu), ay = (float)(int)(int8_t)((cone >> 8) & 0xFFu);
    const float az = (float)(int)(int8_t)((cone >> 16) & 0xFFu), co = (float)(int)(int8_t)(cone >> 24);
    s0 = fmaf(r.gx, ax, fmaf(r.gy, ay, fmaf(r.gz, az, -(co * r.dk))));
    const float a1 = fabsf(ax) + fabsf(ay) + fabsf(az);
    band = fmaf(r.bk, fmaf(r.sigma, a1, fabsf(co)), kBlkTiny);
}
// certainly culled by the cone / certainly kept by it; neither: the literal evaluation decides (a NaN fails both)
ORBIT_BLK_FN bool block_cone_culls(const BlockRecord &r, float s0, float band) { return s0 >= band + r.rr; }
ORBIT_BLK_FN bool block_cone_keeps(float s0, float band) { return s0 < -band; }
// 1: certainly culled, 2: certainly kept, 0: open
ORBIT_BLK_FN uint32_t block_pretest(const BlockRecord &r, uint32_t cone) {
    float s0, band;
    block_pretest_terms(r, cone, s0, band);
    return block_cone_culls(r, s0, band) ? 1u : (block_cone_keeps(s0, band) ? 2u : 0u);
}

} // namespace orbit
