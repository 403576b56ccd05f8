// post_common.h — the arithmetic of orbit_bloom and orbit_post_process (include/orbit_abi_ext.h B1-B9 and T1-T5,
// DESIGN.md §4.27), written once for the device kernels (bloom.hip) and the host mirror (orbit_amd/host/orbit_post.cpp).
// The pieces: post_exp2c / post_powc are B5's and T4's power; bloom_pack / bloom_unpack are B7's storage; bloom_axis is
// B3's coordinate of one axis and bloom_sample its four-texel expression over a `fetch(ix, iy, rgb)` the caller hands in
// (global memory, an LDS tile or a host array: the same floats, so the same bytes); bloom_down_texel is B4 / B5 and
// bloom_up_texel B6 of one destination texel; bloom_down_span / bloom_up_span bound the source indices a run of
// destination texels can touch; post_pixel is T1-T5 of one pixel.  fp32, every operation rounded on its own.
#pragma once
#include "shade_common.h" // shade_log2c, shade_max / min / clamp, finite_or_zero, float_bits / bits_float

namespace orbit {
namespace raster {

constexpr uint32_t kBloomMaxLevels = 6u; // bloom.rs:9

// Between two taps of a stencil on the device: the scheduler keeps one tap's loads from rising above the tap before it
// (left alone it lifts all 13 taps' 156 floats to the top: 212 VGPRs, two waves per SIMD).  No effect on any value.
#ifdef __HIP_DEVICE_COMPILE__
#define ORBIT_POST_TAP_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define ORBIT_POST_TAP_FENCE() ((void)0)
#endif

// 2^x of the same kind as shade_log2c: k = floor(x + 0.5), r = x - k in [-0.5, 0.5], the degree-7 Taylor polynomial of
// 2^r by Horner (its remainder is below 5.2e-9 there), times 2^k built from its bits.  x >= 128 -> +inf, x < -126 -> 0
// (no denormal results), NaN -> NaN.  Products and sums only.
ORBIT_RASTER_FN float post_exp2c(float x) {
    if (x != x) return x;
    if (x >= 128.0f) return INFINITY;
    if (x < -126.0f) return 0.0f;
    const float k = floorf(x + 0.5f);
    const float r = x - k;
    const float c[8] = {1.5252734e-5f, 1.5403530e-4f, 1.3333558e-3f, 9.6181291e-3f, 5.5504109e-2f, 2.4022651e-1f, 6.9314718e-1f, 1.0f};
    float p = c[0];
    for (int i = 1; i < 8; i++) {
        p = p * r;
        p = p + c[i];
    }
    int e = (int)k;
    if (e > 127) { // x in [127.5, 128): 2^127 * 2 * p would overflow the exponent field; p * 2 first
        p = p * 2.0f;
        e = 127;
    }
    return bits_float((int32_t)((uint32_t)(e + 127) << 23)) * p;
}
// pow(x, y) of B5 and T4: x <= 0 (and NaN) -> 0
ORBIT_RASTER_FN float post_powc(float x, float y) {
    if (!(x > 0.0f)) return 0.0f;
    return post_exp2c(y * shade_log2c(x));
}

// ---- B7: B10G11R11_UFLOAT_PACK32.  MANT = 6 (R, G: 11 bits) or 5 (B: 10 bits); 5 exponent bits, bias 15
template <int MANT>
ORBIT_RASTER_FN uint32_t bloom_encode(float x, bool &clamped) {
    constexpr uint32_t kMaxCode = (30u << MANT) | ((1u << MANT) - 1u);
    if (!(fabsf(x) < INFINITY)) return 0u; // B8
    if (!(x > 0.0f)) return 0u;
    const uint32_t b = (uint32_t)float_bits(x);
    const int e = (int)(b >> 23) - 127 + 15;
    if (e >= 31) {
        clamped = true;
        return kMaxCode;
    }
    if (e >= 1) {
        const uint32_t code = ((uint32_t)e << MANT) | ((b & 0x007FFFFFu) >> (23 - MANT));
        if (code == kMaxCode) clamped = true; // x at or above the largest finite value
        return code;
    }
    return (uint32_t)(x * (float)(1u << (14 + MANT))); // below 2^-14: a multiple of the smallest step, truncated
}
template <int MANT>
ORBIT_RASTER_FN float bloom_decode(uint32_t code) {
    const uint32_t e = code >> MANT, m = code & ((1u << MANT) - 1u);
    if (e == 0u) return (float)m * (1.0f / (float)(1u << (14 + MANT)));
    if (e == 31u) return bits_float((int32_t)(0x7F800000u | (m << (23 - MANT)))); // never stored by B8
    return bits_float((int32_t)(((e + 112u) << 23) | (m << (23 - MANT))));
}
ORBIT_RASTER_FN uint32_t bloom_pack(const float *rgb, bool &clamped) {
    return bloom_encode<6>(rgb[0], clamped) | (bloom_encode<6>(rgb[1], clamped) << 11) | (bloom_encode<5>(rgb[2], clamped) << 22);
}
ORBIT_RASTER_FN void bloom_unpack(uint32_t word, float *rgb) {
    rgb[0] = bloom_decode<6>(word & 0x7FFu), rgb[1] = bloom_decode<6>((word >> 11) & 0x7FFu), rgb[2] = bloom_decode<5>(word >> 22);
}

// ---- B1: the chain's shape (orbit_bloom_layout); max_levels 1..6
ORBIT_RASTER_FN void bloom_layout(uint32_t width, uint32_t height, uint32_t max_levels, OrbitBloomLayout &out) {
    const uint32_t m = width > height ? width : height;
    uint32_t levels = 0u;
    for (uint32_t v = m; v != 0u; v >>= 1) levels++; // floor(log2(m)) + 1
    if (levels < 1u) levels = 1u;
    if (levels > kBloomMaxLevels) levels = kBloomMaxLevels;
    if (levels > max_levels) levels = max_levels;
    out.max_levels = max_levels, out.levels = levels, out._pad = 0u;
    uint32_t at = 0u;
    for (uint32_t k = 0; k < kBloomMaxLevels; k++) {
        const bool live = k < levels;
        const uint32_t w = (width >> k) > 1u ? (width >> k) : 1u, h = (height >> k) > 1u ? (height >> k) : 1u;
        out.level_width[k] = live ? w : 0u, out.level_height[k] = live ? h : 0u, out.level_offset[k] = live ? at : 0u;
        if (live) at += w * h;
    }
    out.total_texels = at;
}
// B2 (bloom.rs:106-111), in float, as written
ORBIT_RASTER_FN void bloom_threshold_filter(float threshold, float soft_threshold, float *tf) {
    const float knee = threshold * soft_threshold;
    tf[0] = threshold;
    tf[1] = tf[0] - knee;
    tf[2] = 2.0f * knee;
    tf[3] = 0.25f / (knee + 0.00001f);
}

// ---- B3: one axis of a LinearClamp sample at coordinate u of a level n texels wide
struct BloomAxis {
    uint32_t i0, i1;
    float f;
};
// an integer-valued float (or +-inf) clamped to [0, n - 1]; NaN -> 0
ORBIT_RASTER_FN uint32_t bloom_index(float t, uint32_t n) {
    if (!(t >= 0.0f)) return 0u;
    if (t >= (float)(n - 1u)) return n - 1u;
    return (uint32_t)t;
}
ORBIT_RASTER_FN BloomAxis bloom_axis(float u, uint32_t n) {
    const float s = u * (float)n - 0.5f;
    const float fl = floorf(s);
    BloomAxis a;
    a.f = s - fl;
    a.i0 = bloom_index(fl, n), a.i1 = bloom_index(fl + 1.0f, n);
    return a;
}
template <class Fetch>
ORBIT_RASTER_FN void bloom_sample(const Fetch &fetch, float u, float v, uint32_t src_w, uint32_t src_h, float *out) {
    const BloomAxis ax = bloom_axis(u, src_w), ay = bloom_axis(v, src_h);
    float t00[3], t10[3], t01[3], t11[3];
    fetch(ax.i0, ay.i0, t00), fetch(ax.i1, ay.i0, t10), fetch(ax.i0, ay.i1, t01), fetch(ax.i1, ay.i1, t11);
    const float gx = 1.0f - ax.f, gy = 1.0f - ay.f;
    for (int c = 0; c < 3; c++) out[c] = (t00[c] * gx + t10[c] * ax.f) * gy + (t01[c] * gx + t11[c] * ax.f) * ay.f;
}

// ---- B4: the uv of the downsample's tap d of destination texel i on an axis dst_n texels wide
ORBIT_RASTER_FN float bloom_down_u(uint32_t i, float d, uint32_t dst_n) { return (((float)i + 0.5f) + d) * (1.0f / (float)dst_n); }
// B6: the upsample's
ORBIT_RASTER_FN float bloom_up_u(uint32_t i, float off, uint32_t dst_n) { return (float)i * (1.0f / (float)dst_n) + off; }

// The source indices destination texels [first, last] of one axis can touch.  Every step from (i, d) to an index — the
// exact sum i + 0.5 + d, the rounded product with 1 / dst_n, the rounded product with src_n, the rounded difference with
// 0.5, floorf, + 1 and the clamp — is monotone non-decreasing in i and in d (a correctly rounded operation with one
// operand fixed and non-negative is monotone), so the taps of first at the smallest offset and of last at the largest
// bound every tap between them, rounding included: no margin is needed on top.  For src_n = dst_n the span is 3 texels
// each side (level 0), for src_n = 2 dst_n it is 4 below and 5 above.
ORBIT_RASTER_FN void bloom_down_span(uint32_t first, uint32_t last, uint32_t dst_n, uint32_t src_n, uint32_t &lo, uint32_t &hi) {
    lo = bloom_axis(bloom_down_u(first, -2.0f, dst_n), src_n).i0;
    hi = bloom_axis(bloom_down_u(last, 2.0f, dst_n), src_n).i1;
}
ORBIT_RASTER_FN void bloom_up_span(uint32_t first, uint32_t last, uint32_t dst_n, uint32_t src_n, float r, uint32_t &lo, uint32_t &hi) {
    lo = bloom_axis(bloom_up_u(first, -r, dst_n), src_n).i0;
    hi = bloom_axis(bloom_up_u(last, r, dst_n), src_n).i1;
}

// B5: bloom_downsample.comp:20-35
ORBIT_RASTER_FN float bloom_karis(const float *c) {
    const float kInvGamma = 0.45454547f; // 1.0 / 2.2 as a float
    const float s0 = post_powc(c[0], kInvGamma), s1 = post_powc(c[1], kInvGamma), s2 = post_powc(c[2], kInvGamma);
    const float luma = ((s0 * 0.2126f + s1 * 0.7152f) + s2 * 0.0722f) * 0.25f;
    return 1.0f / (1.0f + luma);
}
ORBIT_RASTER_FN void bloom_prefilter(const float *tf, float *c) {
    const float m = shade_max(c[0], shade_max(c[1], c[2]));
    float soft = shade_clamp(m - tf[1], 0.0f, tf[2]);
    soft = (soft * soft) * tf[3];
    const float contribution = shade_max(m - tf[0], soft) / shade_max(m, 0.00001f);
    for (int i = 0; i < 3; i++) c[i] = c[i] * contribution;
}

// B4 (and B5 when level0) of destination texel (x, y): the 13 taps, the five groups and their sum as the shader has them
template <class Fetch>
ORBIT_RASTER_FN void bloom_down_texel(const Fetch &fetch, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h, uint32_t x,
                                      uint32_t y, bool level0, const float *tf, float *result) {
    // The taps in the shader's order x, y0..y3, z0..z7, each added to its groups as it arrives (x last): the sums are the
    // shader's left-to-right ones and only the centre, the five groups and one tap are alive at a time
    float c[3], t[3], g[5][3];
    const auto tap = [&](float dx, float dy, float *out) {
        bloom_sample(fetch, bloom_down_u(x, dx, dst_w), bloom_down_u(y, dy, dst_h), src_w, src_h, out);
        ORBIT_POST_TAP_FENCE();
    };
    tap(0.0f, 0.0f, c);
    tap(1.0f, 1.0f, g[0]); // y0
    tap(-1.0f, 1.0f, t);   // y1
    for (int i = 0; i < 3; i++) g[0][i] = g[0][i] + t[i];
    tap(1.0f, -1.0f, t); // y2
    for (int i = 0; i < 3; i++) g[0][i] = g[0][i] + t[i];
    tap(-1.0f, -1.0f, t); // y3
    for (int i = 0; i < 3; i++) g[0][i] = (g[0][i] + t[i]) * 0.125f;
    tap(-2.0f, -2.0f, t); // z0
    for (int i = 0; i < 3; i++) g[1][i] = t[i] + t[i]; // :70 as the binary has it: z0 + z0
    tap(-2.0f, 0.0f, g[2]); // z1
    tap(-2.0f, 2.0f, t);    // z2
    for (int i = 0; i < 3; i++) g[2][i] = g[2][i] + t[i];
    tap(0.0f, -2.0f, g[3]); // z3
    for (int i = 0; i < 3; i++) g[1][i] = g[1][i] + g[3][i];
    tap(0.0f, 2.0f, g[4]); // z4
    for (int i = 0; i < 3; i++) g[2][i] = g[2][i] + g[4][i];
    tap(2.0f, -2.0f, t); // z5
    for (int i = 0; i < 3; i++) g[3][i] = g[3][i] + t[i];
    tap(2.0f, 0.0f, t); // z6
    for (int i = 0; i < 3; i++) g[3][i] = g[3][i] + t[i], g[4][i] = g[4][i] + t[i];
    tap(2.0f, 2.0f, t); // z7
    for (int i = 0; i < 3; i++) g[4][i] = g[4][i] + t[i];
    for (int k = 1; k < 5; k++)
        for (int i = 0; i < 3; i++) g[k][i] = (g[k][i] + c[i]) * 0.03125f;
    if (level0)
        for (int k = 0; k < 5; k++) {
            const float w = bloom_karis(g[k]);
            for (int i = 0; i < 3; i++) g[k][i] = g[k][i] * w;
        }
    for (int i = 0; i < 3; i++) result[i] = (((g[0][i] + g[1][i]) + g[2][i]) + g[3][i]) + g[4][i];
    if (level0) bloom_prefilter(tf, result);
}

// B6 of destination texel (x, y): what is added to it
template <class Fetch>
ORBIT_RASTER_FN void bloom_up_texel(const Fetch &fetch, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h, uint32_t x,
                                    uint32_t y, float r, float *result) {
    // x, y0..y3, z0..z3 in the shader's order, each added to its sum as it arrives
    float c[3], t[3], ys[3], zs[3];
    const auto tap = [&](float ox, float oy, float *out) {
        bloom_sample(fetch, bloom_up_u(x, ox, dst_w), bloom_up_u(y, oy, dst_h), src_w, src_h, out);
        ORBIT_POST_TAP_FENCE();
    };
    tap(0.0f, 0.0f, c);
    tap(r, 0.0f, ys);
    tap(0.0f, r, t);
    for (int i = 0; i < 3; i++) ys[i] = ys[i] + t[i];
    tap(-r, 0.0f, t);
    for (int i = 0; i < 3; i++) ys[i] = ys[i] + t[i];
    tap(0.0f, -r, t);
    for (int i = 0; i < 3; i++) ys[i] = ys[i] + t[i];
    tap(r, r, zs);
    tap(-r, -r, t);
    for (int i = 0; i < 3; i++) zs[i] = zs[i] + t[i];
    tap(-r, r, t);
    for (int i = 0; i < 3; i++) zs[i] = zs[i] + t[i];
    tap(r, -r, t);
    for (int i = 0; i < 3; i++) zs[i] = zs[i] + t[i];
    for (int i = 0; i < 3; i++) result[i] = (c[i] * 0.25f + ys[i] * 0.125f) + zs[i] * 0.0625f;
}

// B8 of a colour pixel: its rgb with non-finite components as +0.0f -> all three were finite
ORBIT_RASTER_FN bool bloom_color_texel(const float *color4, float *rgb) {
    bool all_finite = true;
    for (int i = 0; i < 3; i++) {
        rgb[i] = color4[i];
        all_finite = finite_or_zero(rgb[i]) && all_finite;
    }
    return all_finite;
}

// ---- T1-T5 of one pixel
enum : uint32_t { kPostNonfinite = 1u, kPostBloom = 2u };
ORBIT_RASTER_FN float post_clamp01(float x) { return !(x > 0.0f) ? 0.0f : x < 1.0f ? x : 1.0f; } // NaN -> 0
ORBIT_RASTER_FN void post_aces_fit(float *v) {
    for (int i = 0; i < 3; i++) {
        const float a = v[i] * (v[i] + 0.0245786f) - 0.000090537f;
        const float b = v[i] * (0.983729f * v[i] + 0.4329510f) + 0.238081f;
        v[i] = a / b;
    }
}
ORBIT_RASTER_FN float post_srgb(float c) { return c < 0.0031308f ? c * 12.92f : 1.055f * post_powc(c, 0.41666666f) - 0.055f; }
// color4: the pixel's four floats; with_bloom: T1's term from the packed texel `bloom` -> kPost* marks; ldr[4] and the four
// bytes as one word
ORBIT_RASTER_FN uint32_t post_pixel(const float *color4, bool with_bloom, uint32_t bloom, float exposure, float bloom_intensity, bool bgra,
                                    float *ldr, uint32_t &rgba8) {
    uint32_t marks = 0u;
    float hdr[3];
    if (!bloom_color_texel(color4, hdr)) marks |= kPostNonfinite;
    if (with_bloom) { // T1
        float b[3];
        bloom_unpack(bloom, b);
        for (int i = 0; i < 3; i++) {
            const float term = b[i] * bloom_intensity;
            if (term != 0.0f) marks |= kPostBloom;
            hdr[i] = hdr[i] + term;
            if (!finite_or_zero(hdr[i])) marks |= kPostNonfinite;
        }
    }
    float v[3], m[3];
    for (int i = 0; i < 3; i++) v[i] = hdr[i] * exposure;
    m[0] = (0.59719f * v[0] + 0.35458f * v[1]) + 0.04823f * v[2];
    m[1] = (0.07600f * v[0] + 0.90834f * v[1]) + 0.01566f * v[2];
    m[2] = (0.02840f * v[0] + 0.13383f * v[1]) + 0.83777f * v[2];
    post_aces_fit(m);
    ldr[0] = post_clamp01((1.60475f * m[0] + -0.53108f * m[1]) + -0.07367f * m[2]);
    ldr[1] = post_clamp01((-0.10208f * m[0] + 1.10813f * m[1]) + -0.00605f * m[2]);
    ldr[2] = post_clamp01((-0.00327f * m[0] + -0.07276f * m[1]) + 1.07602f * m[2]);
    ldr[3] = 1.0f;
    uint32_t byte[3];
    for (int i = 0; i < 3; i++) byte[i] = (uint32_t)(post_srgb(ldr[i]) * 255.0f + 0.5f);
    rgba8 = bgra ? (byte[2] | (byte[1] << 8) | (byte[0] << 16) | 0xFF000000u) : (byte[0] | (byte[1] << 8) | (byte[2] << 16) | 0xFF000000u);
    return marks;
}

} // namespace raster
} // namespace orbit
