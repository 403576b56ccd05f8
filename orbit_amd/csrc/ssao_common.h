// ssao_common.h — the arithmetic of orbit_ssao (include/orbit_abi_ext.h A1-A9), written once for the
// device kernels (ssao.hip) and the host mirror (orbit_amd/host/orbit_ssao.cpp).  The pieces: ssao_sample is B3's
// four-texel expression of one channel over a `fetch(ix, iy)` the caller hands in; ssao_position is A1 of one texel of the
// SSAO grid (its index as the shader's uvec2 has it, wrapped or beyond the grid alike); ssao_normal is A2 over the five
// positions of the cross; ssao_basis is A3; ssao_table_entry is A4 of one sample, which does not depend on the pixel;
// ssao_occlusion is A5 over such a table; ssao_byte is A6's store; ssao_blur_texel is A7 and ssao_pixel_read A8.  fp32,
// every operation rounded on its own.  Equal inputs, equal functions: equal bytes.
#pragma once
#include "post_common.h" // bloom_axis (B3), and shade_common.h's shade_max / clamp / dot / normalize, shadow_sincos, shadow_project

namespace orbit {
namespace raster {

constexpr uint32_t kSsaoMaxSamples = ORBIT_SSAO_MAX_SAMPLES;

// What a pixel reports beside its byte: A2's branch in bits 0-1 (0: right + up, 1: right + down, 2: left + up, 3: left +
// down), and the rest for A9 and the tests' census
enum : uint32_t { kSsaoBranchMask = 3u, kSsaoNonfinite = 4u, kSsaoTieHorizontal = 8u, kSsaoTieVertical = 16u };
// The tests' census over the samples of every pixel, kept by the mirror only (the device hands nullptr).  proj_at_zero /
// proj_at_one: in-range samples with a component exactly 0 / exactly 1; proj_below_zero / proj_above_one: rejected samples
// with a component one step outside — 1 + 2^-23 above, and below 0 the first value x * 0.5 + 0.5 can take, -2^-24
struct SsaoCensus {
    uint64_t occluded, unoccluded, range_inside, range_zero, range_one, range_nan, depth_equal, proj_at_zero, proj_at_one, proj_below_zero,
        proj_above_one;
};

// B3 of one channel at (u, v) of a w x h plane
template <class Fetch>
ORBIT_RASTER_FN float ssao_sample(const Fetch &fetch, float u, float v, uint32_t w, uint32_t h) {
    const BloomAxis ax = bloom_axis(u, w), ay = bloom_axis(v, h);
    const float t00 = fetch(ax.i0, ay.i0), t10 = fetch(ax.i1, ay.i0), t01 = fetch(ax.i0, ay.i1), t11 = fetch(ax.i1, ay.i1);
    const float gx = 1.0f - ax.f, gy = 1.0f - ay.f;
    return (t00 * gx + t10 * ax.f) * gy + (t01 * gx + t11 * ax.f) * ay.f;
}

ORBIT_RASTER_FN void ssao_cross(const float *a, const float *b, float *out) { // GLSL cross
    out[0] = a[1] * b[2] - b[1] * a[2];
    out[1] = a[2] * b[0] - b[2] * a[0];
    out[2] = a[0] * b[1] - b[0] * a[1];
}
ORBIT_RASTER_FN float ssao_mix(float a, float b, float t) { return a * (1.0f - t) + b * t; }
ORBIT_RASTER_FN float ssao_smoothstep(float e0, float e1, float x) {
    const float t = shade_clamp((x - e0) / (e1 - e0), 0.0f, 1.0f);
    return (t * t) * (3.0f - 2.0f * t);
}

// A1 (ssao.comp:51-71): the view-space position of texel (px, py) of the SSAO grid, px and py as the shader's uvec2 holds
// them (0xFFFFFFFF left of column 0); rcp = 1.0f / float(ssao size); depth: B3 over the full-size plane
template <class Fetch>
ORBIT_RASTER_FN void ssao_position(const Fetch &depth, const float *inverse_projection, uint32_t px, uint32_t py, float rcp_w, float rcp_h,
                                   uint32_t screen_w, uint32_t screen_h, float *position) {
    const float u = ((float)px + 0.5f) * rcp_w, v = ((float)py + 0.5f) * rcp_h;
    const float z = ssao_sample(depth, u, v, screen_w, screen_h);
    const float x = u * 2.0f - 1.0f, y = (1.0f - v) * 2.0f - 1.0f;
    float c[4];
    shadow_project(inverse_projection, x, y, z, 1.0f, c);
    for (int i = 0; i < 3; i++) position[i] = c[i] / c[3];
}

// A2 (:78-115): centre, right, left, down, up -> the normal and the marks
ORBIT_RASTER_FN uint32_t ssao_normal(const float *p0, const float *right, const float *left, const float *down, const float *up, float *normal) {
    const float dr = fabsf(right[2] - p0[2]), dl = fabsf(left[2] - p0[2]), dd = fabsf(down[2] - p0[2]), du = fabsf(up[2] - p0[2]);
    const bool take_right = dr < dl, take_down = dd < du;
    const float *p1, *p2;
    if (take_right && !take_down)
        p1 = right, p2 = up;
    else if (take_right && take_down)
        p1 = down, p2 = right;
    else if (!take_right && !take_down)
        p1 = up, p2 = left;
    else
        p1 = left, p2 = down;
    float a[3], b[3];
    for (int i = 0; i < 3; i++) a[i] = p2[i] - p0[i], b[i] = p1[i] - p0[i];
    ssao_cross(a, b, normal);
    shade_normalize(normal);
    return (take_right ? 0u : 2u) | (take_down ? 1u : 0u) | (dr == dl ? kSsaoTieHorizontal : 0u) | (dd == du ? kSsaoTieVertical : 0u);
}

// A3 (:120-127): the noise texel of SSAO pixel (gx, gy) and the basis around `normal`
ORBIT_RASTER_FN uint32_t ssao_repeat_texel(float coord, uint32_t size) { // NearestRepeat: floor(u * size) wrapped; coord >= 0
    return shade_f2u_sat(floorf(coord * (float)size)) % size;
}
ORBIT_RASTER_FN float ssao_snorm8(int8_t b) { return shade_max((float)b / 127.0f, -1.0f); }
ORBIT_RASTER_FN void ssao_basis(const int8_t *noise, uint32_t noise_size, uint32_t gx, uint32_t gy, const float *normal, float *tangent,
                                float *bitangent) {
    const uint32_t tx = ssao_repeat_texel((float)gx / (float)noise_size, noise_size), ty = ssao_repeat_texel((float)gy / (float)noise_size, noise_size);
    const int8_t *texel = noise + 2u * ((size_t)ty * noise_size + tx);
    float rv[3] = {ssao_snorm8(texel[0]), ssao_snorm8(texel[1]), 0.0f};
    shade_normalize(rv);
    const float d = shade_dot(rv, normal);
    for (int i = 0; i < 3; i++) tangent[i] = rv[i] - normal[i] * d;
    shade_normalize(tangent);
    ssao_cross(normal, tangent, bitangent);
}

// A4 (:134-141) of sample i: the hemisphere direction in entry[0..2] and the radius in entry[3]
ORBIT_RASTER_FN void ssao_table_entry(const uint8_t *samples, uint32_t samples_size, uint32_t i, uint32_t sample_count, float min_radius,
                                      float max_radius, float *entry) {
    const float fi = (float)i / (float)sample_count;
    const float z = (float)samples[4u * ssao_repeat_texel(fi, samples_size) + 2u] / 255.0f;
    uint32_t bits = (i << 16) | (i >> 16); // hammersley_2d, functions.glsl:51-61
    bits = ((bits & 0x55555555u) << 1) | ((bits & 0xAAAAAAAAu) >> 1);
    bits = ((bits & 0x33333333u) << 2) | ((bits & 0xCCCCCCCCu) >> 2);
    bits = ((bits & 0x0F0F0F0Fu) << 4) | ((bits & 0xF0F0F0F0u) >> 4);
    bits = ((bits & 0x00FF00FFu) << 8) | ((bits & 0xFF00FF00u) >> 8);
    const float rdi = (float)bits * 2.3283064365386963e-10f;
    const float phi = (rdi * 2.0f) * kShadePi; // hemispherepoint_uniform(fi, rdi)
    const float cos_theta = 1.0f - fi;
    const float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
    float s, c;
    shadow_sincos(phi, s, c);
    entry[0] = c * sin_theta, entry[1] = s * sin_theta, entry[2] = cos_theta;
    entry[3] = ssao_mix(min_radius, max_radius, z * z);
}

// A5's range test and range_check, on their own for the tests
ORBIT_RASTER_FN bool ssao_in_range(const float *q) {
    return q[0] == shade_clamp(q[0], 0.0f, 1.0f) && q[1] == shade_clamp(q[1], 0.0f, 1.0f) && q[2] == shade_clamp(q[2], 0.0f, 1.0f);
}
ORBIT_RASTER_FN float ssao_range_check(float min_radius, float sample_depth, float w) {
    const float sample_depth_lin = 0.01f / sample_depth;
    return ssao_smoothstep(0.0f, 1.0f, min_radius / fabsf(sample_depth_lin - w));
}

// A5 (:140-154) of one pixel over table[4 * sample_count] -> the occlusion sum; in_range: how many samples passed the
// range test; census (may be null): the tests' counters
template <class Fetch>
ORBIT_RASTER_FN float ssao_occlusion(const Fetch &depth, const float *projection, uint32_t screen_w, uint32_t screen_h, const float *p0,
                                     const float *tangent, const float *bitangent, const float *normal, const float *table,
                                     uint32_t sample_count, float min_radius, uint32_t &in_range, SsaoCensus *census) {
    float occlusion = 0.0f;
    in_range = 0u;
    for (uint32_t i = 0; i < sample_count; i++) {
        const float *e = table + 4u * i;
        float sp[3], c[4];
        for (int k = 0; k < 3; k++) {
            const float cone = (tangent[k] * e[0] + bitangent[k] * e[1]) + normal[k] * e[2];
            sp[k] = p0[k] - cone * e[3];
        }
        shadow_project(projection, sp[0], sp[1], sp[2], 1.0f, c);
        float q[3];
        for (int k = 0; k < 3; k++) q[k] = c[k] / c[3];
        q[0] = q[0] * 0.5f + 0.5f, q[1] = q[1] * -0.5f + 0.5f;
        if (!ssao_in_range(q)) {
            if (census)
                for (int k = 0; k < 3; k++) {
                    if (q[k] < 0.0f && q[k] >= -5.9604645e-8f) census->proj_below_zero++;
                    if (q[k] == 1.00000012f) census->proj_above_one++;
                }
            continue;
        }
        in_range++;
        const float sample_depth = ssao_sample(depth, q[0], q[1], screen_w, screen_h);
        const float range_check = ssao_range_check(min_radius, sample_depth, c[3]);
        const bool occluded = sample_depth >= q[2];
        occlusion = occlusion + (occluded ? 1.0f : 0.0f) * range_check;
        if (census) {
            for (int k = 0; k < 3; k++) {
                if (q[k] == 0.0f) census->proj_at_zero++;
                if (q[k] == 1.0f) census->proj_at_one++;
            }
            occluded ? census->occluded++ : census->unoccluded++;
            if (sample_depth == q[2]) census->depth_equal++;
            if (range_check != range_check)
                census->range_nan++;
            else if (range_check == 0.0f)
                census->range_zero++;
            else if (range_check == 1.0f)
                census->range_one++;
            else
                census->range_inside++;
        }
    }
    return occlusion;
}

// A6: the R8 byte of a value; NaN -> 0 and nonfinite
ORBIT_RASTER_FN uint32_t ssao_byte(float c, bool &nonfinite) {
    nonfinite = c != c;
    if (nonfinite) return 0u;
    return (uint32_t)(shade_clamp(c, 0.0f, 1.0f) * 255.0f + 0.5f);
}

// A6 of a pixel's occlusion sum -> its byte; marks: ssao_normal's, or-ed with kSsaoNonfinite where the value is NaN
ORBIT_RASTER_FN uint32_t ssao_pixel_byte(float occlusion, uint32_t sample_count, uint32_t &marks) {
    bool nonfinite;
    const uint32_t byte = ssao_byte(1.0f - occlusion / (float)sample_count, nonfinite);
    if (nonfinite) marks |= kSsaoNonfinite;
    return byte;
}

// A7 (ssao_blur.comp) of texel (x, y) of a w x h image: fetch(ix, iy) = byte / 255.0f
template <class Fetch>
ORBIT_RASTER_FN uint32_t ssao_blur_texel(const Fetch &fetch, uint32_t x, uint32_t y, uint32_t w, uint32_t h) {
    float sums[4];
    for (int g = 0; g < 4; g++) {
        const float ox = (g & 1) ? 2.0f : 0.0f, oy = (g & 2) ? 2.0f : 0.0f;
        const BloomAxis ax = bloom_axis((((float)x + 0.5f) - ox) / (float)w, w), ay = bloom_axis((((float)y + 0.5f) - oy) / (float)h, h);
        sums[g] = ((fetch(ax.i0, ay.i1) + fetch(ax.i1, ay.i1)) + fetch(ax.i1, ay.i0)) + fetch(ax.i0, ay.i0);
    }
    const float sum = (((sums[0] + sums[1]) + sums[2]) + sums[3]) * 0.0625f;
    bool nonfinite;
    return ssao_byte(sum, nonfinite);
}

// A8 (forward.frag:336-337) of screen pixel (x, y): B3 of the blurred image
template <class Fetch>
ORBIT_RASTER_FN float ssao_pixel_read(const Fetch &fetch, uint32_t x, uint32_t y, uint32_t screen_w, uint32_t screen_h, uint32_t w, uint32_t h) {
    return ssao_sample(fetch, ((float)x + 0.5f) / (float)screen_w, ((float)y + 0.5f) / (float)screen_h, w, h);
}

} // namespace raster
} // namespace orbit
