// fragment_common.h — the arithmetic of orbit_surface_fragments (include/orbit_abi_ext.h F2-F7), written
// once for the device kernel (surface_fragments.hip) and the host mirror (orbit_amd/host/orbit_raster.cpp).  Two steps:
// fragment_corner is F3, the vertex stage of one corner; fragment_pixel is the work of an owned pixel: F2's checks, the
// three corners, F4's interpolation, F5's uv differences, F6's material and F7's zeroing.  Both sides run both per pixel.
// Equal inputs, equal functions: equal bytes.  Every read is of the bytes a rule names and no more: 12 + 4 + 8 + 4 of a
// vertex, 2 of a meshlet, so a buffer may end with its last attribute.
#pragma once
#include "../../include/orbit_abi_ext.h"
#include "surface_common.h" // finite_or_zero, and raster_common.h's clip_position

namespace orbit {
namespace raster {

enum FragmentVerdict : uint32_t { kFragmentWritten = 0, kFragmentUnshaded = 1, kFragmentStale = 2 }; // of an owned pixel
constexpr uint32_t kFragmentFloats = 17u; // world_pos 4 @0, normal 3 @4, tangent 4 @7, uv 2 @11, uv_grad 4 @13

struct FragmentCorner { // F3's outputs of one corner: 13 floats
    float wp[4], n[3], t[4], uv[2];
};

// the cull path's snorm8 (orbit_device.h): a product with the float of 0x3C010204, not a quotient; -128 is not clamped
ORBIT_RASTER_FN float fragment_snorm8(int8_t i) { return (float)(int32_t)i * bits_float(0x3C010204); }

// F3's normalize(M3 x v): M3 = rows and columns 0..2 of the column-major m
ORBIT_RASTER_FN void fragment_direction(const float *m, float x, float y, float z, float *out) {
    float v[3];
    for (int r = 0; r < 3; r++) v[r] = (m[r] * x + m[4 + r] * y) + m[8 + r] * z;
    const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int r = 0; r < 3; r++) out[r] = v[r] / len;
}

// F3 of global vertex g < vertex_count of an entity < entity_count
ORBIT_RASTER_FN void fragment_corner(const OrbitSurfaceFragments &j, uint32_t g, const OrbitEntityData &e, FragmentCorner &out) {
    const uint8_t *row = (const uint8_t *)j.vertices + (uint64_t)g * j.vertex_stride;
    float pos[3];
    int8_t n[4], t[4];
    __builtin_memcpy(pos, row + j.position_offset, 12);
    __builtin_memcpy(n, row + j.normal_offset, 4);
    __builtin_memcpy(out.uv, row + j.uv_offset, 8);
    __builtin_memcpy(t, row + j.tangent_offset, 4);
    const Clip wp = clip_position(e.model_matrix, pos[0], pos[1], pos[2]);
    out.wp[0] = wp.x, out.wp[1] = wp.y, out.wp[2] = wp.z, out.wp[3] = wp.w;
    fragment_direction(e.normal_matrix, fragment_snorm8(n[0]), fragment_snorm8(n[1]), fragment_snorm8(n[2]), out.n);
    fragment_direction(e.normal_matrix, fragment_snorm8(t[0]), fragment_snorm8(t[1]), fragment_snorm8(t[2]), out.t);
    out.t[3] = fragment_snorm8(t[3]);
}

// F4 of one component
ORBIT_RASTER_FN float fragment_mix(float a0, float a1, float a2, float l0, float l1, float l2) { return (a0 * l0 + a1 * l1) + a2 * l2; }

// F2 and F4-F7 of pixel p, owned by command k < n -> the verdict; kFragmentWritten: out[0..16] in kFragmentFloats' order,
// material = F6, degenerate = F7's count of the pixel
ORBIT_RASTER_FN uint32_t fragment_pixel(const OrbitSurfaceFragments &j, uint32_t k, size_t p, float *out, uint32_t &material, bool &degenerate) {
    degenerate = false, material = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < kFragmentFloats; i++) out[i] = 0.0f;
    uint32_t tri[4];
    __builtin_memcpy(tri, j.triangle + 4u * p, 16);
    if (tri[0] == 0xFFFFFFFFu) return kFragmentUnshaded;
    const uint32_t *cmd = (const uint32_t *)j.draw_commands + 1u + 7u * (size_t)k;
    const uint32_t entity = cmd[4], meshlet = cmd[6];
    if (tri[0] >= j.entity_count || tri[0] != entity || (uint64_t)tri[1] >= j.vertex_count || (uint64_t)tri[2] >= j.vertex_count ||
        (uint64_t)tri[3] >= j.vertex_count || meshlet >= j.meshlet_count)
        return kFragmentStale;
    uint16_t material_index; // F6
    __builtin_memcpy(&material_index, (const uint8_t *)j.meshlets + 32u * (size_t)meshlet + 28u, 2);
    material = material_index;
    const OrbitEntityData &e = j.entity_data[entity];
    FragmentCorner c[3];
    for (int i = 0; i < 3; i++) fragment_corner(j, tri[1 + i], e, c[i]);
    float l[2];
    __builtin_memcpy(l, j.bary + 2u * p, 8);
    const float l1 = l[0], l2 = l[1];
    float l0 = (1.0f - l1) - l2;
    if (l0 < 0.0f) l0 = 0.0f;
    for (int i = 0; i < 4; i++) out[i] = fragment_mix(c[0].wp[i], c[1].wp[i], c[2].wp[i], l0, l1, l2);
    for (int i = 0; i < 3; i++) out[4 + i] = fragment_mix(c[0].n[i], c[1].n[i], c[2].n[i], l0, l1, l2);
    for (int i = 0; i < 4; i++) out[7 + i] = fragment_mix(c[0].t[i], c[1].t[i], c[2].t[i], l0, l1, l2);
    for (int i = 0; i < 2; i++) out[11 + i] = fragment_mix(c[0].uv[i], c[1].uv[i], c[2].uv[i], l0, l1, l2);
    if (j.grad) { // F5
        float d[4];
        __builtin_memcpy(d, j.grad + 4u * p, 16);
        for (int i = 0; i < 2; i++) {
            const float e1 = c[1].uv[i] - c[0].uv[i], e2 = c[2].uv[i] - c[0].uv[i];
            out[13 + i] = e1 * d[0] + e2 * d[1];
            out[15 + i] = e1 * d[2] + e2 * d[3];
        }
    }
    bool all_finite = true; // F7
    for (uint32_t i = 0; i < kFragmentFloats; i++) all_finite = finite_or_zero(out[i]) && all_finite;
    degenerate = !all_finite;
    return kFragmentWritten;
}

} // namespace raster
} // namespace orbit
