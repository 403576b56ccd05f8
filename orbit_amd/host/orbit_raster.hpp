// orbit_raster.hpp — host mirror of orbit_raster_depth (include/orbit_abi_ext.h R1-R9), and of
// orbit_raster_visibility and orbit_visibility_resolve (V1-V4, §4.13): the depth prepass of a
// MeshletDrawCommandBuffer, and the same pass keeping the winner, on HOST copies of the same buffers, sequential.  It is the reference of the GPU
// tests: the same depth bytes, the same counters, and a per-command flag where the device latches ORBIT_E_RANGE.  The
// arithmetic (transform, snap, setup, edge functions, depth plane) is ../csrc/raster_common.h, shared with the kernel;
// this side evaluates every edge function at every sample of a triangle's box directly, command after command (for a
// wide triangle of ORBIT_RASTER_WIDE_GUARD, R4w: at every sample of the 8 x 8 tiles of the box that no edge rules out).
#pragma once
#include <cstdint>

#include "../../include/orbit_abi_ext.h"

namespace orbit {
namespace raster {

struct HostJob {
    const uint32_t *draw_commands; // {count; 7 words per command}
    uint32_t max_commands;
    const uint32_t *meshlet_data;
    uint64_t meshlet_data_words;
    const uint8_t *vertices;
    uint64_t vertex_count;
    uint32_t vertex_stride, position_offset;
    const OrbitEntityData *entity_data;
    uint32_t entity_count;
    const float *view_proj;
    float *depth;
    uint32_t width, height, flags;
};

// Throws Panic for what the device call answers with ORBIT_E_INVALID.  stats and command_error (min(count,
// max_commands) flags, 1 = skipped by a range check) may be null.
void raster_depth(const HostJob &job, OrbitRasterStats *stats, int32_t *command_error);

// The same walk into width * height u64 words (V2); job.depth is not read.  command_error also flags V3's nt > 256.
void raster_visibility(const HostJob &job, uint64_t *visibility, uint32_t command_base, OrbitRasterStats *stats,
                       int32_t *command_error);

// orbit_visibility_resolve on a host buffer; depth, command_pixels (max_commands words) and stats may be null, not all.
void visibility_resolve(const uint64_t *visibility, uint32_t width, uint32_t height, uint32_t command_base,
                        uint32_t max_commands, float *depth, uint32_t *command_pixels, OrbitVisibilityStats *stats);

// orbit_visibility_compact (C1-C6, §4.18) on host buffers: the job's pointers are HOST pointers, `workspace` and
// `workspace_bytes` are not read.  Sequential, the obvious loop.  *status (may be null) = what the device call latches:
// ORBIT_E_RANGE if a visible command was inconsistent, else ORBIT_E_CAPACITY if one was dropped, else ORBIT_OK (the
// scan, which finds the first, runs before the emit, which finds the second).  Throws Panic for ORBIT_E_INVALID.
void visibility_compact(const OrbitVisibilityCompact &job, int32_t *status);

// orbit_visibility_surface (S1-S7, §4.21) on host buffers: the job's pointers are HOST pointers.  The obvious loop over
// the pixels, each through ../csrc/surface_common.h.  *status (may be null) = what the device call latches: ORBIT_E_RANGE
// if a pixel was stale, else ORBIT_OK.  Throws Panic for ORBIT_E_INVALID.
void visibility_surface(const OrbitVisibilitySurface &job, int32_t *status);

// orbit_visibility_surface_drawn (S2d, S3c, S3w, §4.23) on host buffers: the same loop, each pixel through
// surface_triangle_drawn and surface_pixel_drawn.  raster_flags: how the buffer was drawn, a subset of
// ORBIT_RASTER_CLIP_NEAR | ORBIT_RASTER_WIDE_GUARD; 0 gives visibility_surface's bytes.
void visibility_surface_drawn(const OrbitVisibilitySurface &job, uint32_t raster_flags, int32_t *status);

// orbit_surface_fragments (F1-F8, §4.24) on host buffers: the job's pointers are HOST pointers.  The obvious loop over
// the pixels, each through ../csrc/fragment_common.h.  *status (may be null) = what the device call latches: ORBIT_E_RANGE
// if a pixel was stale, else ORBIT_OK.  Throws Panic for ORBIT_E_INVALID (alignment and aliasing aside).
void surface_fragments(const OrbitSurfaceFragments &job, int32_t *status);

// orbit_fragments_shade (L1-L9, §4.25) on host buffers: the job's pointers are HOST pointers.  The obvious loop over the
// pixels, each through ../csrc/shade_common.h with the canonical slice; the FORCE flags are checked and change nothing.
// *status (may be null) = what the device call latches: ORBIT_E_RANGE if a pixel was stale, else ORBIT_OK.  Throws Panic
// for ORBIT_E_INVALID (alignment and aliasing aside).
void fragments_shade(const OrbitFragmentsShade &job, int32_t *status);

// orbit_fragments_shade_shadowed (H1-H10 on L1-L9, §4.26) on host buffers, as fragments_shade: the obvious loop over the
// pixels, each through ../csrc/shadow_common.h.  Throws Panic for ORBIT_E_INVALID (alignment and aliasing aside).
void fragments_shade_shadowed(const OrbitFragmentsShadeShadowed &job, int32_t *status);
// orbit_fragments_shade_sky (K1-K10 on H1-H10 and L1-L9, §4.31) on host buffers, as fragments_shade_shadowed: the obvious
// loop over the pixels, the covered ones through ../csrc/shade_common.h's walk in sky_common.h's SkyTier, the uncovered ones through its
// sky_box_pixel.  Throws Panic for what sky_check names: everything the device answers with ORBIT_E_INVALID, alignment
// and aliasing included.  census (may be null): ORBIT_HOST_SKY_CENSUS counters (orbit_host_c.h).
void fragments_shade_sky(const OrbitFragmentsShadeSky &job, int32_t *status, uint64_t *census = nullptr);
// H6 of the pixels (x0 + x, y0 + y), x < width, y < height, row-major: theta and the project's sine and cosine of it
void shadow_rotation(uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, float *theta, float *sine, float *cosine);

} // namespace raster
} // namespace orbit
