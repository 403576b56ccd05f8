// fragments_shade_shadowed.hip — orbit_fragments_shade_shadowed (include/orbit_abi_ext.h H1-H10 on top of L1-L9,
// DESIGN.md §4.26): orbit_fragments_shade with the shadowed directional lights served — cascade selection, bias, the
// 12-tap blocker search and the 32 x 4-tap filter over the caller's float depth maps.  The arithmetic is shade_common.h's
// and shadow_common.h's, shared with the host mirror, which is the pin.
//
// The two launches, the two forms of the light walk and the tile loop are shade_walk.h's, in ShadowedTier: the clear also
// clears shadow_stats and with ORBIT_SHADE_CLEAR fills shadow_factor (1.0f) and cascade (0xFFFFFFFF).  H1's range check of
// a shadow row runs where the light's index is checked: per lane in the one form, by the staging lane in the other.
// H2-H8 run per lane inside either form: the taps are a pixel's own gathers, the offset table is read at wave-uniform
// indices from constant memory.  Lanes whose blocker count is 0 or 12 idle while their neighbours filter (DESIGN.md §4.26
// counts how often).
#include "shade_walk.h"

namespace orbit {
namespace {

// the shadowed tier on the device: H10's words, planes and stats block
struct ShadowedDevice : ShadowedTier {
    static constexpr uint32_t kWords = kShadowEnd;
    __device__ static void count(uint32_t *count, bool written, const Extra &sp) { shadow_count(count, written, sp); }
    __device__ static void store(const Job &j, size_t p, const Extra &sp) { shadow_store(j, p, sp); }
    __device__ static void flush(const Job &j, const uint32_t *count) { shadow_flush(j, count); }
};

template <bool STAGED>
__global__ __launch_bounds__(kShadeThreads) void shadowed_kernel(const OrbitFragmentsShadeShadowed j, const uint32_t tiles_x,
                                                                 const uint32_t tiles, int32_t *status) {
    shade_tiles<ShadowedDevice, STAGED>(j, tiles_x, tiles, status);
}

} // namespace

hipError_t launch_fragments_shade_shadowed(const OrbitFragmentsShadeShadowed &job, uint32_t num_cus, uint32_t grid_cap, int32_t *status,
                                           hipStream_t s) {
    const ShadeGrid g = shade_grid(job.shade, num_cus, grid_cap);
    const hipError_t e = launch_shade_clear(job.shade, job.shadow_factor, job.cascade, job.shadow_stats, nullptr, g.cap, s);
    if (e != hipSuccess) return e;
    return launch_shade_tiles(shadowed_kernel<true>, shadowed_kernel<false>, job, g, status, s);
}

} // namespace orbit
