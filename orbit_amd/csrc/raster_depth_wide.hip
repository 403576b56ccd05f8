// raster_depth_wide.hip — raster_depth.hip compiled as RasterVariant::Wide: the kernel that ORBIT_RASTER_WIDE_GUARD
// launches, with or without CLIP_NEAR (include/orbit_abi_ext.h R4w), its occupancy query and its
// launch.  A translation unit of its own, as raster_depth_clip.hip is.
#define ORBIT_RASTER_VARIANT Wide
#include "raster_depth.hip"
