// raster_visibility_clip.hip — raster_visibility.hip compiled as RasterVariant::ClipNear: the kernel that
// ORBIT_RASTER_CLIP_NEAR launches (include/orbit_abi_ext.h R3c), its occupancy query and its launch; the
// resolve is not compiled again.  A translation unit of its own, as raster_depth_clip.hip is.
#define ORBIT_RASTER_VARIANT ClipNear
#include "raster_visibility.hip"
