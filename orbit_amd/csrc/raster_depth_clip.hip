// raster_depth_clip.hip — raster_depth.hip compiled as RasterVariant::ClipNear: the kernel that ORBIT_RASTER_CLIP_NEAR
// launches (include/orbit_abi_ext.h R3c), its occupancy query and its launch.  A translation unit of
// its own, because a second instantiation of the walker in one unit changes how the first one is scheduled (§4.14).
#define ORBIT_RASTER_VARIANT ClipNear
#include "raster_depth.hip"
