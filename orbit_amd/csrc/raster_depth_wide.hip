// raster_depth_wide.hip — raster_depth.hip compiled a third time with ORBIT_RASTER_CLIP = 2: the kernel that
// ORBIT_RASTER_WIDE_GUARD launches (include/orbit_abi_ext.h R4w), the walker of raster_walk.h with kWide,
// and its launch.  A translation unit of its own, so that the other two depth kernels stay what they were.
#define ORBIT_RASTER_CLIP 2
#include "raster_depth.hip"
