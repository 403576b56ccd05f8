// raster_visibility_wide.hip — raster_visibility.hip compiled a third time with ORBIT_RASTER_CLIP = 2: the kernel that
// ORBIT_RASTER_WIDE_GUARD launches (include/orbit_abi_ext.h R4w) and its launch; the resolve is not
// compiled again.  A translation unit of its own, so that the other two visibility kernels stay what they were.
#define ORBIT_RASTER_CLIP 2
#include "raster_visibility.hip"
