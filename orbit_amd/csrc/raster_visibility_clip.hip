// raster_visibility_clip.hip — raster_visibility.hip compiled a second time with ORBIT_RASTER_CLIP = 1: the kernel that
// ORBIT_RASTER_CLIP_NEAR launches (include/orbit_abi_ext.h R3c) and its launch; the resolve is not
// compiled again.  A translation unit of its own, so that raster_visibility.hip's kernel stays what it was.
#define ORBIT_RASTER_CLIP 1
#include "raster_visibility.hip"
