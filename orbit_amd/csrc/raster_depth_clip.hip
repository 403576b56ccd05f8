// raster_depth_clip.hip — raster_depth.hip compiled a second time with ORBIT_RASTER_CLIP = 1: the kernel that
// ORBIT_RASTER_CLIP_NEAR launches (include/orbit_abi_ext.h R3c), the walker of raster_walk.h with
// kClipNear, and its launch.  A translation unit of its own, so that raster_depth.hip's kernel stays, instruction for
// instruction, what it was before the flag existed.
#define ORBIT_RASTER_CLIP 1
#include "raster_depth.hip"
