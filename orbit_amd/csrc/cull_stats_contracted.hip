// cull_stats_contracted.hip — cull_stats.hip compiled a second time with ORBIT_CONTRACT = 1 (orbit_device.h madd: every
// OpDot / OpMatrixTimesVector / OpMatrixTimesMatrix / Length / Distance of the cull shaders as an fma chain): the counts
// of a context with OrbitCaps.arith_profile = ORBIT_ARITH_CONTRACTED, class for class those of its contracted culls.  The
// externally visible launcher gets a suffix; the canonical one hands a launch whose parameter block says `arith` over to it
// (kernels.h).  The product's default build is cull_stats.hip itself, untouched by this file.
#define ORBIT_CONTRACT 1
#define launch_cull_stats launch_cull_stats_contracted
#include "cull_stats.hip"
