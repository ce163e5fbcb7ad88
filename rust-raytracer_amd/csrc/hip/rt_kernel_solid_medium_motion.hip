// rt_kernel_solid_medium_motion.hip — the 32 SOLID + MEDIUM + MOTION instantiations of the megakernel (solid textures) as a translation
// unit of their own; see rt_kernel_solid.hip.
#include <hip/hip_runtime.h>

#define RT_KERNEL_MOTION_TU
#include "rt_kernel.hip"

#define RT_SOLID_DEFINE(HL, S, LDS, A, LE, MO, ME) template __global__ void rtk::rt_megakernel<HL, S, LDS, false, A, LE, MO, ME, true>(rtk::KArgs);
RT_SOLID_INSTANTIATIONS(RT_SOLID_DEFINE, true, true)
