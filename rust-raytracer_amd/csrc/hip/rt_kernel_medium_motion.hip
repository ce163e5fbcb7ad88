// rt_kernel_medium_motion.hip — the 32 MEDIUM + MOTION instantiations of the megakernel (media in a scene with moving spheres,
// DESIGN.md §14 and §15) as a translation unit of their own; see rt_kernel_medium.hip.
#include <hip/hip_runtime.h>

#define RT_KERNEL_MOTION_TU
#include "rt_kernel.hip"

#define RT_MEDIUM_DEFINE(HL, S, LDS, A, LE, MO) template __global__ void rtk::rt_megakernel<HL, S, LDS, false, A, LE, MO, true>(rtk::KArgs);
RT_MEDIUM_INSTANTIATIONS(RT_MEDIUM_DEFINE, true)
