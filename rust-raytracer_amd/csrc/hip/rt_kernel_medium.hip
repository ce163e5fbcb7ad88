// rt_kernel_medium.hip — the 32 static MEDIUM instantiations of the megakernel (participating media) as a translation
// unit of their own, compiled beside rt_hip_api.hip (built with -DRT_MOTION_TU_SPLIT, which declares them `extern template`).  Built
// alone, rt_hip_api.hip instantiates them itself (tools/codeobj_stats.py, tools/ab_bench.py).
#include <hip/hip_runtime.h>

#define RT_KERNEL_MOTION_TU
#include "rt_kernel.hip"

#define RT_MEDIUM_DEFINE(HL, S, LDS, A, LE, MO) template __global__ void rtk::rt_megakernel<HL, S, LDS, false, A, LE, MO, true>(rtk::KArgs);
RT_MEDIUM_INSTANTIATIONS(RT_MEDIUM_DEFINE, false)
