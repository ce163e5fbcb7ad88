// rt_kernel_motion.hip — the 48 MOTION instantiations of the megakernel (motion blur) as a translation unit of their
// own.  The product build (build.py) compiles it beside rt_hip_api.hip, which is built with -DRT_MOTION_TU_SPLIT and declares these
// instantiations `extern template`, so the two halves of the kernel set compile in parallel.  Built alone, rt_hip_api.hip
// instantiates them itself (tools/codeobj_stats.py, tools/ab_bench.py).
#include <hip/hip_runtime.h>

#define RT_KERNEL_MOTION_TU
#include "rt_kernel.hip"

#define RT_MOTION_DEFINE(HL, S, LDS, WIDE, A, LE) template __global__ void rtk::rt_megakernel<HL, S, LDS, WIDE, A, LE, true>(rtk::KArgs);
RT_MOTION_INSTANTIATIONS(RT_MOTION_DEFINE)
