// rt_kernel_set.hip — one set of the megakernel's instantiations, the valid keys with key >> 6 == RT_KERNEL_SET (rt_kernel.hip:
// SOLID 4 | MEDIUM 2 | MOTION 1), as a translation unit of its own.  The product build (build.py) compiles it once per set 1 - 7 beside
// rt_hip_api.hip, which holds set 0 and, built with -DRT_KERNEL_SET_SPLIT, takes the other sets' table slices from here.
#if !defined(RT_KERNEL_SET) || RT_KERNEL_SET < 1 || RT_KERNEL_SET > 7
#error "compile with -DRT_KERNEL_SET=1 .. 7"
#endif
#include "rt_kernel.hip"

template rtk::KernelSetTable rtk::kernel_set<RT_KERNEL_SET>();
