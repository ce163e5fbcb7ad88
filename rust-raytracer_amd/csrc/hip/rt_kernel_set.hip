// rt_kernel_set.hip — one set of the megakernel's instantiations, the valid keys with key >> 6 == RT_KERNEL_SET (rt_kernel.hip:
// QUADS 8 | SOLID 4 | MEDIUM 2 | MOTION 1), as a translation unit of its own.  The product build (build.py) compiles it once per set 1 - 15
// beside rt_hip_api.hip, which holds set 0 and, built with -DRT_KERNEL_SET_SPLIT, takes the other sets' table slices from here.  (The sets
// 8 - 15, the QUADS kernels of DESIGN.md §20, hold eight instantiations each.)
#if !defined(RT_KERNEL_SET) || RT_KERNEL_SET < 1 || RT_KERNEL_SET > 15
#error "compile with -DRT_KERNEL_SET=1 .. 15"
#endif
#include "rt_kernel.hip"

template rtk::KernelSetTable rtk::kernel_set<RT_KERNEL_SET>();
