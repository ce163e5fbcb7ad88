#pragma once
// TEST INFRASTRUCTURE (tests/test_flat_update_cpu.py): the kernel-language emulation of tests/update/emu plus the few things
// csrc/hip/rt_flat_build.hip uses beyond it — 16-byte double2 stores, atomicMin, a device-to-device copy.
#include "../../../update/emu/hip/hip_runtime.h"
struct double2 { double x, y; };
inline double2 make_double2(double a, double b) { return {a, b}; }
inline uint32_t atomicMin(uint32_t* p, uint32_t v) { uint32_t o = __atomic_load_n(p, __ATOMIC_RELAXED); while (o > v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} return o; }
constexpr int hipMemcpyDeviceToDevice = 3;
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, int, hipStream_t) { std::memcpy(dst, src, n); return 0; }
