#pragma once
// TEST INFRASTRUCTURE (tests/test_update_cpu.py): just enough of the HIP kernel language to run csrc/hip/rt_grid_build.hip on the CPU —
// blocks one after another, a block's threads as real threads with a barrier for __syncthreads, atomics as host atomics.
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint2 { uint32_t x, y; }; struct uint4 { uint32_t x, y, z, w; };
inline uint2 make_uint2(uint32_t a, uint32_t b) { return {a, b}; }
inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return {a, b, c, d}; }
inline thread_local dim3 threadIdx, blockIdx;
inline std::barrier<>* g_bar = nullptr;
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline uint32_t atomicMax(uint32_t* p, uint32_t v) { uint32_t o = __atomic_load_n(p, __ATOMIC_RELAXED); while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} return o; }
typedef int hipError_t; typedef void* hipStream_t;
constexpr int hipSuccess = 0;
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { std::memset(p, v, n); return 0; }
template <typename K, typename... A>
void hipLaunchKernelGGL(K k, dim3 grid, dim3 block, size_t, hipStream_t, A... a) {
  for (unsigned b = 0; b < grid.x; ++b) {
    std::barrier<> bar(block.x);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; ++t) th.emplace_back([=]() { blockIdx = dim3(b); threadIdx = dim3(t); k(a...); });
    for (auto& x : th) x.join();
  }
}
