// host emulation shim: one std::thread per HIP thread, blocks run one after another
#pragma once
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstddef>
#include <thread>
#include <vector>
#include <functional>
#define DPGP_GRAM_GRAD_MAX_Q 64
#define DPGP_OK 0
#define DPGP_ERR_LAUNCH -100
#define DPGP_PRELAUNCH()
#define DPGP_LAUNCH_CHECK()
#define __global__
#define __shared__
#define __align__(x)
#define __launch_bounds__(x)
#define __restrict__
typedef void *hipStream_t;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct double2 { double x, y; };
static thread_local dim3 threadIdx, blockIdx;
alignas(16) unsigned char g_smem[200000];
static std::barrier<> *g_bar;
static inline void __syncthreads() { g_bar->arrive_and_wait(); }
static inline int dpgp_ceil_div(int a, int b) { return (a + b - 1) / b; }
enum { hipSuccess = 0, hipFuncAttributeMaxDynamicSharedMemorySize = 1 };
static inline int hipFuncSetAttribute(const void *, int, int) { return hipSuccess; }
template <typename K, typename... A>
void hipLaunchKernelGGL(K kern, dim3 grid, dim3 block, size_t, hipStream_t, A... args) {
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            std::barrier<> bar(block.x);
            g_bar = &bar;
            std::vector<std::thread> ts;
            for (unsigned t = 0; t < block.x; ++t)
                ts.emplace_back([=]() { threadIdx = dim3(t); blockIdx = dim3(bx, by); kern(args...); });
            for (auto &th : ts) th.join();
        }
}
