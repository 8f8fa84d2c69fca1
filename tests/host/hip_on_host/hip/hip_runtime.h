// A stand-in for <hip/hip_runtime.h> that runs a kernel launch on CPU threads, for tests/host/mesh_eval_kernels_check.cpp only:
// with this directory first on the include path, csrc/mesh_eval.hip (and the real csrc/psdf_common.h) compile as plain C++20, so
// the kernels' own source runs under the address and undefined-behaviour sanitizers with no GPU.  What it models: one workgroup at
// a time, its threads as std::threads when hip_on_host::concurrent is set (kernels that use __syncthreads or __ballot need that;
// the barrier is a std::barrier, a ballot gathers the 64 lanes of the caller's wave), otherwise one after the other.  It models no
// timing, no memory hierarchy and no other part of the HIP API.
#pragma once
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)
#define __shared__ static

using std::isfinite;
using std::max;
using std::min;

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
typedef void* hipStream_t;
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
inline hipError_t hipGetLastError() { return hipSuccess; }

namespace hip_on_host {
inline bool concurrent = false;          // set by the caller before an entry whose kernel synchronises or ballots
inline std::barrier<>* barrier = nullptr;
inline unsigned char votes[1024];
}  // namespace hip_on_host
inline thread_local dim3 threadIdx, blockIdx;

inline void __syncthreads() { hip_on_host::barrier->arrive_and_wait(); }
// every thread of the workgroup must call it (true of the kernels checked here)
inline unsigned long long __ballot(bool vote) {
  using namespace hip_on_host;
  votes[threadIdx.x] = vote;
  barrier->arrive_and_wait();
  unsigned long long mask = 0;
  const unsigned wave = threadIdx.x & ~63u;
  for (unsigned l = 0; l < 64; l++) mask |= (unsigned long long)votes[wave + l] << l;
  barrier->arrive_and_wait();
  return mask;
}
inline int __popc(unsigned v) { return __builtin_popcount(v); }
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline int atomicAdd(int32_t* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline int atomicOr(int32_t* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
struct float4 {
  float x, y, z, w;
};
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
// cross-lane operations psdf_common.h names in helpers the checked kernels never call
template <class T> T __shfl_xor(T v, int, int) { return v; }
template <class T> T __shfl_up(T v, int, int) { return v; }
#define __builtin_amdgcn_update_dpp(old, src, ...) (src)

template <class Kernel, class... Args>
void hipLaunchKernelGGL(Kernel kernel, dim3 grid, dim3 block, int, hipStream_t, Args... args) {
  if (!hip_on_host::concurrent) {
    for (unsigned b = 0; b < grid.x; b++)
      for (unsigned t = 0; t < block.x; t++) {
        blockIdx = dim3(b);
        threadIdx = dim3(t);
        kernel(args...);
      }
    return;
  }
  // one std::thread per thread of a workgroup, the workgroups one after the other with a barrier between them.  A thread that
  // leaves the kernel early waits there, so an early exit must be taken by the whole workgroup (true of the kernels checked here).
  std::barrier<> bar(block.x);
  hip_on_host::barrier = &bar;
  std::fill(hip_on_host::votes, hip_on_host::votes + 1024, 0);
  std::vector<std::thread> threads;
  for (unsigned t = 0; t < block.x; t++)
    threads.emplace_back([&, t] {
      for (unsigned b = 0; b < grid.x; b++) {
        blockIdx = dim3(b);
        threadIdx = dim3(t);
        kernel(args...);
        bar.arrive_and_wait();
      }
    });
  for (auto& th : threads) th.join();
}
