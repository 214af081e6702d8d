// The wave64 and 256-thread-block sums and prefixes of the collision, statistics, selection and table kernels (multi_agent.hip, trial_stats.hip,
// postprocess.hip, cons_tables.hip): one text each, so the fixed order that a float sum's bits depend on is the same order everywhere.  Sets no fp contract.
#pragma once
#include <hip/hip_runtime.h>

namespace mmd {

// sum over the wave, on every lane: the xor butterfly 32, 16, .., 1 (fixed order: the result does not depend on scheduling)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// maximum over the wave, on every lane: the same butterfly
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}

// minimum over the wave, on every lane: the same butterfly
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}

// sum over a 256-thread block, on every thread.  LAST: the kernel's last use of lds4, which needs no barrier behind the read
template <bool LAST = false>
__device__ __forceinline__ int block_sum(int v, int* lds4) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  const int s = lds4[0] + lds4[1] + lds4[2] + lds4[3];
  if (!LAST) __syncthreads();
  return s;
}

// the cross-wave tail of the block prefixes: lds4[w] = wave w's total -> the block total; `before` = the total of the waves below this one
__device__ __forceinline__ int waves_before(const int* lds4, int& before) {
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  int total = before = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    before += w < wave ? lds4[w] : 0;
    total += lds4[w];
  }
  __syncthreads();
  return total;
}

// exclusive prefix of `flag` over a 256-thread block in thread order (one ballot a wave); returns the block total
__device__ __forceinline__ int block_prefix(bool flag, int* lds4, int& prefix) {
  const int lane = threadIdx.x & 63;
  const unsigned long long bal = __ballot(flag);
  if (lane == 0) lds4[threadIdx.x >> 6] = __popcll(bal);
  int before;
  const int total = waves_before(lds4, before);
  prefix = before + __popcll(bal & ((1ull << lane) - 1ull));
  return total;
}

// exclusive prefix of `v` over a 256-thread block in thread order (a __shfl_up scan a wave); returns the block total
__device__ __forceinline__ int block_prefix_count(int v, int* lds4, int& prefix) {
  const int lane = threadIdx.x & 63;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    inc += lane >= d ? o : 0;
  }
  if (lane == 63) lds4[threadIdx.x >> 6] = inc;
  int before;
  const int total = waves_before(lds4, before);
  prefix = before + inc - v;
  return total;
}

}  // namespace mmd
