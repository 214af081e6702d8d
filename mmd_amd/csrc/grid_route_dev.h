// What the descent kernels of grid_route.hip and route_seeds.hip share: the lattice tile of a cell.
#pragma once
#include <hip/hip_runtime.h>

namespace mmd {

__device__ __forceinline__ long long floor_div(long long a, long long b) {     // b > 0
  const long long q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

}  // namespace mmd
