// lm_reduce.h -- the workgroup reductions of the kernels that run lm_internal.h's optimiser (pose_kernels.hip, optsim3_kernels.hip, lba_kernels.hip).
// Device only: the host builds of the arithmetic (tests/cpp_*) include lm_internal.h, never this.
//
// Reduction order: a lane's own rows (sequential) -> xor butterfly inside the wave (a + b == b + a, so every lane holds the same
// bits) -> the wave sums in wave order through LDS.  It depends on nothing but the workgroup's own rows, so a result is
// byte-identical from run to run, at any position in a batch and for any batch size.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

// The N sums of a workgroup of WAVES waves, left in tot[0 .. N); red holds WAVES rows of STRIDE doubles.  The callers leave H, b
// and chi in LDS (tot) and read them from there (uniform addresses: broadcasts) -- lm_nacc doubles less per lane to keep in
// registers across the trial loop, which is what lets two waves share a SIMD.
template <int N, int STRIDE, int WAVES>
__device__ inline void lm_reduce(double* v, double* red, double* tot, int tid) {
#pragma unroll
  for (int k = 0; k < N; k++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
  }
  __syncthreads();   // the readers of the reduction before are done
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) red[(tid >> 6) * STRIDE + k] = v[k];
  }
  __syncthreads();
  if (tid < N) {
    double s = red[tid];
#pragma unroll
    for (int w = 1; w < WAVES; w++) s += red[w * STRIDE + tid];
    tot[tid] = s;
  }
  __syncthreads();
}

// The count of the workgroup, returned to every lane; red holds WAVES ints
template <int WAVES>
__device__ inline int lm_reduce_count(int c, int* red, int tid) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = c;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < WAVES; w++) s += red[w];
  return s;
}

// The maximum of the workgroup, returned to every lane (max is exact in any order); red holds WAVES doubles
template <int WAVES>
__device__ inline double lm_reduce_max(double m, double* red, int tid) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; w++) s = fmax(s, red[w]);
  return s;
}
