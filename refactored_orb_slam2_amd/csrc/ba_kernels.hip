// ba_kernels.hip -- Optimizer::BundleAdjustment (L/src/Optimizer.cc:43-231) for a batch of problems: every keyframe but the one with
// mnId == 0 free, every observed point marginalised, ONE optimize() call of n iterations with the Huber kernel on every edge or on
// none, inside one launch.  No classification, no second round, no erase list.
//
// One workgroup of 256 threads per problem.  The plan, the spreading of one optimize() call over the lanes and the writing of the
// estimates are lba_optimize.h's, shared with lba_kernels.hip; the arithmetic is lba_internal.h's.  What is here is the schedule
// and the result record.
#include "lba_optimize.h"

__global__ __launch_bounds__(LBA_THREADS) void ba_kernel(LbaLaunch L, int n_iterations, orbfe_ba_result* results) {
  __shared__ LbaShared sh;
  const int tid = threadIdx.x;
  const orbfe_lba_problem Q = L.problems[blockIdx.x];
  orbfe_ba_result res;
  res.rounds = -1;
  res.n_free = res.n_edges = res.iterations = res.trials = res.reserved = 0;
  res.chi2_first = res.chi2_final = 0.0;
  LbaWs W;
  const int state = lba_prepare(L, Q, sh, W);
  if (state != LBA_UNADDRESSABLE) {
    res.n_free = W.n_free;
    res.n_edges = W.n_e;
  }
  if (state != LBA_READY) {   // uniform: nothing of the problem could be addressed, or its inputs have gone through as they are
    res.rounds = state == LBA_IDLE ? 0 : -1;
    if (tid == 0) results[blockIdx.x] = res;
    return;
  }
  LbaCall call;
  lba_optimize_call(W, sh, (L.flags & ORBFE_BA_ROBUST) != 0, ba_delta_mono(), n_iterations, call);
  res.rounds = 1;
  res.iterations = call.iterations;
  res.trials = call.trials;
  res.chi2_first = call.chi2_first;
  res.chi2_final = call.chi2_final;
  lba_write_estimates(L, Q, sh, W, true);
  if (tid == 0) results[blockIdx.x] = res;
}

void orbfe_launch_ba(const LbaLaunch& L, int n_iterations, orbfe_ba_result* result, int P, hipStream_t s) {
  if (P < 1) return;
  hipLaunchKernelGGL(ba_kernel, dim3(P), dim3(LBA_THREADS), 0, s, L, n_iterations, result);
}
