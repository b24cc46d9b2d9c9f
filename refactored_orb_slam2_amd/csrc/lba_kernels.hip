// lba_kernels.hip -- Optimizer::LocalBundleAdjustment (L/src/Optimizer.cc:437-760) for a batch of problems: free keyframe poses and
// marginalised points, both rounds of up to 5 and 10 Levenberg iterations with up to ten trials each, all inside one launch.  The
// arithmetic is lba_internal.h's, one item per call; this file is the choreography.
//
// One workgroup of 256 threads per problem.  How the workgroup builds its plan and how the items of one optimize() call are spread over
// its lanes is stated once, in lba_optimize.h, for this kernel and for ba_kernels.hip; what is here is the schedule of
// LocalBundleAdjustment: two calls, the classification of every edge after each, the erase list.
#include "lba_optimize.h"

__global__ __launch_bounds__(LBA_THREADS) void lba_kernel(LbaLaunch L) {
  __shared__ LbaShared sh;
  const int tid = threadIdx.x;
  const orbfe_lba_problem Q = L.problems[blockIdx.x];
  orbfe_lba_result* result = L.result + blockIdx.x;
  orbfe_lba_result res;
  res.rounds = -1;
  res.n_free = 0;
  res.n_edges = 0;
  res.iterations[0] = res.iterations[1] = res.trials[0] = res.trials[1] = 0;
  res.n_dropped = res.n_erase = res.reserved = 0;
  res.chi2_first[0] = res.chi2_first[1] = res.chi2_final[0] = res.chi2_final[1] = 0.0;
  LbaWs W;
  const int state = lba_prepare(L, Q, sh, W);
  if (state == LBA_UNADDRESSABLE) {
    if (tid == 0) *result = res;
    return;
  }
  uint8_t* erase = L.erase + Q.edge_offset;
  res.n_free = W.n_free;
  res.n_edges = W.n_e;
  if (state != LBA_READY) {   // uniform: the inputs have gone through as they are
    for (int i = tid; i < W.n_e; i += LBA_THREADS) erase[i] = 0;
    res.rounds = state == LBA_REFUSED ? -1 : 0;
    if (tid == 0) *result = res;
    return;
  }

  const bool first_only = (L.flags & ORBFE_LBA_FIRST_ROUND_ONLY) != 0;
  int rounds = 0;
  for (int rnd = 0; rnd < 2; rnd++) {
    LbaCall call;
    lba_optimize_call(W, sh, rnd == 0, pose_delta(false), rnd == 0 ? 5 : 10, call);
    if (rnd == 0) {
      res.iterations[0] = call.iterations;
      res.trials[0] = call.trials;
      res.chi2_first[0] = call.chi2_first;
      res.chi2_final[0] = call.chi2_final;
    } else {
      res.iterations[1] = call.iterations;
      res.trials[1] = call.trials;
      res.chi2_first[1] = call.chi2_first;
      res.chi2_final[1] = call.chi2_final;
    }
    rounds++;
    // Optimizer.cc:662-688, :700-724
    const bool last = rnd == 1 || first_only;
    int bad = 0;
    for (int i = tid; i < W.n_e; i += LBA_THREADS) {
      const int b = lba_edge_bad(W, i) ? 1 : 0;
      bad += b;
      if (last) erase[i] = (uint8_t)((b ? ORBFE_LBA_ERASE : 0) | (W.level[i] ? ORBFE_LBA_DROPPED : 0));
      else W.level[i] = (uint8_t)b;
    }
    bad = lm_reduce_count<LBA_WAVES>(bad, sh.red_i, tid);
    __syncthreads();
    if (last) {
      res.n_erase = bad;
      break;
    }
    res.n_dropped = bad;
  }
  res.rounds = rounds;
  lba_write_estimates(L, Q, sh, W, false);
  if (tid == 0) *result = res;
}

void orbfe_launch_lba(const LbaLaunch& L, int P, hipStream_t s) {
  if (P < 1) return;
  hipLaunchKernelGGL(lba_kernel, dim3(P), dim3(LBA_THREADS), 0, s, L);
}
