// optsim3.cpp -- C ABI of Optimizer::OptimizeSim3 (include/orbfe.h: orbfe_optimize_sim3, orbfe_optimize_sim3_batch_device).  The entry
// points validate, stage and launch optsim3_kernels.hip.  No CPU fallback: without a device both forms are an error.
#include <string.h>

#include "host_internal.h"
#include "optsim3_internal.h"

#define OS_MAX_PAIRS 9500   // the frame limit of the projection searches (include/orbfe.h: hard limits)

extern "C" int orbfe_optimize_sim3_batch_device(int P, const orbfe_sim3_view* d_view1, const orbfe_sim3_view* d_view2,
                                                const orbfe_optsim3_pair* d_pairs, const int32_t* d_n, int cap, const float* d_s_R_t_in,
                                                const float* d_th2, const int32_t* d_fix_scale, orbfe_optsim3_result* d_result,
                                                uint8_t* d_bad, void* stream) {
  if (P < 0 || P > OS_MAX_PROBLEMS || cap < 0 || cap > OS_MAX_PAIRS) {
    orbfe_set_error("optimize sim3 batch: P %d (0 .. %d), cap %d (0 .. %d)", P, OS_MAX_PROBLEMS, cap, OS_MAX_PAIRS);
    return ORBFE_ERR_INVALID;
  }
  if (!d_view1 || !d_view2 || !d_n || !d_s_R_t_in || !d_th2 || !d_fix_scale || !d_result || (cap > 0 && (!d_pairs || !d_bad))) {
    orbfe_set_error("optimize sim3 batch: every pointer is required (d_pairs and d_bad with cap > 0)");
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_view1 & 3) || ((uintptr_t)d_view2 & 3) || ((uintptr_t)d_pairs & 3) || ((uintptr_t)d_n & 3) || ((uintptr_t)d_s_R_t_in & 3) ||
      ((uintptr_t)d_th2 & 3) || ((uintptr_t)d_fix_scale & 3) || ((uintptr_t)d_result & 3)) {
    orbfe_set_error("optimize sim3 batch: records must be 4-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (P == 0) return ORBFE_OK;
  OsLaunch L;
  memset(&L, 0, sizeof(L));
  L.view1 = d_view1; L.view2 = d_view2; L.pairs = d_pairs; L.n = d_n; L.cap = cap; L.s_R_t_in = d_s_R_t_in; L.th2 = d_th2;
  L.fix_scale = d_fix_scale; L.result = d_result; L.bad = d_bad;
  orbfe_launch_optimize_sim3(L, P, (hipStream_t)stream);
  return hip_status("optimize sim3 batch: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_optimize_sim3(const orbfe_sim3_view* view1, const orbfe_sim3_view* view2, const orbfe_optsim3_pair* pairs, int n,
                                   const float* s_R_t_in, float th2, int fix_scale, orbfe_optsim3_result* result, uint8_t* bad) {
  if (!view1 || !view2 || !s_R_t_in || !result) {
    orbfe_set_error("optimize sim3: both views, s_R_t_in and result are required");
    return ORBFE_ERR_INVALID;
  }
  if (n < 0 || n > OS_MAX_PAIRS || !(th2 > 0.0f)) {
    orbfe_set_error("optimize sim3: n %d (0 .. %d), th2 %g (> 0)", n, OS_MAX_PAIRS, (double)th2);
    return ORBFE_ERR_INVALID;
  }
  if (n > 0 && (!pairs || !bad)) {
    orbfe_set_error("optimize sim3: pairs and bad are required for n > 0");
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (n == 0) {   // no edge: nothing is launched
    memset(result, 0, sizeof(*result));
    result->s = s_R_t_in[0];
    memcpy(result->R, s_R_t_in + 1, sizeof(result->R));
    memcpy(result->t, s_R_t_in + 10, sizeof(result->t));
    return ORBFE_OK;
  }
  HostCall c("optimize sim3");
  const size_t o_v1 = c.in(sizeof(orbfe_sim3_view)), o_v2 = c.in(sizeof(orbfe_sim3_view)), o_scal = c.in(64),
               o_pairs = c.in((size_t)n * sizeof(orbfe_optsim3_pair));
  const size_t o_res = c.out(sizeof(orbfe_optsim3_result)), o_bad = c.out((size_t)n);
  int rc;
  if ((rc = c.open())) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  memcpy(h + o_v1, view1, sizeof(orbfe_sim3_view));
  memcpy(h + o_v2, view2, sizeof(orbfe_sim3_view));
  // the scalars of the problem: 13 floats of the transform, th2, then n and fix_scale as int32
  memcpy(h + o_scal, s_R_t_in, 13 * sizeof(float));
  memcpy(h + o_scal + 52, &th2, sizeof(float));
  const int32_t scal[2] = {n, fix_scale != 0};
  memcpy(h + o_scal + 56, scal, sizeof(scal));
  memcpy(h + o_pairs, pairs, (size_t)n * sizeof(orbfe_optsim3_pair));
  if ((rc = c.upload())) return rc;
  OsLaunch L;
  memset(&L, 0, sizeof(L));
  L.view1 = (const orbfe_sim3_view*)(d + o_v1); L.view2 = (const orbfe_sim3_view*)(d + o_v2);
  L.pairs = (const orbfe_optsim3_pair*)(d + o_pairs); L.n = (const int32_t*)(d + o_scal + 56); L.cap = n;
  L.s_R_t_in = (const float*)(d + o_scal); L.th2 = (const float*)(d + o_scal + 52); L.fix_scale = (const int32_t*)(d + o_scal + 60);
  L.result = (orbfe_optsim3_result*)(d + o_res); L.bad = d + o_bad;
  orbfe_launch_optimize_sim3(L, 1, c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(result, h + o_res, sizeof(*result));
  memcpy(bad, h + o_bad, (size_t)n);
  return ORBFE_OK;
}
