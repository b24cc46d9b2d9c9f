// gba_internal.h -- what gba_kernels.hip and gba.cpp share: the workspace of ONE large problem of Optimizer::BundleAdjustment that
// the whole grid works on, the records the control kernel leaves for the host loop, and the launch interface.  The arithmetic is
// lba_internal.h's, item by item; this header adds no formula of its own beyond naming the terms a lane adds when it sums another
// kernel's shares (gba_edge_rho, gba_scale3, gba_scale6: the operands lba_point_build / lba_point_chi, lba_point_update and
// lba_pose_update add to their running sums, in their order).
#pragma once
#include "lba_internal.h"

constexpr int GBA_TB = 6 * ORBFE_GBA_TILE_KEYFRAMES;   // rows of one tile of the reduced system
constexpr int GBA_CHUNK = 4096;                        // edges per workgroup of the keyframe-list plan

enum { GBA_TRIAL = 0, GBA_BUILD = 1, GBA_DONE = 2 };   // GbaControl.action: what the host enqueues next

struct GbaDev {      // the problem's state, in HBM; written by one-workgroup kernels only (fail, invalid: the same value by many lanes)
  PoseIntr K;
  int state;         // LBA_REFUSED / LBA_IDLE / LBA_READY (lba_optimize.h's values)
  int invalid, n_free, ns, fail;
  int it, qmax, iterations, trials;
  double lambda, ni, current_chi, chi2_first, rho;
};

struct GbaControl {  // what the host loop reads once per trial
  int action, pop, state, n_free, ns, iterations, trials, reserved;
  double lambda, chi2_first, chi2;
};

struct GbaWs {       // carved over the caller's workspace for kf_cap keyframes, point_cap points and edge_cap edges
  LbaWs W;           // lba_internal.h's arrays (F = kf_cap); pose, pose_bak and the row-block maps point into HBM here
  double *b, *y, *x, *diag;   // [6 kf_cap]
  int *fi_of_kf;              // [kf_cap]: -1 for a fixed keyframe
  int *chunk_cnt;             // [chunks][kf_cap]: edges of free keyframe fi in chunk c, then their offset inside the keyframe's list
  uint8_t* pairs;             // [kf_cap][kf_cap]: row blocks (i < j) that share a point
  GbaDev* dev;
  GbaControl* control;
};

__host__ __device__ inline size_t gba_align(size_t v) { return (v + 255) & ~(size_t)255; }
__host__ __device__ inline size_t gba_chunks(int NE) { return ((size_t)NE + GBA_CHUNK - 1) / GBA_CHUNK; }
__host__ __device__ inline size_t gba_ws_bytes(int F, int NP, int NE) {
  size_t s = lba_ws_bytes(F, NP, NE);
  s += gba_align((size_t)2 * F * sizeof(PoseSE3));
  s += gba_align((size_t)24 * F * sizeof(double));
  s += gba_align(((size_t)5 * F + 1) * sizeof(int));
  s += gba_align(gba_chunks(NE) * (size_t)F * sizeof(int));
  s += gba_align((size_t)F * F);
  s += gba_align(sizeof(GbaDev)) + gba_align(sizeof(GbaControl));
  return s;
}
inline void gba_ws_carve(uint8_t* base, int F, int NP, int NE, GbaWs& G) {
  lba_ws_carve(base, F, NP, NE, G.W);
  uint8_t* p = base + lba_ws_bytes(F, NP, NE);
  G.W.pose = reinterpret_cast<PoseSE3*>(p);
  G.W.pose_bak = G.W.pose + F;
  p += gba_align((size_t)2 * F * sizeof(PoseSE3));
  G.b = reinterpret_cast<double*>(p);
  G.y = G.b + (size_t)6 * F;
  G.x = G.y + (size_t)6 * F;
  G.diag = G.x + (size_t)6 * F;
  p += gba_align((size_t)24 * F * sizeof(double));
  int* i = reinterpret_cast<int*>(p);
  G.W.slot_of_kf = i; i += F;
  G.fi_of_kf = i; i += F;
  G.W.kf_of_fi = i; i += F;
  G.W.fi_of_slot = i; i += F;
  G.W.kf_start = i;
  p += gba_align(((size_t)5 * F + 1) * sizeof(int));
  G.chunk_cnt = reinterpret_cast<int*>(p);
  p += gba_align(gba_chunks(NE) * (size_t)F * sizeof(int));
  G.pairs = p;
  p += gba_align((size_t)F * F);
  G.dev = reinterpret_cast<GbaDev*>(p);
  p += gba_align(sizeof(GbaDev));
  G.control = reinterpret_cast<GbaControl*>(p);
}

// What lba_point_build and lba_point_chi add to the running chi2 for edge i, from the chi2 they left in the edge
__host__ __device__ inline double gba_edge_rho(const LbaWs& W, int i, bool robust, double delta_mono) {
  const double chi2 = W.chi2[i];
  double rho0 = chi2, rho1;
  if (robust) lm_huber(chi2, !(W.edges[i].u_right < 0) ? pose_delta(true) : delta_mono, &rho0, &rho1);
  return rho0;
}
// What lba_point_update adds to computeScale for point p, and lba_pose_update for row block `slot`, one term at a time
__host__ __device__ inline void gba_scale3(const LbaWs& W, int p, double lambda, double* scale) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double x = W.xl[3 * p + k];
    *scale += x * (lambda * x + W.bl[3 * p + k]);
  }
}
__host__ __device__ inline void gba_scale6(const LbaWs& W, int slot, double lambda, const double* xp, double* scale) {
  const int fi = W.fi_of_slot[slot];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const double x = xp[6 * slot + j];
    *scale += x * (lambda * x + W.bp[6 * fi + j]);
  }
}

struct GbaLaunch {   // the arguments of orbfe_global_bundle_adjustment_device, all in HBM
  const orbfe_pose_camera* camera;
  const float* poses;
  const uint8_t* fixed;
  const uint8_t* points;
  int point_stride;
  const orbfe_lba_edge* edges;
  int n_kf, n_points, n_edges, n_iterations, flags;
  float* poses_out;
  float* points_out;
  orbfe_ba_result* result;
};

// gba_kernels.hip: the whole call on `s`; synchronous.  pinned: a GbaControl in pinned host memory.  phase_ms: null, or 7 sums of
// stream-event times (plan, build, Dinv / Schur, factorisation, solves, update / chi2, control read-back) for tools/gba_rate.py
enum { GBA_PH_PLAN, GBA_PH_BUILD, GBA_PH_SCHUR, GBA_PH_FACTOR, GBA_PH_SOLVE, GBA_PH_UPDATE, GBA_PH_CONTROL, GBA_PHASES };
hipError_t orbfe_run_gba(const GbaLaunch& L, const GbaWs& G, GbaControl* pinned, hipStream_t s, float* phase_ms);
