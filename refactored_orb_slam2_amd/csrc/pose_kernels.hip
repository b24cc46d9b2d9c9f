// pose_kernels.hip -- Optimizer::PoseOptimization (L/src/Optimizer.cc:233-435) for a batch of frames: one 6-DoF vertex, one unary
// edge per keypoint with a map point, four rounds of up to ten Levenberg iterations with up to ten trials each, all inside one
// launch.  The arithmetic is pose_internal.h's and, for the optimiser around the edges, lm_internal.h's.
//
// One workgroup of 512 threads per frame.  Lane t owns keypoint rows t, t + 512, ... and walks them in that order.  The edges of the
// first 2 048 rows are gathered once into LDS (keypoint, mvuRight, assignment -> point record: 7 floats and a flag byte per row); a
// row behind them is re-read from global memory for every evaluation, so no per-frame workspace exists and `cap` is bounded by
// nothing but the library's frame limit.  An iteration is one pass that accumulates the 21 upper entries of H, the 6 of b and chi in
// double, and every trial one pass for chi alone.  The sums are lm_reduce.h's: in an order that depends on nothing but the frame's
// own rows, so a frame's result is byte-identical from run to run, at any position in a batch and for any batch size.
// H, b and chi are left in LDS.  One wave runs the 6 x 6 solve, exp and the pose update of a trial and hands x and the trial pose
// to the others through LDS; the Levenberg bookkeeping (a few operations) is repeated by every lane on those identical values, so
// control flow is uniform over the workgroup by construction, which is what lets the barriers sit inside the trial loop.
// mvInvLevelSigma2 is indexed per lane and therefore read from LDS, not from a by-value argument.
// Level (0 / 1) of an edge between rounds = a flag bit in LDS (outlier[row] for a row behind the cache), which its own lane wrote.
//
// Deliberate deviation: after a round every edge is classified by its chi2 at the round's final pose.  The
// reference reads, for a level-0 edge, the error its last trial left behind (also a rejected one); the difference is ~1e-10.
#include "pose_internal.h"
#include "lm_reduce.h"

#ifndef PO_THREADS
#define PO_THREADS 512   // 64, 256 and 1 024 threads were measured against it: profiles/pose_optimization.md
#endif
#define PO_WAVES (PO_THREADS / 64)

struct PoRows {   // one frame's rows
  const orbfe_keypoint* kps;
  const float* u_right;      // nullable
  int32_t* assigned;
  const uint8_t* points;     // the source frame's records
  int stride, n_points, n_levels;
};

__device__ inline bool po_load_edge(const PoRows& F, const float* sig, int i, PoseEdge& E) {
  const int a = F.assigned[i];
  if (a < 0 || a >= F.n_points) return false;
  const int oct = F.kps[i].octave;
  if (oct < 0 || oct >= F.n_levels) return false;
  const float* P = reinterpret_cast<const float*>(F.points + (size_t)a * F.stride);
  const float r = F.u_right ? F.u_right[i] : -1.0f;
  E.X = (double)P[0];
  E.Y = (double)P[1];
  E.Z = (double)P[2];
  E.ou = (double)F.kps[i].x;
  E.ov = (double)F.kps[i].y;
  E.our = (double)r;
  E.stereo = !(r < 0);   // Optimizer.cc:279
  E.w = (double)sig[oct];
  return true;
}

// The edges of the first PO_LDS_ROWS keypoint rows, as the floats they are, in LDS: the ~120 passes of a frame then cost an LDS read
// per value instead of the dependent global loads assignment -> point record.  Rows behind it (frames larger than any KITTI / EuRoC
// / TUM frame) are re-read from global memory on every pass.  flags: 1 = an edge, 2 = stereo, 4 = level 1 (outlier).
#define PO_LDS_ROWS 2048
struct PoCache {
  float ou[PO_LDS_ROWS], ov[PO_LDS_ROWS], our[PO_LDS_ROWS], X[PO_LDS_ROWS], Y[PO_LDS_ROWS], Z[PO_LDS_ROWS], w[PO_LDS_ROWS];
  uint8_t flags[PO_LDS_ROWS];
};

// the edge of row i and its level; false when the row is no edge
__device__ inline bool po_edge(const PoRows& F, const PoCache& C, const float* sig, const uint8_t* outl, int i, PoseEdge& E, bool& level1) {
  if (i < PO_LDS_ROWS) {
    const uint8_t fl = C.flags[i];
    if (!(fl & 1)) return false;
    E.ou = (double)C.ou[i];
    E.ov = (double)C.ov[i];
    E.our = (double)C.our[i];
    E.X = (double)C.X[i];
    E.Y = (double)C.Y[i];
    E.Z = (double)C.Z[i];
    E.w = (double)C.w[i];
    E.stereo = (fl & 2) != 0;
    level1 = (fl & 4) != 0;
    return true;
  }
  if (!po_load_edge(F, sig, i, E)) return false;
  level1 = outl[i] != 0;
  return true;
}

__global__ __launch_bounds__(PO_THREADS) void pose_optimize_kernel(int n_frames, const orbfe_keypoint* __restrict__ keys_un,
                                                                   const float* __restrict__ u_right, const int32_t* __restrict__ n_rows,
                                                                   int cap, int32_t* assigned, const uint8_t* __restrict__ points,
                                                                   int point_stride, const int32_t* __restrict__ n_points, int p_cap,
                                                                   int frame_shift, const orbfe_pose_camera* __restrict__ camera,
                                                                   const float* __restrict__ Tcw_in, orbfe_pose_result* result,
                                                                   uint8_t* outlier, int flags) {
  __shared__ double red[PO_WAVES * POSE_NACC];
  __shared__ double Hb[POSE_NACC];   // H (21), b (6), chi of the iteration
  __shared__ double chi_t;           // chi of the trial
  __shared__ double sh_x[6];         // the trial's update, pose and whether the solve succeeded
  __shared__ PoseSE3 sh_trial;
  __shared__ int sh_ok;
  __shared__ int red_i[PO_WAVES];
  __shared__ float sig[ORBFE_MAX_LEVELS];
  __shared__ PoCache cache;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(n_rows[f], 0), cap);
  int fs = (f - frame_shift) % n_frames;
  if (fs < 0) fs += n_frames;
  const size_t row0 = (size_t)f * cap;
  PoRows F;
  F.kps = keys_un + row0;
  F.u_right = u_right ? u_right + row0 : nullptr;
  F.assigned = assigned + row0;
  F.points = points + (size_t)fs * p_cap * point_stride;
  F.stride = point_stride;
  F.n_points = min(max(n_points[fs], 0), p_cap);
  F.n_levels = min(camera->n_levels, ORBFE_MAX_LEVELS);   // sig[] holds no more
  uint8_t* outl = outlier + row0;
  if (tid < ORBFE_MAX_LEVELS) sig[tid] = camera->inv_level_sigma2[tid];
  PoseIntr K;
  K.fx = (double)camera->fx;
  K.fy = (double)camera->fy;
  K.cx = (double)camera->cx;
  K.cy = (double)camera->cy;
  K.bf = (double)camera->mbf;
  __syncthreads();

  // nInitialCorrespondences; mvbOutlier = false (rows without a point too: the reference leaves those untouched)
  int cnt = 0;
  for (int i = tid; i < n; i += PO_THREADS) {
    PoseEdge E;
    const bool is_edge = po_load_edge(F, sig, i, E);
    cnt += is_edge ? 1 : 0;
    outl[i] = 0;
    if (i < PO_LDS_ROWS) {   // the float values back as they came: every widening above was exact
      cache.flags[i] = (uint8_t)(is_edge ? (E.stereo ? 3 : 1) : 0);
      if (is_edge) {
        cache.ou[i] = (float)E.ou;
        cache.ov[i] = (float)E.ov;
        cache.our[i] = (float)E.our;
        cache.X[i] = (float)E.X;
        cache.Y[i] = (float)E.Y;
        cache.Z[i] = (float)E.Z;
        cache.w[i] = (float)E.w;
      }
    }
  }
  const int n_initial = lm_reduce_count<PO_WAVES>(cnt, red_i, tid);
  const float* Tin = Tcw_in + (size_t)f * 12;
  if (n_initial < 3) {   // Optimizer.cc:357: return 0, the pose is not touched
    if (tid == 0) {
      orbfe_pose_result r;
#pragma unroll
      for (int j = 0; j < 12; j++) r.Tcw[j] = Tin[j];
      r.n_initial = n_initial;
      r.n_bad = 0;
      r.n_inliers = 0;
      r.rounds = 0;
      r.iterations = 0;
      result[f] = r;
    }
    return;
  }

  const PoseSE3 pose0 = pose_from_Tcw(Tin);
  PoseSE3 pose = pose0;
  int n_bad = 0, rounds = 0, iterations = 0;
  bool robust = true;
  for (int rnd = 0; rnd < 4; rnd++) {
    pose = pose0;   // Optimizer.cc:370: every round starts from the input pose
    LmState lm;
    lm.lambda = 0.0;
    lm.ni = 2.0;
    const int n_active = n_initial - n_bad;   // the level-0 edges
    for (int it = 0; it < 10 && n_active > 0; it++) {
      double acc[POSE_NACC];
#pragma unroll
      for (int k = 0; k < POSE_NACC; k++) acc[k] = 0.0;
      for (int i = tid; i < n; i += PO_THREADS) {
        PoseEdge E;
        bool level1;
        if (!po_edge(F, cache, sig, outl, i, E, level1) || level1) continue;
        double e[3], x, y, z, rho0, rho1 = 1.0;
        const double chi2 = pose_edge_error(E, K, pose, e, &x, &y, &z);
        rho0 = chi2;
        if (robust) lm_huber(chi2, pose_delta(E.stereo), &rho0, &rho1);
        double J[3][6];   // linearizeOplus, then constructQuadraticForm
        pose_edge_jacobian(K, x, y, z, J[0], J[1], J[2]);
        lm_accumulate<6>(J[0], J[1], J[2], E.stereo, e[0], e[1], e[2], E.w, rho0, rho1, acc);
      }
      lm_reduce<POSE_NACC, POSE_NACC, PO_WAVES>(acc, red, Hb, tid);
      double current_chi = Hb[lm_chi<6>];
      if (it == 0) {
        lm.lambda = lm_lambda_init<6>(Hb);
        lm.ni = 2.0;
      }
      double rho = 0.0;
      int qmax = 0;
      do {
        // the 6 x 6 solve, exp and the pose update: one wave; every wave of a SIMD repeating them would take that SIMD's time again
        if (tid < 64) {
          double xs[6];
          const bool ok = lm_ldlt_solve<6>(Hb, lm.lambda, Hb + lm_b<6>, xs);
          PoseSE3 t = pose;
          if (ok) t = pose_mul(pose_exp(xs), pose);   // oplus
          if (tid == 0) {
#pragma unroll
            for (int j = 0; j < 6; j++) sh_x[j] = xs[j];
            sh_trial = t;
            sh_ok = ok ? 1 : 0;
          }
        }
        __syncthreads();
        double x[6];
#pragma unroll
        for (int j = 0; j < 6; j++) x[j] = sh_x[j];
        const PoseSE3 trial = sh_trial;
        const bool ok2 = sh_ok != 0;
        __syncthreads();   // read before the next trial's solve writes them again
        double temp_chi = 0.0;
        if (ok2) {   // uniform
          for (int i = tid; i < n; i += PO_THREADS) {
            PoseEdge E;
            bool level1;
            if (!po_edge(F, cache, sig, outl, i, E, level1) || level1) continue;
            double e[3], px, py, pz, rho0, rho1;
            const double chi2 = pose_edge_error(E, K, trial, e, &px, &py, &pz);
            rho0 = chi2;
            if (robust) lm_huber(chi2, pose_delta(E.stereo), &rho0, &rho1);
            temp_chi += rho0;
          }
          lm_reduce<1, POSE_NACC, PO_WAVES>(&temp_chi, red, &chi_t, tid);
          temp_chi = chi_t;
        }
        if (lm_trial<6>(lm, ok2, current_chi, temp_chi, x, Hb + lm_b<6>, &rho)) {
          current_chi = temp_chi;
          pose = trial;
        } else if (!isfinite(lm.lambda)) {
          break;
        }
        qmax++;
      } while (rho < 0 && qmax < 10);
      iterations++;
      if (qmax == 10 || rho == 0 || !isfinite(lm.lambda)) break;   // Terminate
    }
    // Optimizer.cc:374-421
    int bad = 0;
    for (int i = tid; i < n; i += PO_THREADS) {
      PoseEdge E;
      bool level1;
      if (!po_edge(F, cache, sig, outl, i, E, level1)) continue;
      double e[3], x, y, z;
      const float chi2 = (float)pose_edge_error(E, K, pose, e, &x, &y, &z);
      const int o = chi2 > pose_bound(E.stereo) ? 1 : 0;
      outl[i] = (uint8_t)o;
      if (i < PO_LDS_ROWS) cache.flags[i] = (uint8_t)((E.stereo ? 3 : 1) | (o ? 4 : 0));
      bad += o;
    }
    n_bad = lm_reduce_count<PO_WAVES>(bad, red_i, tid);
    if (rnd == 2) robust = false;
    rounds++;
    if (n_initial < 10) break;   // Optimizer.cc:423
  }
  if (tid == 0) {
    orbfe_pose_result r;
    pose_to_Tcw(pose, r.Tcw);
    r.n_initial = n_initial;
    r.n_bad = n_bad;
    r.n_inliers = n_initial - n_bad;
    r.rounds = rounds;
    r.iterations = iterations;
    result[f] = r;
  }
  if (flags & ORBFE_POSE_DISCARD) {   // Tracking.cc:815-826
    for (int i = tid; i < n; i += PO_THREADS)
      if (outl[i]) {
        F.assigned[i] = -1;
        outl[i] = 0;
      }
  }
}

void orbfe_launch_pose_optimize(int n_frames, const orbfe_keypoint* keys_un, const float* u_right, const int32_t* n, int cap,
                                int32_t* assigned, const uint8_t* points, int point_stride, const int32_t* n_points, int p_cap,
                                int frame_shift, const orbfe_pose_camera* camera, const float* Tcw_in, orbfe_pose_result* result,
                                uint8_t* outlier, int flags, hipStream_t s) {
  if (n_frames < 1) return;
  hipLaunchKernelGGL(pose_optimize_kernel, dim3(n_frames), dim3(PO_THREADS), 0, s, n_frames, keys_un, u_right, n, cap, assigned, points,
                     point_stride, n_points, p_cap, frame_shift, camera, Tcw_in, result, outlier, flags);
}
