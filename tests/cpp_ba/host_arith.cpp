// host_arith.cpp -- csrc/lba_internal.h under the schedule of Optimizer::BundleAdjustment, and csrc/initial_map_internal.h, compiled
// for the HOST: the items that ba_kernels.hip and initial_map_kernels.hip spread over the lanes of a workgroup, walked in order
// here, so that the arithmetic the kernels execute can be compared with the numpy yardstick on a machine without a GPU
// (tests/test_ba_cpu.py).  Same flags as the library (-ffp-contract=off).  chi2 and computeScale are summed in vertex order (poses,
// then points), where the kernel reduces over lanes; counts are exact either way.
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/initial_map_internal.h"

// orbfe_bundle_adjustment on the host: same arguments (edges already point by point, keyframes ascending), same outputs.
// Returns 0, or -1 where the device form refuses the problem.
extern "C" int ba_host(const orbfe_pose_camera* camera, const float* poses, const uint8_t* fixed, int n_kf, const float* points,
                       int n_points, const orbfe_lba_edge* edges, int n_edges, int n_iterations, int flags, float* poses_out,
                       float* points_out, orbfe_ba_result* result) {
  orbfe_ba_result res;
  memset(&res, 0, sizeof(res));
  res.n_edges = n_edges;
  memcpy(poses_out, poses, (size_t)n_kf * 48);
  memcpy(points_out, points, (size_t)n_points * 12);
  std::vector<int> kf_of_fi, slot_of_kf(n_kf, -1), fi_of_slot;
  for (int k = 0; k < n_kf; k++)
    if (!fixed[k]) kf_of_fi.push_back(k);
  const int n_free = (int)kf_of_fi.size();
  res.n_free = n_free;
  bool valid = n_free <= ORBFE_LBA_MAX_FREE;
  for (int i = 0; i < n_edges; i++) valid = valid && lba_edge_valid(edges, i, n_kf, n_points);
  if (!valid) {
    res.rounds = -1;
    *result = res;
    return -1;
  }
  if (n_free == 0 || n_edges == 0) {
    *result = res;
    return 0;
  }
  std::vector<uint8_t> ws(lba_ws_bytes(n_free, n_points, n_edges));
  std::vector<PoseSE3> pose(n_kf), pose_bak(n_kf);
  std::vector<int> kf_start(n_free + 1, 0);
  fi_of_slot.resize(n_free);
  LbaWs W;
  lba_ws_carve(ws.data(), n_free, n_points, n_edges, W);
  W.n_kf = n_kf; W.n_pt = n_points; W.n_e = n_edges; W.n_free = n_free;
  W.edges = edges;
  W.K = PoseIntr{(double)camera->fx, (double)camera->fy, (double)camera->cx, (double)camera->cy, (double)camera->mbf};
  W.pose = pose.data(); W.pose_bak = pose_bak.data(); W.slot_of_kf = slot_of_kf.data(); W.kf_of_fi = kf_of_fi.data();
  W.kf_start = kf_start.data(); W.fi_of_slot = fi_of_slot.data();
  for (int k = 0; k < n_kf; k++) pose[k] = pose_from_Tcw(poses + (size_t)k * 12);
  for (int p = 0; p < n_points; p++) {
    for (int j = 0; j < 3; j++) W.pt[3 * p + j] = (double)points[3 * p + j];
    W.pt_start[p] = W.pt_end[p] = 0;
    W.pt_active[p] = 0;
  }
  for (int i = 0; i < n_edges; i++) {
    const int p = edges[i].point;
    if (i == 0 || edges[i - 1].point != p) W.pt_start[p] = i;
    if (i == n_edges - 1 || edges[i + 1].point != p) W.pt_end[p] = i + 1;
    W.level[i] = 0;
    W.chi2[i] = 0.0;
  }
  int ns = 0;
  {
    int o = 0;
    for (int fi = 0; fi < n_free; fi++) {
      kf_start[fi] = o;
      for (int i = 0; i < n_edges; i++)
        if (edges[i].kf == kf_of_fi[fi]) W.kf_list[o++] = i;
      if (o > kf_start[fi]) {   // initializeOptimization: a free keyframe with an edge has a row block
        fi_of_slot[ns] = fi;
        slot_of_kf[kf_of_fi[fi]] = ns++;
      }
    }
    kf_start[n_free] = o;
  }
  const int n = 6 * ns;
  std::vector<double> bs(n), y(n), x(n), diag(n);
  const bool robust = (flags & ORBFE_BA_ROBUST) != 0;
  const double delta = ba_delta_mono();
  LmState lm{0.0, 2.0};
  double current_chi = 0.0;
  for (int it = 0; it < n_iterations; it++) {
    double chi = 0.0, maxd = 0.0;
    for (int p = 0; p < n_points; p++) lba_point_build(W, p, robust, &chi, &maxd, delta);
    for (int t = 0; t < ns * LBA_EKF; t++) {
      const double s = lba_kf_sum(W, fi_of_slot[t / LBA_EKF], t % LBA_EKF);
      if (lba_is_diag(t % LBA_EKF)) maxd = fmax(fabs(s), maxd);
    }
    current_chi = chi;
    if (it == 0) {
      lm.lambda = 1e-5 * maxd;
      lm.ni = 2.0;
      res.chi2_first = current_chi;
    }
    double rho = 0.0;
    int qmax = 0;
    do {
      const double lambda = lm.lambda;
      for (int p = 0; p < n_points; p++) lba_point_dinv(W, p, lambda);
      for (int t = 0; t < n; t++) bs[t] = lba_bschur(W, fi_of_slot[t / 6], t % 6);
      for (int i = 0; i < ns; i++)
        for (int j = i; j < ns; j++)
          for (int r = 0; r < 6; r++)
            for (int c = (i == j ? r : 0); c < 6; c++)
              W.S[(size_t)(6 * j + c) * n + (6 * i + r)] = lba_schur_entry(W, fi_of_slot[i], fi_of_slot[j], r, c, lambda);
      const bool ok2 = lba_cholesky_solve(W.S, n, diag.data(), bs.data(), y.data(), x.data());
      double temp_chi = 0.0, scale = 0.0, scale_pt = 0.0;
      if (ok2) {
        for (int s = 0; s < ns; s++) lba_pose_update(W, s, lambda, x.data(), &scale);
        for (int p = 0; p < n_points; p++) lba_point_update(W, p, lambda, x.data(), &scale_pt);
        scale += scale_pt;
        for (int p = 0; p < n_points; p++) lba_point_chi(W, p, robust, &temp_chi, delta);
      }
      res.trials++;
      if (lm_trial_scaled(lm, ok2, current_chi, temp_chi, scale, &rho)) {
        current_chi = temp_chi;
      } else {
        if (ok2) {
          for (int p = 0; p < n_points; p++) lba_point_pop(W, p);
          for (int s = 0; s < ns; s++) pose[kf_of_fi[fi_of_slot[s]]] = pose_bak[kf_of_fi[fi_of_slot[s]]];
        }
        if (!isfinite(lm.lambda)) break;
      }
      qmax++;
    } while (rho < 0 && qmax < 10);
    res.iterations++;
    if (qmax == 10 || rho == 0 || !isfinite(lm.lambda)) break;
  }
  res.chi2_final = current_chi;
  res.rounds = 1;
  for (int k = 0; k < n_kf; k++) pose_to_Tcw(pose[k], poses_out + (size_t)k * 12);
  for (int p = 0; p < n_points; p++)
    if (W.pt_start[p] < W.pt_end[p])
      for (int j = 0; j < 3; j++) points_out[3 * p + j] = (float)W.pt[3 * p + j];
  *result = res;
  return 0;
}

// The build stage of orbfe_create_initial_map on the host: index[n1] (-1 behind the points), points[n1][3] compacted, edges[2 n1]
// compacted, poses[2][12]; returns the number of points
extern "C" int imap_build_host(const orbfe_pose_camera* camera, const float* keys1, int n1, const float* keys2, int n2,
                               const int32_t* matches12, const float* P3D, const uint64_t* triangulated, const float* R21, const float* t21,
                               const int32_t* octaves1, const int32_t* octaves2, const float* pose1, int32_t* index, float* points,
                               orbfe_lba_edge* edges, float* poses) {
  int n = 0;
  for (int i = 0; i < n1; i++) {
    if (!imap_is_point(matches12[i], n2, triangulated[i >> 6], i & 63)) continue;
    const int m = matches12[i];
    index[n] = i;
    for (int c = 0; c < 3; c++) points[3 * n + c] = P3D[3 * i + c];
    imap_edges(*camera, n, keys1 + 2 * i, octaves1[i], keys2 + 2 * m, octaves2[m], edges + 2 * n);
    n++;
  }
  for (int j = n; j < n1; j++) index[j] = -1;
  imap_poses(pose1, R21, t21, poses);
  return n;
}

// The finish stage on the host, from the adjustment's outputs (poses_ba[2][12], points_ba[n][3] compacted) and the keypoint of
// frame 2 of every point: depths[n], poses[2][12], points[n][3] compacted, result (its ba record is left alone)
extern "C" void imap_finish_host(const float* poses_ba, const float* points_ba, const int32_t* match_of_point, int n, int n2, int q,
                                 int min_points, int ba_rounds, float* depths, float* poses, float* points,
                                 orbfe_initial_map_result* result) {
  std::vector<uint32_t> keys(n);
  std::vector<int> owner(n2 > 0 ? n2 : 1, -1);
  for (int j = 0; j < n; j++) {
    depths[j] = imap_depth(poses_ba, points_ba + 3 * j);
    keys[j] = imap_depth_key(depths[j]);
    owner[match_of_point[j]] = j;
  }
  int tracked = 0;
  for (int j = 0; j < n; j++) tracked += owner[match_of_point[j]] == j ? 1 : 0;
  std::stable_sort(keys.begin(), keys.end());
  const float median = n > 0 ? imap_key_depth(keys[(n - 1) / q]) : 0.0f;
  const int reason = imap_reason(n, median, tracked, min_points, ba_rounds);
  const float inv = imap_inv_median(median);
  for (int j = 0; j < 24; j++) poses[j] = (reason == 0 && j >= 12 && (j & 3) == 3) ? imap_scaled(poses_ba[j], inv) : poses_ba[j];
  for (int j = 0; j < 3 * n; j++) points[j] = reason == 0 ? imap_scaled(points_ba[j], inv) : points_ba[j];
  result->n_points = n;
  result->tracked = tracked;
  result->median_depth = median;
  result->success = reason == 0;
  result->reason = reason;
}

// sizeof of the records of include/orbfe.h, for the layout check of the ctypes side
extern "C" void ba_host_sizes(int32_t* out) {
  out[0] = (int32_t)sizeof(orbfe_ba_result);
  out[1] = (int32_t)offsetof(orbfe_ba_result, chi2_first);
  out[2] = (int32_t)sizeof(orbfe_initial_map_result);
  out[3] = (int32_t)offsetof(orbfe_initial_map_result, ba);
  out[4] = (int32_t)offsetof(orbfe_initial_map_result, median_depth);
}
