// host_arith.cpp -- csrc/lba_internal.h, with the pose_internal.h and lm_internal.h under it, compiled for the HOST: the items that
// lba_kernels.hip spreads over the lanes of a workgroup, walked in order here, so that the arithmetic the kernel executes can be
// compared with the numpy yardstick on a machine without a GPU (tests/test_lba_cpu.py).  Same flags as the library
// (-ffp-contract=off).  chi2 and computeScale are summed in vertex order (poses, then points), where the kernel reduces over lanes.
#include <stddef.h>
#include <string.h>

#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/lba_internal.h"

// orbfe_local_bundle_adjustment on the host: same arguments (edges already point by point, keyframes ascending), same outputs.
// Returns 0, or -1 where the device form refuses the problem.
extern "C" int lba_host(const orbfe_pose_camera* camera, const float* poses, const uint8_t* fixed, int n_kf, const float* points,
                        int n_points, const orbfe_lba_edge* edges, int n_edges, int flags, float* poses_out, float* points_out,
                        uint8_t* erase, orbfe_lba_result* result) {
  orbfe_lba_result res;
  memset(&res, 0, sizeof(res));
  res.n_edges = n_edges;
  memcpy(poses_out, poses, (size_t)n_kf * 48);
  memcpy(points_out, points, (size_t)n_points * 12);
  memset(erase, 0, (size_t)n_edges);
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
  {
    int o = 0;
    for (int fi = 0; fi < n_free; fi++) {
      kf_start[fi] = o;
      for (int i = 0; i < n_edges; i++)
        if (edges[i].kf == kf_of_fi[fi]) W.kf_list[o++] = i;
    }
    kf_start[n_free] = o;
  }
  std::vector<double> bs(6 * n_free), y(6 * n_free), x(6 * n_free), diag(6 * n_free);
  const bool first_only = (flags & ORBFE_LBA_FIRST_ROUND_ONLY) != 0;
  for (int rnd = 0; rnd < 2; rnd++) {
    const bool robust = rnd == 0;
    int ns = 0;
    for (int fi = 0; fi < n_free; fi++) {
      int c = 0;
      for (int q = kf_start[fi]; q < kf_start[fi + 1]; q++) c += W.level[W.kf_list[q]] ? 0 : 1;
      if (c > 0) {
        fi_of_slot[ns] = fi;
        slot_of_kf[kf_of_fi[fi]] = ns++;
      } else {
        slot_of_kf[kf_of_fi[fi]] = -1;
      }
    }
    const int n = 6 * ns;
    LmState lm{0.0, 2.0};
    double current_chi = 0.0;
    int iterations = 0, trials = 0;
    for (int it = 0; it < (rnd == 0 ? 5 : 10); it++) {
      double chi = 0.0, maxd = 0.0;
      for (int p = 0; p < n_points; p++) lba_point_build(W, p, robust, &chi, &maxd);
      for (int t = 0; t < ns * LBA_EKF; t++) {
        const double s = lba_kf_sum(W, fi_of_slot[t / LBA_EKF], t % LBA_EKF);
        if (lba_is_diag(t % LBA_EKF)) maxd = fmax(fabs(s), maxd);
      }
      current_chi = chi;
      if (it == 0) {
        lm.lambda = 1e-5 * maxd;
        lm.ni = 2.0;
        res.chi2_first[rnd] = current_chi;
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
          for (int p = 0; p < n_points; p++) lba_point_chi(W, p, robust, &temp_chi);
        }
        trials++;
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
      iterations++;
      if (qmax == 10 || rho == 0 || !isfinite(lm.lambda)) break;
    }
    res.iterations[rnd] = iterations;
    res.trials[rnd] = trials;
    res.chi2_final[rnd] = current_chi;
    res.rounds = rnd + 1;
    const bool last = rnd == 1 || first_only;
    int bad = 0;
    for (int i = 0; i < n_edges; i++) {
      const int b = lba_edge_bad(W, i) ? 1 : 0;
      bad += b;
      if (last) erase[i] = (uint8_t)((b ? ORBFE_LBA_ERASE : 0) | (W.level[i] ? ORBFE_LBA_DROPPED : 0));
      else W.level[i] = (uint8_t)b;
    }
    if (last) {
      res.n_erase = bad;
      break;
    }
    res.n_dropped = bad;
  }
  for (int k = 0; k < n_kf; k++)
    if (!fixed[k]) pose_to_Tcw(pose[k], poses_out + (size_t)k * 12);
  for (int p = 0; p < n_points; p++)
    if (W.pt_start[p] < W.pt_end[p])
      for (int j = 0; j < 3; j++) points_out[3 * p + j] = (float)W.pt[3 * p + j];
  *result = res;
  return 0;
}

// sizeof of the records of include/orbfe.h, for the layout check of the ctypes side
extern "C" void lba_host_sizes(int32_t* out) {
  out[0] = (int32_t)sizeof(orbfe_lba_edge);
  out[1] = (int32_t)sizeof(orbfe_lba_problem);
  out[2] = (int32_t)sizeof(orbfe_lba_result);
  out[3] = (int32_t)offsetof(orbfe_lba_result, chi2_first);
  out[4] = (int32_t)offsetof(orbfe_lba_result, n_dropped);
}
