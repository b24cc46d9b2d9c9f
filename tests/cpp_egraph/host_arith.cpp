// host_arith.cpp -- csrc/egraph_internal.h, with the headers under it, compiled for the HOST: the per-edge and per-vertex items that
// egraph_kernels.hip hands to its lanes, in plain loops, so that the arithmetic the kernel executes can be compared with the numpy
// yardstick on a machine without a GPU (tests/test_egraph_cpu.py).  Same flags as the library (-ffp-contract=off).
#include <stddef.h>
#include <string.h>

#include "../../refactored_orb_slam2_amd/csrc/egraph_internal.h"

// The measurement of every edge (8 doubles: q, t, s), the error at the start estimates (err: 7 per edge, the SE3 form fills 6) and the
// Jacobians of vertex 0 and vertex 1 (Ji, Jj: 49 per edge, column-major D x D), whether the vertices are fixed or not
extern "C" void egraph_host_linearize(const orbfe_eg_vertex* V, const orbfe_eg_edge* E, int n_edges, int se3, double* meas, double* err,
                                      double* Ji, double* Jj) {
  for (int e = 0; e < n_edges; e++) {
    const bool loop = E[e].kind == ORBFE_EG_LOOP_CONNECTION;
    const OsSim3 Siw = eg_load(loop ? V[E[e].i].Scw : V[E[e].i].Snc), Sjw = eg_load(loop ? V[E[e].j].Scw : V[E[e].j].Snc);
    OsSim3 C = eg_measurement(Siw, Sjw);
    OsSim3 Si = eg_load(V[E[e].i].Scw), Sj = eg_load(V[E[e].j].Scw);
    if (se3) {
      C = eg_to_se3(C);
      Si = eg_to_se3(Si);
      Sj = eg_to_se3(Sj);
    }
    orbfe_eg_sim3 rec;
    eg_store(C, rec);
    memcpy(meas + 8 * (size_t)e, &rec, 64);
    double* er = err + 7 * (size_t)e;
    double* ji = Ji + 49 * (size_t)e;
    double* jj = Jj + 49 * (size_t)e;
    if (se3) {
      eg_error_se3(C.q, Si.q, Sj.q, er);
      eg_jacobians_se3(C.q, Si.q, Sj.q, ji, jj);
    } else {
      eg_error_sim3(C, Si, Sj, er);
      for (int d = 0; d < 7; d++) {
        double ep[7], em[7];
        eg_error_sim3(C, os_perturbed(Si, 1 + 2 * d, false), Sj, ep);
        eg_error_sim3(C, os_perturbed(Si, 2 + 2 * d, false), Sj, em);
        for (int r = 0; r < 7; r++) ji[d * 7 + r] = os_central(ep[r], em[r]);
        eg_error_sim3(C, Si, os_perturbed(Sj, 1 + 2 * d, false), ep);
        eg_error_sim3(C, Si, os_perturbed(Sj, 2 + 2 * d, false), em);
        for (int r = 0; r < 7; r++) jj[d * 7 + r] = os_central(ep[r], em[r]);
      }
    }
  }
}

// oplus of one record with an update of 7 (6 with se3) doubles
extern "C" void egraph_host_oplus(const orbfe_eg_sim3* in, const double* x, int se3, orbfe_eg_sim3* out) {
  const OsSim3 S = se3 ? eg_to_se3(eg_load(*in)) : eg_load(*in);
  eg_store(se3 ? eg_oplus_se3(S, x) : os_oplus(S, x, false), *out);
}

// poses_out rows of n records
extern "C" void egraph_host_poses(const orbfe_eg_sim3* in, int n, int se3, float* out) {
  for (int k = 0; k < n; k++) eg_pose_row(eg_load(in[k]), se3 != 0, out + 12 * (size_t)k);
}

// orbfe_sim3_correct_points on the host
extern "C" void egraph_host_correct_points(const float* points, int n, const int32_t* ref, const orbfe_eg_sim3* from, const orbfe_eg_sim3* to,
                                           float* out) {
  for (int p = 0; p < n; p++) {
    if (ref[p] < 0) {
      memcpy(out + 3 * (size_t)p, points + 3 * (size_t)p, 12);
      continue;
    }
    eg_correct_point(eg_load(from[ref[p]]), eg_load(to[ref[p]]), points + 3 * (size_t)p, out + 3 * (size_t)p);
  }
}
