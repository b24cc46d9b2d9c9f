// host_arith.cpp -- csrc/optsim3_internal.h, with the lm_internal.h under it, compiled for the HOST: the loops that
// optsim3_kernels.hip spreads over the lanes of a workgroup, sequential here, so that the arithmetic the kernel executes can be
// compared with the numpy yardstick on a machine without a GPU (tests/test_optsim3_cpu.py).  Same flags as the library
// (-ffp-contract=off).  Sums run in correspondence order.
#include <stddef.h>
#include <string.h>

#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/optsim3_internal.h"

namespace {
struct Problem {
  std::vector<OsPair> E;
  std::vector<uint8_t> bad;
  OsCam K1, K2;
  double delta;
  bool fix_scale;
};

void edge(const OsSim3* T, const OsCam& K, double X, double Y, double Z, double ou, double ov, double w, double delta, double* acc) {
  double e0, e1, J0[7], J1[7];
  os_error(T[0], K, X, Y, Z, ou, ov, &e0, &e1);
  for (int d = 0; d < 7; d++) {
    double p0, p1, m0, m1;
    os_error(T[1 + 2 * d], K, X, Y, Z, ou, ov, &p0, &p1);
    os_error(T[2 + 2 * d], K, X, Y, Z, ou, ov, &m0, &m1);
    J0[d] = os_central(p0, m0);
    J1[d] = os_central(p1, m1);
  }
  double rho0, rho1;
  lm_huber(os_chi2(e0, e1, w), delta, &rho0, &rho1);
  lm_accumulate<7>(J0, J1, J0, false, e0, e1, 0.0, w, rho0, rho1, acc);   // two rows: the third J0 is a stand-in
}

double edge_chi2(const OsSim3& S, const OsCam& K, double X, double Y, double Z, double ou, double ov, double w) {
  double e0, e1;
  os_error(S, K, X, Y, Z, ou, ov, &e0, &e1);
  return os_chi2(e0, e1, w);
}

double robust_chi(const Problem& P, const OsSim3& S) {
  const OsSim3 Si = os_inverse(S);
  double chi = 0.0, rho0, rho1;
  for (size_t i = 0; i < P.E.size(); i++) {
    if (P.bad[i]) continue;
    const OsPair& E = P.E[i];
    lm_huber(edge_chi2(S, P.K1, E.x2, E.y2, E.z2, E.u1, E.v1, E.w1), P.delta, &rho0, &rho1);
    chi += rho0;
    lm_huber(edge_chi2(Si, P.K2, E.x1, E.y1, E.z1, E.u2, E.v2, E.w2), P.delta, &rho0, &rho1);
    chi += rho0;
  }
  return chi;
}
}  // namespace

// orbfe_optimize_sim3 on the host: same arguments, same outputs
extern "C" void optsim3_host(const orbfe_sim3_view* view1, const orbfe_sim3_view* view2, const orbfe_optsim3_pair* pairs, int n,
                             const float* s_R_t_in, float th2f, int fix_scale, orbfe_optsim3_result* result, uint8_t* bad) {
  orbfe_optsim3_result res;
  memset(&res, 0, sizeof(res));
  res.s = s_R_t_in[0];
  memcpy(res.R, s_R_t_in + 1, sizeof(res.R));
  memcpy(res.t, s_R_t_in + 10, sizeof(res.t));
  res.n_pairs = n;
  *result = res;
  if (n == 0) return;
  Problem P;
  P.E.resize(n);
  P.bad.assign(n, 0);
  P.K1 = OsCam{(double)view1->fx, (double)view1->fy, (double)view1->cx, (double)view1->cy};
  P.K2 = OsCam{(double)view2->fx, (double)view2->fy, (double)view2->cx, (double)view2->cy};
  P.delta = os_delta(th2f);
  P.fix_scale = fix_scale != 0;
  const double th2 = (double)th2f;
  for (int i = 0; i < n; i++) {
    float c1[3], c2[3];
    os_prepare(*view1, *view2, pairs[i], c1, c2);
    OsPair& E = P.E[i];
    E.x1 = c1[0]; E.y1 = c1[1]; E.z1 = c1[2];
    E.x2 = c2[0]; E.y2 = c2[1]; E.z2 = c2[2];
    E.u1 = pairs[i].obs1[0]; E.v1 = pairs[i].obs1[1];
    E.u2 = pairs[i].obs2[0]; E.v2 = pairs[i].obs2[1];
    E.w1 = pairs[i].inv_sigma2_1; E.w2 = pairs[i].inv_sigma2_2;
    bad[i] = 0;
  }
  OsSim3 S = os_from_floats(s_R_t_in);
  int n_bad = 0;
  for (int call = 0; call < 2; call++) {
    const int max_its = call == 0 ? 5 : (n_bad > 0 ? 10 : 5);
    LmState lm{0.0, 2.0};
    int its = 0;
    for (int it = 0; it < max_its; it++) {
      OsSim3 T[2 * OS_NTRANSFORMS];
      for (int j = 0; j < OS_NTRANSFORMS; j++) {
        T[j] = os_perturbed(S, j, P.fix_scale);
        T[OS_NTRANSFORMS + j] = os_inverse(T[j]);
      }
      double Hb[OS_NACC] = {0};
      for (int i = 0; i < n; i++) {
        if (P.bad[i]) continue;
        const OsPair& E = P.E[i];
        edge(T, P.K1, E.x2, E.y2, E.z2, E.u1, E.v1, E.w1, P.delta, Hb);
        edge(T + OS_NTRANSFORMS, P.K2, E.x1, E.y1, E.z1, E.u2, E.v2, E.w2, P.delta, Hb);
      }
      double current_chi = Hb[lm_chi<7>];
      if (it == 0) {
        lm.lambda = lm_lambda_init<7>(Hb);
        lm.ni = 2.0;
      }
      double rho = 0.0;
      int qmax = 0;
      do {
        double x[7];
        const bool ok2 = lm_ldlt_solve<7>(Hb, lm.lambda, Hb + lm_b<7>, x);
        OsSim3 trial = S;
        if (ok2) trial = os_oplus(S, x, P.fix_scale);
        const double temp_chi = ok2 ? robust_chi(P, trial) : 0.0;
        if (lm_trial<7>(lm, ok2, current_chi, temp_chi, x, Hb + lm_b<7>, &rho)) {
          current_chi = temp_chi;
          S = trial;
        } else if (!isfinite(lm.lambda)) {
          break;
        }
        qmax++;
      } while (rho < 0 && qmax < 10);
      its++;
      if (qmax == 10 || rho == 0 || !isfinite(lm.lambda)) break;
    }
    res.iterations[call] = its;
    const OsSim3 Si = os_inverse(S);
    int nb = 0;
    for (int i = 0; i < n; i++) {
      if (P.bad[i]) continue;
      const OsPair& E = P.E[i];
      const double c12 = edge_chi2(S, P.K1, E.x2, E.y2, E.z2, E.u1, E.v1, E.w1);
      const double c21 = edge_chi2(Si, P.K2, E.x1, E.y1, E.z1, E.u2, E.v2, E.w2);
      if (c12 > th2 || c21 > th2) {
        P.bad[i] = bad[i] = 1;
        nb++;
      }
    }
    if (call == 0) {
      n_bad = res.n_bad = nb;
      if (n - nb < 10) {
        *result = res;
        return;
      }
    } else {
      res.n_inliers = n - n_bad - nb;
    }
  }
  float v[13];
  os_to_floats(S, v);
  res.s = v[0];
  memcpy(res.R, v + 1, sizeof(res.R));
  memcpy(res.t, v + 10, sizeof(res.t));
  *result = res;
}

// the arithmetic alone, for the closed-form checks: Sim3(update) as 8 doubles (qx qy qz qw tx ty tz s)
extern "C" void optsim3_host_exp(const double* u, double* out) {
  const OsSim3 S = os_exp(u);
  out[0] = S.q.qx; out[1] = S.q.qy; out[2] = S.q.qz; out[3] = S.q.qw;
  out[4] = S.q.tx; out[5] = S.q.ty; out[6] = S.q.tz; out[7] = S.s;
}

// lm_internal.h's solve alone, for a vertex of n = 6 or 7 dimensions: (H + lambda I) x = b with H as its n (n + 1) / 2 upper entries.
// Returns 1 when every pivot was > 0, 0 when one was not, -1 for another n.
extern "C" int optsim3_host_ldlt(int n, const double* Hu, double lambda, const double* b, double* x) {
  if (n == 6) return lm_ldlt_solve<6>(Hu, lambda, b, x) ? 1 : 0;
  if (n == 7) return lm_ldlt_solve<7>(Hu, lambda, b, x) ? 1 : 0;
  return -1;
}

// sizeof of the two records of include/orbfe.h, for the layout check of the ctypes side
extern "C" void optsim3_host_sizes(int32_t* out) {
  out[0] = (int32_t)sizeof(orbfe_optsim3_pair);
  out[1] = (int32_t)sizeof(orbfe_optsim3_result);
  out[2] = (int32_t)offsetof(orbfe_optsim3_result, n_pairs);
  out[3] = (int32_t)offsetof(orbfe_optsim3_result, iterations);
}
