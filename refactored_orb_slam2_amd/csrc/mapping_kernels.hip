// mapping_kernels.hip -- the triangulation half of LocalMapping::CreateNewMapPoints (L/src/LocalMapping.cc:261-421) for every match
// of a (pKF1, pKF2) pair: one thread per pKF1 feature, ascending feature index = the reference's pair order.  The arithmetic is
// mapping_internal.h; this file only moves the rows.  blockIdx.y is the neighbour, so both view records are uniform per workgroup
// and travel through scalar loads; the per-lane octave indexes them in memory, never a by-value copy (frustum_kernels.hip, lesson 58).
// The triangulation kernel uses no atomics, no LDS and no scratch: a row's record depends on its own inputs only, so the result is
// independent of the launch shape.  The count kernel behind it sums the accepted rows of a pair in a fixed order over 1 KiB of LDS.
#include "mapping_internal.h"

#define TRI_THREADS 256
#define NP_DW (int)(sizeof(orbfe_new_point) / 4)   // 11
static_assert(sizeof(orbfe_tri_view) == 224 && sizeof(orbfe_new_point) == 44, "record layout");

__device__ __forceinline__ int tri_rows(const int32_t* n, int n_host, int k, int cap) {
  const int v = n ? n[k] : n_host;
  return min(max(v, 0), cap);
}

__global__ __launch_bounds__(TRI_THREADS) void triangulate_matches_kernel(TriLaunch T) {
  const int k = blockIdx.y, i = blockIdx.x * TRI_THREADS + threadIdx.x;
  const int nA = tri_rows(T.nA, T.nA_host, k, T.capA);
  if (i >= nA) return;   // rows at and behind nA[k] are neither read nor written
  const int nB = tri_rows(T.nB, T.nB_host, k, T.capB);
  const orbfe_tri_view& V1 = T.view1[0];
  const orbfe_tri_view& V2 = T.view2[k];
  const size_t rowA = (size_t)k * T.capA + i;
  orbfe_new_point P;
  uint32_t* pw = reinterpret_cast<uint32_t*>(&P);
#pragma unroll
  for (int j = 0; j < NP_DW; j++) pw[j] = 0u;
  P.idx2 = -1;
  P.code = ORBFE_TRI_NO_MATCH;
  const int idx2 = T.matchA[rowA];
  if (idx2 >= 0 && idx2 < nB) {
    const int L1 = min(V1.n_levels, ORBFE_MAX_LEVELS), L2 = min(V2.n_levels, ORBFE_MAX_LEVELS);
    const size_t rowB = (size_t)k * T.capB + idx2;
    const orbfe_keypoint kp1 = T.keys1[i], kp2 = T.keys2[rowB];
    if (kp1.octave >= 0 && kp1.octave < L1 && kp2.octave >= 0 && kp2.octave < L2) {   // otherwise "no match", nothing more is read
      TriObs o1, o2;
      o1.x = kp1.x; o1.y = kp1.y; o1.octave = kp1.octave;
      o1.u_right = T.u_right1 ? T.u_right1[i] : -1.0f;
      o1.depth = (T.depth1 && o1.u_right >= 0) ? T.depth1[i] : -1.0f;
      o2.x = kp2.x; o2.y = kp2.y; o2.octave = kp2.octave;
      o2.u_right = T.u_right2 ? T.u_right2[rowB] : -1.0f;
      o2.depth = (T.depth2 && o2.u_right >= 0) ? T.depth2[rowB] : -1.0f;
      const float ratio_factor = 1.5f * V1.scale_factors[1];   // 1.5f * mfScaleFactor (:210); mvScaleFactors[1] == mfScaleFactor
      int path;
      P.code = tri_pair(V1, V2, o1, o2, V1.level_sigma2[o1.octave], V2.level_sigma2[o2.octave], V1.scale_factors[o1.octave],
                        V2.scale_factors[o2.octave], V1.scale_factors[L1 - 1], ratio_factor, P, &path);
      P.path = path;
      P.idx2 = idx2;
      if (P.code != ORBFE_TRI_OK) {
#pragma unroll
        for (int j = 0; j < 8; j++) pw[j] = 0u;
      } else if (T.validA) {
        T.validA[i] = 0;   // pKF1->AddMapPoint(pMP, idx1) (:410): the next neighbour's search skips this feature (ORBmatcher.cc:655-664)
      }
    }
  }
  uint32_t* out = reinterpret_cast<uint32_t*>(T.out + rowA);
#pragma unroll
  for (int j = 0; j < NP_DW; j++) out[j] = pw[j];
}

// Accepted rows per pair, in a fixed order: one workgroup per pair, per-thread partial counts, a tree over LDS.
__global__ __launch_bounds__(TRI_THREADS) void triangulate_count_kernel(const orbfe_new_point* __restrict__ out, const int32_t* __restrict__ nA,
                                                                        int nA_host, int capA, int32_t* __restrict__ n_new,
                                                                        const int32_t* __restrict__ counters, int counter_stride,
                                                                        int32_t* __restrict__ n_matches) {
  __shared__ int red[TRI_THREADS];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int n = tri_rows(nA, nA_host, k, capA);
  int c = 0;
  for (int i = tid; i < n; i += TRI_THREADS) c += out[(size_t)k * capA + i].code == ORBFE_TRI_OK;
  red[tid] = c;
  __syncthreads();
  for (int s = TRI_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    n_new[k] = red[0];
    if (counters) n_matches[k] = counters[(size_t)k * counter_stride + 1];
  }
}

void orbfe_launch_triangulate(const TriLaunch& t, int K, hipStream_t s) {
  if (K < 1 || t.capA < 1) return;
  hipLaunchKernelGGL(triangulate_matches_kernel, dim3((t.capA + TRI_THREADS - 1) / TRI_THREADS, K), dim3(TRI_THREADS), 0, s, t);
}

void orbfe_launch_triangulate_count(const orbfe_new_point* out, const int32_t* nA, int nA_host, int capA, int32_t* n_new,
                                    const int32_t* counters, int counter_stride, int32_t* n_matches, int K, hipStream_t s) {
  if (K < 1) return;
  hipLaunchKernelGGL(triangulate_count_kernel, dim3(K), dim3(TRI_THREADS), 0, s, out, nA, nA_host, capA, n_new, counters, counter_stride,
                     n_matches);
}
