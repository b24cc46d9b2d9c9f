// bow_kernels.hip -- the searches over common vocabulary nodes, for gfx950 (MI355X, wave64).
// Kernel               replaces (reference file:line, L/ = Source/Libraries/ORB_SLAM2/)
// bow_match            SearchByBoW(KeyFrame*, Frame&) and SearchByBoW(KeyFrame*, KeyFrame*)    L/src/ORBmatcher.cc:161-273,494-612
// triangulation_match  SearchForTriangulation, with CheckDistEpipolarLine                     L/src/ORBmatcher.cc:614-764,137-159
// bow_finish           the rotation-consistency cut that ends both                            L/src/ORBmatcher.cc:255-270,594-609,737-761
// Compiled with -ffp-contract=off: every float expression is evaluated un-fused, as the reference does.
#include "search_device.h"   // WAVE, wave_min_u32, hamming256, load_desc, rot_bin, three_maxima

// SearchByBoW(KeyFrame*, Frame&, ...) (L/src/ORBmatcher.cc:161-273).  The host merge-joins the two FeatureVectors
// on NodeId; every common node is an independent problem (a feature belongs to exactly one node), so one wave
// takes one node: keyframe features in vIndicesKF order, the lanes share the node's frame features (best /
// second-best over those not matched yet, strict "<" in vIndicesF order), matches written immediately so that
// later keyframe features skip them (:208-209).  Rotation histogram by global atomics, finished by bow_finish.
__global__ __launch_bounds__(64) void bow_match_kernel(BowParams P) {
  extern __shared__ __attribute__((aligned(16))) uint8_t taken[];  // per frame feature of this node
  const int lane = threadIdx.x;
  // sequential mode (a frame feature listed under several nodes or, in the KF-KF form, a first-keyframe feature under several
  // common nodes -- never produced by DBoW2, but legal input; search_plan.h decides): one wave walks all node pairs in NodeId
  // order and reads the match table from memory, as the reference does
  const int first = P.sequential ? 0 : blockIdx.x, last = P.sequential ? P.n_pairs : blockIdx.x + 1;
  for (int pi = first; pi < last; pi++) {
  const BowPair pr = P.pairs[pi];
  __syncthreads();
  for (int i = lane; i < pr.countB; i += WAVE)
    taken[i] = (uint8_t)((P.sequential && __hip_atomic_load(&P.matchB[P.idxB[pr.startB + i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) ||
                         (P.validB && !P.validB[P.idxB[pr.startB + i]]));  // KF-KF: pMP2 missing or bad (:543-549)
  __syncthreads();
  for (int iKF = 0; iKF < pr.countA; iKF++) {
    const int realIdxKF = P.idxA[pr.startA + iKF];
    if (!P.validA[realIdxKF]) continue;  // no map point, or a bad one (:191-197)
    uint4 a0, a1;
    load_desc(P.descA + (size_t)realIdxKF * 32, a0, a1);
    int bestd = 256, bestj = -1, second = 256;
    for (int iF = lane; iF < pr.countB; iF += WAVE) {
      if (taken[iF]) continue;
      const int realIdxF = P.idxB[pr.startB + iF];
      uint4 b0, b1;
      load_desc(P.descB + (size_t)realIdxF * 32, b0, b1);
      const int d = hamming256(a0, a1, b0, b1);
      if (d < bestd) { second = bestd; bestd = d; bestj = iF; }
      else if (d < second) second = d;
    }
    // merge: first minimum in vIndicesF order, second = smallest of everything else
    const unsigned key = bestj >= 0 ? (((unsigned)bestd << 16) | (unsigned)bestj) : 0xFFFFFFFFu;
    const unsigned b = wave_min_u32(key);
    if (b != 0xFFFFFFFFu) {
      const unsigned other = (key == b) ? 0xFFFFFFFFu : key;
      int s2 = min(second, other != 0xFFFFFFFFu ? (int)(other >> 16) : 256);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) s2 = min(s2, __shfl_xor(s2, d, WAVE));
      const int bestDist1 = (int)(b >> 16), bestF = (int)(b & 0xffff);
      // KF-Frame accepts bestDist <= TH_LOW (:224), KF-KF only bestDist < TH_LOW (:564)
      if ((P.kf_mode ? bestDist1 < ORBFE_TH_LOW : bestDist1 <= ORBFE_TH_LOW) && (float)bestDist1 < P.nnratio * (float)s2) {
        if (lane == 0) {
          const int realIdxF = P.idxB[pr.startB + bestF];
          __hip_atomic_store(&P.matchB[realIdxF], realIdxKF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (P.kf_mode) P.matchA[realIdxKF] = realIdxF;
          taken[bestF] = 1;
          if (P.sequential)  // the same feature may be listed again inside this node
            for (int t = 0; t < pr.countB; t++)
              if (P.idxB[pr.startB + t] == realIdxF) taken[t] = 1;
          if (P.check_ori) {
            const int bin = rot_bin(P.angleA[realIdxKF], P.angleB[realIdxF]);
            const int pos = atomicAdd(&P.counters[0], 1);
            P.push_idx[pos] = P.kf_mode ? realIdxKF : realIdxF;  // rotHist holds idx1 in the KF-KF variant (:579)
            P.push_bin[pos] = (uint8_t)bin;
            atomicAdd(&P.counters[2 + bin], 1);
          }
          atomicAdd(&P.counters[1], 1);
        }
      }
    }
    __syncthreads();
  }
  }
}

// SearchForTriangulation (L/src/ORBmatcher.cc:614-764): one wave per common vocabulary node.  Nothing couples two features
// of pKF1 (vbMatched2 is never set), so each is an independent arg-min over the node's pKF2 features that pass the
// gates: dist <= TH_LOW, the epipole distance for two monocular keypoints (:697-703), CheckDistEpipolarLine (:137-159);
// `dist > bestDist` rejects, so of equal distances the LAST one in list order wins.
__global__ __launch_bounds__(64) void triangulation_match_kernel(TriParams T) {
  const BowParams& P = T.b;
  const int lane = threadIdx.x;
  const int first = P.sequential ? 0 : blockIdx.x, last = P.sequential ? P.n_pairs : blockIdx.x + 1;
  for (int pi = first; pi < last; pi++) {
    const BowPair pr = P.pairs[pi];
    for (int i1 = 0; i1 < pr.countA; i1++) {
      const int idx1 = P.idxA[pr.startA + i1];
      if (!P.validA[idx1]) continue;   // has a map point, or monocular under bOnlyStereo (:655-664)
      const bool bStereo1 = T.stereoA[idx1] != 0;
      const orbfe_keypoint kp1 = T.keysA[idx1];
      uint4 a0, a1;
      load_desc(P.descA + (size_t)idx1 * 32, a0, a1);
      // epipolar line in the second image l = x1' F12 = [a b c]
      const float* F = T.ep.F12;
      const float la = kp1.x * F[0] + kp1.y * F[3] + F[6];
      const float lb = kp1.x * F[1] + kp1.y * F[4] + F[7];
      const float lc = kp1.x * F[2] + kp1.y * F[5] + F[8];
      const float den = la * la + lb * lb;
      unsigned key = 0xFFFFFFFFu;   // dist << 16 | (0xffff - position): minimum = smallest distance, last position
      for (int i2 = lane; i2 < pr.countB; i2 += WAVE) {
        const int idx2 = P.idxB[pr.startB + i2];
        if (!P.validB[idx2]) continue;   // matched map point, or monocular under bOnlyStereo (:677-686)
        uint4 b0, b1;
        load_desc(P.descB + (size_t)idx2 * 32, b0, b1);
        const int dist = hamming256(a0, a1, b0, b1);
        if (dist > ORBFE_TH_LOW) continue;
        const orbfe_keypoint kp2 = T.keysB[idx2];
        if (!bStereo1 && !T.stereoB[idx2]) {
          const float distex = T.ep.ex - kp2.x, distey = T.ep.ey - kp2.y;
          if (distex * distex + distey * distey < 100 * T.ep.scale_factors[kp2.octave & (ORBFE_MAX_LEVELS - 1)]) continue;
        }
        const float num = la * kp2.x + lb * kp2.y + lc;
        if (den == 0) continue;
        const float dsqr = num * num / den;
        if (!((double)dsqr < 3.84 * (double)T.ep.level_sigma2[kp2.octave & (ORBFE_MAX_LEVELS - 1)])) continue;
        const unsigned k = ((unsigned)dist << 16) | (unsigned)(0xffff - i2);
        key = min(key, k);
      }
      const unsigned b = wave_min_u32(key);
      if (b != 0xFFFFFFFFu && lane == 0) {
        const int idx2 = P.idxB[pr.startB + (0xffff - (int)(b & 0xffff))];
        P.matchA[idx1] = idx2;
        atomicAdd(&P.counters[1], 1);
        if (P.check_ori) {
          const int bin = rot_bin(kp1.angle, T.keysB[idx2].angle);
          const int pos = atomicAdd(&P.counters[0], 1);
          P.push_idx[pos] = idx1;
          P.push_bin[pos] = (uint8_t)bin;
          atomicAdd(&P.counters[2 + bin], 1);
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void bow_finish_kernel(BowParams P) {
  __shared__ int top[3];
  __shared__ int removed;
  if (threadIdx.x == 0) {
    removed = 0;
    int i1, i2, i3;
    three_maxima(P.counters + 2, ORBFE_HISTO_LENGTH, i1, i2, i3);
    top[0] = i1; top[1] = i2; top[2] = i3;
  }
  __syncthreads();
  if (P.check_ori) {
    const int np = P.counters[0];
    int r = 0;
    for (int k = threadIdx.x; k < np; k += 256) {
      const int bin = P.push_bin[k];
      if (bin != top[0] && bin != top[1] && bin != top[2]) { (P.kf_mode ? P.matchA : P.matchB)[P.push_idx[k]] = -1; r++; }
    }
    if (r) atomicAdd(&removed, r);
  }
  __syncthreads();
  if (threadIdx.x == 0) P.counters[1] -= removed;
}

// ------------------------------------------------------------------------------------------------ launchers
void orbfe_launch_bow(const BowParams& p, int n_pairs, int max_countB, hipStream_t s) {
  if (n_pairs > 0)
    hipLaunchKernelGGL(bow_match_kernel, dim3(p.sequential ? 1 : n_pairs), dim3(64), (size_t)((max_countB + 15) & ~15), s, p);
  hipLaunchKernelGGL(bow_finish_kernel, dim3(1), dim3(256), 0, s, p);
}
void orbfe_launch_triangulation(const TriParams& p, int n_pairs, hipStream_t s) {
  if (n_pairs > 0) hipLaunchKernelGGL(triangulation_match_kernel, dim3(p.b.sequential ? 1 : n_pairs), dim3(64), 0, s, p);
  hipLaunchKernelGGL(bow_finish_kernel, dim3(1), dim3(256), 0, s, p.b);
}
