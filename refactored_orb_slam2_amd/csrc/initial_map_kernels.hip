// initial_map_kernels.hip -- Tracking::CreateInitialMapMonocular (L/src/Tracking.cc:546-666) for a batch of problems, from what
// Initializer::Initialize left in device memory to a scaled map: three launches on one stream, one workgroup of 256 threads per
// problem in each.  The arithmetic is initial_map_internal.h's, one item per call; the adjustment in the middle is ba_kernels.hip.
//   imap_build_kernel    a lane per keypoint of frame 1: the word of 64 verdicts "this match becomes a point" is one wave's ballot; the
//                        place of a point is the popcount prefix over the words (at most 64 of them) plus the popcount of the bits
//                        below its own; the lane writes the index entry, the point and its two edges, all in order of i
//   ba_kernel            Optimizer::BundleAdjustment on the problems the build wrote: 2 keyframes, the first fixed
//   imap_finish_kernel   a lane per point: its depth in the initial keyframe as an ordered key in LDS (at most 4 096, 16 KB); the
//                        order statistic by 32 counting passes over the keys, one per bit of the key; the keypoints of frame 2 that
//                        hold a point by letting every point sign its keypoint's slot in LDS (whoever wins, one signature stands per
//                        keypoint) and counting the signatures that stand; the reset rule; the rescale
// No atomics; every count is lm_reduce_count's, so a problem's bytes depend on its own rows only.
#include "initial_map_internal.h"
#include "lm_reduce.h"

#define IMAP_THREADS 256
#define IMAP_WAVES (IMAP_THREADS / 64)
#define IMAP_WORDS (ORBFE_INIT_MAX_MATCHES / 64)
static_assert(sizeof(orbfe_initial_map_result) == 72 && sizeof(orbfe_ba_result) == 40, "record layout");

__device__ __forceinline__ int imap_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(IMAP_THREADS) void imap_build_kernel(ImapLaunch L) {
  __shared__ unsigned long long words[IMAP_WORDS];
  __shared__ int prefix[IMAP_WORDS + 1];
  const int p = blockIdx.x, tid = threadIdx.x, cap = L.cap, W = (cap + 63) >> 6;
  const int n1 = imap_clamp(L.n1[p], cap), n2 = imap_clamp(L.n2[p], cap), n1_words = (n1 + 63) >> 6;
  const int32_t* matches = L.matches12 + (size_t)p * cap;
  const uint64_t* tri = L.triangulated + (size_t)p * W;
  for (int i = tid; i < n1_words * 64; i += IMAP_THREADS) {   // a wave per word: i >> 6 is uniform over the wave
    const bool is = i < n1 && imap_is_point(matches[i], n2, tri[i >> 6], i & 63);
    const unsigned long long b = __ballot(is);
    if ((tid & 63) == 0) words[i >> 6] = b;
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int w = 0; w < n1_words; w++) {
      prefix[w] = o;
      o += __popcll(words[w]);
    }
    prefix[n1_words] = o;
  }
  __syncthreads();
  const int n = prefix[n1_words];
  const orbfe_pose_camera& cam = *L.camera;   // read where it lies: a copy indexed by an octave would live in scratch memory
  const float* keys1 = L.keys1 + (size_t)p * cap * 2;
  const float* keys2 = L.keys2 + (size_t)p * cap * 2;
  const float* P3D = L.P3D + (size_t)p * cap * 3;
  const int32_t* oct1 = L.octaves1 + (size_t)p * cap;
  const int32_t* oct2 = L.octaves2 + (size_t)p * cap;
  int32_t* index = L.index + (size_t)p * cap;
  float* pts = L.ba_points + (size_t)p * cap * 3;
  orbfe_lba_edge* edges = L.ba_edges + (size_t)p * cap * 2;
  for (int i = tid; i < n1; i += IMAP_THREADS) {
    const unsigned long long w = words[i >> 6];
    if (!((w >> (i & 63)) & 1ull)) continue;
    const int j = prefix[i >> 6] + __popcll(w & ((1ull << (i & 63)) - 1ull));
    const int32_t m = matches[i];
    index[j] = i;
    pts[3 * j] = P3D[3 * i];
    pts[3 * j + 1] = P3D[3 * i + 1];
    pts[3 * j + 2] = P3D[3 * i + 2];
    imap_edges(cam, j, keys1 + 2 * i, oct1[i], keys2 + 2 * m, oct2[m], edges + 2 * j);
  }
  for (int j = n + tid; j < n1; j += IMAP_THREADS) index[j] = -1;
  if (tid == 0) {
    const orbfe_init_result& r = L.init[p];
    imap_poses(L.pose1 ? L.pose1 + (size_t)p * 12 : nullptr, r.R21, r.t21, L.ba_poses + (size_t)p * 24);
    L.ba_fixed[2 * p] = 1;
    L.ba_fixed[2 * p + 1] = 0;
    orbfe_lba_problem Q;
    Q.kf_offset = 2 * p; Q.n_kf = 2;
    Q.point_offset = p * cap; Q.n_points = n;
    Q.edge_offset = 2 * p * cap; Q.n_edges = 2 * n;
    L.problems[p] = Q;
  }
}

__global__ __launch_bounds__(IMAP_THREADS) void imap_finish_kernel(ImapLaunch L) {
  __shared__ uint32_t keys[ORBFE_INIT_MAX_MATCHES];
  __shared__ int owner[ORBFE_INIT_MAX_MATCHES];
  __shared__ int red_i[IMAP_WAVES];
  const int p = blockIdx.x, tid = threadIdx.x, cap = L.cap, W = (cap + 63) >> 6;
  const int n1 = imap_clamp(L.n1[p], cap), n2 = imap_clamp(L.n2[p], cap);
  const int n = L.problems[p].n_points;   // <= n1
  const orbfe_ba_result* ba = L.ba_result + p;
  const int32_t* matches = L.matches12 + (size_t)p * cap;
  const uint64_t* tri = L.triangulated + (size_t)p * W;
  const int32_t* index = L.index + (size_t)p * cap;
  const float* T = L.ba_poses_out + (size_t)p * 24;
  const float* X = L.ba_points_out + (size_t)p * cap * 3;
  for (int j = tid; j < n; j += IMAP_THREADS) {
    keys[j] = imap_depth_key(imap_depth(T, X + 3 * j));
    owner[matches[index[j]]] = j;   // plain stores: one of the points of a keypoint stands there afterwards
  }
  __syncthreads();
  int mine = 0;
  for (int j = tid; j < n; j += IMAP_THREADS) mine += owner[matches[index[j]]] == j ? 1 : 0;
  const int tracked = lm_reduce_count<IMAP_WAVES>(mine, red_i, tid);
  // vDepths[(size - 1) / q] of the sorted depths: the largest key K with fewer than rank + 1 keys below it, found bit by bit
  const int rank = n > 0 ? (n - 1) / L.q : 0;
  uint32_t K = 0;
  for (int bit = 31; bit >= 0; bit--) {
    const uint32_t t = K | (1u << bit);
    int c = 0;
    for (int j = tid; j < n; j += IMAP_THREADS) c += keys[j] < t ? 1 : 0;
    c = lm_reduce_count<IMAP_WAVES>(c, red_i, tid);
    if (c <= rank) K = t;   // uniform
  }
  const float median = n > 0 ? imap_key_depth(K) : 0.0f;
  const int reason = imap_reason(n, median, tracked, L.min_points, ba->rounds);
  const float inv = imap_inv_median(median);
  const bool scale = reason == 0;

  float* poses = L.poses + (size_t)p * 24;
  float* points = L.points + (size_t)p * cap * 3;
  float* poses_ba = L.poses_ba ? L.poses_ba + (size_t)p * 24 : nullptr;
  float* points_ba = L.points_ba ? L.points_ba + (size_t)p * cap * 3 : nullptr;
  if (tid < 24) {
    const float v = T[tid];
    if (poses_ba) poses_ba[tid] = v;
    poses[tid] = (scale && tid >= 12 && (tid & 3) == 3) ? imap_scaled(v, inv) : v;
  }
  for (int i = tid; i < n1; i += IMAP_THREADS) {   // the rows without a point; the others are the scatter's below
    if (imap_is_point(matches[i], n2, tri[i >> 6], i & 63)) continue;
    for (int c = 0; c < 3; c++) {
      points[3 * i + c] = 0.0f;
      if (points_ba) points_ba[3 * i + c] = 0.0f;
    }
  }
  for (int j = tid; j < n; j += IMAP_THREADS) {
    const int i = index[j];
    for (int c = 0; c < 3; c++) {
      const float v = X[3 * j + c];
      if (points_ba) points_ba[3 * i + c] = v;
      points[3 * i + c] = scale ? imap_scaled(v, inv) : v;
    }
  }
  if (tid == 0) {
    orbfe_initial_map_result& r = L.result[p];
    r.n_points = n;
    r.tracked = tracked;
    r.median_depth = median;
    r.success = scale ? 1 : 0;
    r.reason = reason;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    r.ba.rounds = ba->rounds; r.ba.n_free = ba->n_free; r.ba.n_edges = ba->n_edges; r.ba.iterations = ba->iterations;
    r.ba.trials = ba->trials; r.ba.reserved = 0; r.ba.chi2_first = ba->chi2_first; r.ba.chi2_final = ba->chi2_final;
  }
}

void orbfe_launch_initial_map(const ImapLaunch& L, int P, hipStream_t s) {
  if (P < 1) return;
  hipLaunchKernelGGL(imap_build_kernel, dim3(P), dim3(IMAP_THREADS), 0, s, L);
  LbaLaunch B;
  memset(&B, 0, sizeof(B));
  B.camera = L.camera; B.problems = L.problems; B.poses = L.ba_poses; B.fixed = L.ba_fixed; B.points = (const uint8_t*)L.ba_points;
  B.point_stride = 12; B.edges = L.ba_edges; B.kf_cap = 2; B.point_cap = L.cap; B.edge_cap = 2 * L.cap; B.flags = ORBFE_BA_ROBUST;
  B.poses_out = L.ba_poses_out; B.points_out = L.ba_points_out; B.workspace = L.lba_workspace;
  orbfe_launch_ba(B, L.n_iterations, L.ba_result, P, s);
  hipLaunchKernelGGL(imap_finish_kernel, dim3(P), dim3(IMAP_THREADS), 0, s, L);
}
