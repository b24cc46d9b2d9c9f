// fuse_kernels.hip -- the row search of a resident fuse batch for gfx950 (MI355X, wave64): every ORBmatcher::Fuse call of
// LocalMapping::SearchInNeighbors (L/src/LocalMapping.cc:425-509, L/src/ORBmatcher.cc:766-907; Fuse with Sim3 :909-1027) in one launch.
//
// Row (k, i) is what orbfe_kf_search computes for point i in target k: kf_project (the prologue kf_queries_kernel runs) and then
// enumerate_window on target k's grid with the first-minimum rule of proj_best_kernel -- both stated once, in search_device.h, so a row is
// those kernels' bytes.  The 96-byte query that route writes to HBM per row and reads back never exists here: the point's 72-byte
// record is read from the one shared table and its query stays in registers.
//
// Lanes per row.  The prologue is one LANE per row (the target's camera record and 1/sigma2 table in LDS: a by-value record indexed
// with the per-lane level would live in scratch memory, DESIGN lesson 58).  The rows that pass it are then walked one at a time by the
// whole WAVE, the query broadcast from its lane with readlane -- enumerate_window as it stands, so the enumeration order cannot
// differ from the single call's.  A wave per row from the start would run the prologue 64 times over for every row, the rejected ones
// included.  A walk is three dependent round trips (cell ranges, cell records, descriptors), and a wave makes its walks one after
// the other: FUSE_WAVE_ROWS rows per wave set the length of that chain.  With 64 (every lane a row) the full search of 30 targets x
// 1 000 points is 120 workgroups and 90 us, each wave walking ~60 rows in a row on a mostly empty device; with 8 it is 21 us, and
// 4 .. 32 are measured in profiles/search_in_neighbors.md.
#include <hip/hip_runtime.h>

#include "fuse_internal.h"
#include "search_device.h"

static_assert(sizeof(orbfe_kf_camera) == 220 && sizeof(orbfe_kf_point) == 72 && sizeof(orbfe_kf_result) == 24, "record layout");

#define FUSE_THREADS 256     // four waves per workgroup, all on one target
#ifndef FUSE_WAVE_ROWS
#define FUSE_WAVE_ROWS 8     // rows per wave: a wave walks its surviving rows one after the other, three dependent round trips each
#endif
#define FUSE_ROWS (FUSE_WAVE_ROWS * (FUSE_THREADS / WAVE))   // rows per workgroup

__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ unsigned lane_u(unsigned v, int l) { return (unsigned)__builtin_amdgcn_readlane((int)v, l); }

template <int GATE>   // 2: Fuse's chi-square gate, 1: none (Fuse with Sim3)
__global__ __launch_bounds__(FUSE_THREADS) void fuse_rows_kernel(FuseRows A, int blocks_per_target) {
  __shared__ orbfe_kf_camera cam;
  __shared__ float s_inv[ORBFE_MAX_LEVELS];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int k = A.first_target + (int)(blockIdx.x / (unsigned)blocks_per_target);
  // row slot of this lane: FUSE_WAVE_ROWS rows per wave, on its first lanes (the others only help with the walk)
  const int slot = ((int)(blockIdx.x % (unsigned)blocks_per_target) * (FUSE_THREADS / WAVE) + (tid >> 6)) * FUSE_WAVE_ROWS + lane;
  const int j = lane < FUSE_WAVE_ROWS ? slot : A.n_rows;
  if (tid < (int)(sizeof(orbfe_kf_camera) / 4))
    reinterpret_cast<uint32_t*>(&cam)[tid] = reinterpret_cast<const uint32_t*>(A.cams + k)[tid];
  __syncthreads();
  if (tid < ORBFE_MAX_LEVELS)   // zero beyond the target's levels, as the single call's staging leaves it
    s_inv[tid] = (A.inv_sigma2 && tid < cam.n_levels) ? A.inv_sigma2[(size_t)k * ORBFE_MAX_LEVELS + tid] : 0.f;
  __syncthreads();

  FrameBatch F = A.F;   // the grid geometry of target k, where the targets' image bounds differ
  if (A.geo) {
    const float4 g = reinterpret_cast<const float4*>(A.geo)[k];
    F.min_x = g.x; F.min_y = g.y; F.gw_inv = g.z; F.gh_inv = g.w;
  }
  orbfe_query q;
  uint32_t* qw = reinterpret_cast<uint32_t*>(&q);
#pragma unroll
  for (int w = 0; w < (int)(sizeof(orbfe_query) / 4); w++) qw[w] = 0u;
  orbfe_kf_result res;
  res.best_idx = -1; res.best_dist = 256; res.level = -1; res.u = 0.f; res.v = 0.f; res.u_r = 0.f;
  int i = -1;
  if (j < A.n_rows) i = A.point_idx ? A.point_idx[j] : j;
  const bool live = i >= 0 && i < A.n_points;
  if (live) {
    orbfe_kf_point mp = A.points[i];
    if (A.skip && A.skip[(size_t)k * A.n_points + i]) mp.skip = 1;
    kf_project(cam, mp, A.mode, q, res);
  }
  // the surviving rows of this wave, one at a time on all 64 lanes (no lane has left: the DPP reductions need the whole wave)
  unsigned long long todo = __ballot(q.valid != 0);
  const uint32_t* dw = reinterpret_cast<const uint32_t*>(q.desc);
  while (todo) {
    const int L = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    orbfe_query w;   // wave-uniform copy of lane L's query: what enumerate_window reads of it
    w.u = lane_f(q.u, L); w.v = lane_f(q.v, L); w.u_r = lane_f(q.u_r, L); w.radius = lane_f(q.radius, L);
    w.min_level = __builtin_amdgcn_readlane(q.min_level, L);
    w.max_level = __builtin_amdgcn_readlane(q.max_level, L);
    const uint4 q0 = make_uint4(lane_u(dw[0], L), lane_u(dw[1], L), lane_u(dw[2], L), lane_u(dw[3], L));
    const uint4 q1 = make_uint4(lane_u(dw[4], L), lane_u(dw[5], L), lane_u(dw[6], L), lane_u(dw[7], L));
    unsigned key = 0xFFFFFFFFu;
    int mine = -1;
    enumerate_window<GATE>(F, k, w, q0, q1, [&](int rank, int idx, int dist, int) {
      const unsigned kk = ((unsigned)dist << 16) | (unsigned)min(rank, 0xffff);
      if (kk < key) { key = kk; mine = idx; }
    }, s_inv);
    const unsigned b = wave_min_u32(key);   // first minimum in GetFeaturesInArea order: strict `dist < bestDist`
    int bi = -1;
    if (b != 0xFFFFFFFFu) {
      const unsigned long long wm = __ballot(key == b);
      bi = __builtin_amdgcn_readlane(mine, __ffsll((long long)wm) - 1);
    }
    if (lane == L) {
      res.best_idx = bi;
      res.best_dist = bi >= 0 ? (int)(b >> 16) : 256;
    }
  }
  if (live) A.out[(size_t)(k - A.out_first) * A.out_stride + (A.out_by_list ? j : i)] = res;
}

__global__ __launch_bounds__(256) void fuse_scatter_kernel(orbfe_kf_point* __restrict__ table, int n_points,
                                                           const orbfe_kf_point* __restrict__ records, const int32_t* __restrict__ idx, int n) {
  constexpr int DW = (int)(sizeof(orbfe_kf_point) / 4);
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int j = t / DW, w = t % DW;
  if (j >= n) return;
  const int i = idx[j];
  if (i < 0 || i >= n_points) return;
  reinterpret_cast<uint32_t*>(table + i)[w] = reinterpret_cast<const uint32_t*>(records + j)[w];
}

void orbfe_launch_fuse_rows(const FuseRows& a, hipStream_t s) {
  const int n_t = a.n_targets - a.first_target;
  if (n_t < 1 || a.n_rows < 1) return;
  const int bpt = (a.n_rows + FUSE_ROWS - 1) / FUSE_ROWS;
  const dim3 grid((unsigned)((size_t)n_t * (size_t)bpt));   // <= K * n_points, which the host keeps within int32
  if (a.mode == ORBFE_KF_FUSE) hipLaunchKernelGGL(fuse_rows_kernel<2>, grid, dim3(FUSE_THREADS), 0, s, a, bpt);
  else hipLaunchKernelGGL(fuse_rows_kernel<1>, grid, dim3(FUSE_THREADS), 0, s, a, bpt);
}

void orbfe_launch_fuse_scatter(orbfe_kf_point* table, int n_points, const orbfe_kf_point* records, const int32_t* idx, int n, hipStream_t s) {
  if (n < 1) return;
  const size_t threads = (size_t)n * (sizeof(orbfe_kf_point) / 4);
  hipLaunchKernelGGL(fuse_scatter_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, table, n_points, records, idx, n);
}
