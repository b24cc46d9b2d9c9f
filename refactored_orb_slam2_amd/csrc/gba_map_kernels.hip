// gba_map_kernels.hip -- the map update behind the global bundle adjustment (L/src/LoopClosing.cc:648-703).  The arithmetic is
// gba_map_internal.h's; what is stated here is who does which keyframe or point and where the barriers are.
//
// The reference's breadth-first walk gives a keyframe that was not optimised the pose (Tcw * parent.Twc) * parent.mTcwGBA.  The bracket
// reads poses from before the walk only, so it is a function of the keyframe and its parent; the product is a function of the
// parent's NEW pose only.  Any schedule that computes a keyframe after its parent therefore gives the reference's bytes:
//   prepare   a lane per keyframe: an optimised one takes its row of gba_poses and SetPose's derivation; one with a parent leaves
//             Tchildc in the Tcw of its record, marked GM_PENDING; every other one is unreached and keeps its old pose
//   chain     ONE workgroup: a done-mark per keyframe in LDS (a bit; the optimised ones to begin with), a lane's pending keyframes in
//             a 64-bit mask in registers.  A round: every pending keyframe whose parent's mark is set multiplies Tchildc by the
//             parent's pose and stores its own; a barrier; the marks of the round are set; a barrier.  A mark is set only behind the
//             barrier that ends the round it was earned in, so a round reads the marks and the poses of earlier rounds only, and the
//             round count is the depth of the deepest propagated keyframe.  The loop ends with the first round that sets no mark.
//             What is still pending then -- a cycle, a chain under an unreached keyframe -- is unreached
//   finish    a lane per keyframe: SetPose's derivation of a propagated pose, the old pose for what stayed pending; the counts
//   points    a lane per point: gba_points, the move with the reference keyframe's record, or the point as it is; the counts
// The counts reach the result record by integer atomics, one per workgroup and field.  No floating-point atomics.
#include "gba_map_internal.h"

__device__ inline void gm_load12(const float* p, float* T) {
#pragma unroll
  for (int i = 0; i < 12; i++) T[i] = p[i];
}
__device__ inline void gm_store12(float* p, const float* T) {
#pragma unroll
  for (int i = 0; i < 12; i++) p[i] = T[i];
}

// the old pose with its SetPose derivation, for an unreached keyframe
__device__ inline void gm_write_record(orbfe_gba_map_keyframe& rec, const float* Tcw, float half_baseline, int status) {
  float Twc[12], Cw[3];
  gm_set_pose(Tcw, half_baseline, Twc, Cw);
  gm_store12(rec.Tcw, Tcw);
  gm_store12(rec.Twc, Twc);
  rec.Cw[0] = Cw[0];
  rec.Cw[1] = Cw[1];
  rec.Cw[2] = Cw[2];
  rec.status = status;
}

__global__ __launch_bounds__(256) void gba_map_prepare_kernel(GmLaunch L) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= L.n_kf) return;
  const int row = L.kf_gba_row[k], par = L.parent[k];
  float T[12];
  orbfe_gba_map_keyframe& rec = L.kf_out[k];
  if (row >= 0 && row < L.n_gba_kf) {
    gm_load12(L.gba_poses + 12 * (size_t)row, T);
    gm_write_record(rec, T, L.half_baseline, ORBFE_GBA_MAP_KF_OPTIMISED);
    return;
  }
  gm_load12(L.poses + 12 * (size_t)k, T);
  if (row < 0 && par >= 0 && par < L.n_kf) {
    float P[12], Tchildc[12];
    gm_load12(L.poses + 12 * (size_t)par, P);
    gm_relative(T, P, L.half_baseline, Tchildc);
    gm_store12(rec.Tcw, Tchildc);
    rec.status = GM_PENDING;
    return;
  }
  gm_write_record(rec, T, L.half_baseline, ORBFE_GBA_MAP_KF_UNREACHED);
}

__global__ __launch_bounds__(GM_CHAIN_THREADS) void gba_map_chain_kernel(GmLaunch L) {
  __shared__ uint32_t done[ORBFE_GBA_MAP_MAX_KEYFRAMES / 32];
  const int tid = threadIdx.x, n = L.n_kf;
  for (int w = tid; w < ORBFE_GBA_MAP_MAX_KEYFRAMES / 32; w += GM_CHAIN_THREADS) done[w] = 0;
  __syncthreads();
  uint64_t pending = 0;
  for (int j = 0, k = tid; k < n; j++, k += GM_CHAIN_THREADS) {
    const int st = L.kf_out[k].status;
    if (st == ORBFE_GBA_MAP_KF_OPTIMISED) atomicOr(&done[k >> 5], 1u << (k & 31));
    if (st == GM_PENDING) pending |= (uint64_t)1 << j;
  }
  __syncthreads();
  int rounds = 0;
  for (;;) {
    uint64_t earned = 0;
    for (uint64_t m = pending; m; m &= m - 1) {
      const int j = __ffsll((unsigned long long)m) - 1;
      const int k = tid + j * GM_CHAIN_THREADS;
      const int par = L.parent[k];   // in 0 .. n_kf - 1: the prepare kernel marks nothing else pending
      if (!((done[par >> 5] >> (par & 31)) & 1u)) continue;
      float Tchildc[12], P[12], T[12];
      gm_load12(L.kf_out[k].Tcw, Tchildc);
      gm_load12(L.kf_out[par].Tcw, P);
      gm_propagate(Tchildc, P, T);
      gm_store12(L.kf_out[k].Tcw, T);
      L.kf_out[k].status = ORBFE_GBA_MAP_KF_PROPAGATED;
      earned |= (uint64_t)1 << j;
    }
    if (!__syncthreads_or(earned != 0)) break;   // also: the poses of this round are written before the next one reads them
    for (uint64_t m = earned; m; m &= m - 1) {
      const int k = tid + (__ffsll((unsigned long long)m) - 1) * GM_CHAIN_THREADS;
      atomicOr(&done[k >> 5], 1u << (k & 31));
    }
    pending &= ~earned;
    rounds++;
    __syncthreads();
  }
  if (tid == 0) L.result->rounds = rounds;
}

// adds a workgroup's counts to the result record: c[i] of every lane into field[i]
template <int N>
__device__ inline void gm_count(int32_t* field, const int (&c)[N], int* sh) {
  if (threadIdx.x < N) sh[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; i++)
    if (c[i]) atomicAdd(&sh[i], c[i]);
  __syncthreads();
  if (threadIdx.x < N && sh[threadIdx.x]) atomicAdd(&field[threadIdx.x], sh[threadIdx.x]);
}

__global__ __launch_bounds__(256) void gba_map_finish_kernel(GmLaunch L) {
  __shared__ int sh[3];
  const int k = blockIdx.x * 256 + threadIdx.x;
  int c[3] = {0, 0, 0};
  if (k < L.n_kf) {
    orbfe_gba_map_keyframe& rec = L.kf_out[k];
    int st = rec.status;
    float T[12];
    if (st == ORBFE_GBA_MAP_KF_PROPAGATED) {
      gm_load12(rec.Tcw, T);
      gm_write_record(rec, T, L.half_baseline, st);
    } else if (st == GM_PENDING) {
      st = ORBFE_GBA_MAP_KF_UNREACHED;
      gm_load12(L.poses + 12 * (size_t)k, T);
      gm_write_record(rec, T, L.half_baseline, st);
    }
    c[0] = st == ORBFE_GBA_MAP_KF_OPTIMISED;
    c[1] = st == ORBFE_GBA_MAP_KF_PROPAGATED;
    c[2] = st == ORBFE_GBA_MAP_KF_UNREACHED;
  }
  gm_count(&L.result->n_optimised, c, sh);
}

// One thread per point, any grid size
__global__ __launch_bounds__(256) void gba_map_points_kernel(GmLaunch L) {
  __shared__ int sh[3];
  int c[3] = {0, 0, 0};
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)L.n_points; p += (size_t)gridDim.x * 256) {
    const float* X = reinterpret_cast<const float*>(L.points + p * (size_t)L.point_stride);
    float o[3] = {X[0], X[1], X[2]};
    const int row = L.point_gba_row[p], r = L.ref[p];
    if (row >= 0) {
      if (row < L.n_gba_points) {
        o[0] = L.gba_points[3 * (size_t)row];
        o[1] = L.gba_points[3 * (size_t)row + 1];
        o[2] = L.gba_points[3 * (size_t)row + 2];
        c[0]++;
      } else {
        c[2]++;
      }
    } else if (r >= 0 && r < L.n_kf && L.kf_out[r].status != ORBFE_GBA_MAP_KF_UNREACHED) {
      float Tbef[12], Twc[12];
      const float Xw[3] = {o[0], o[1], o[2]};
      gm_load12(L.poses + 12 * (size_t)r, Tbef);
      gm_load12(L.kf_out[r].Twc, Twc);
      gm_move_point(Tbef, Twc, Xw, o);
      c[1]++;
    } else {
      c[2]++;
    }
    L.points_out[3 * p] = o[0];
    L.points_out[3 * p + 1] = o[1];
    L.points_out[3 * p + 2] = o[2];
  }
  gm_count(&L.result->n_taken, c, sh);
}

void orbfe_launch_gba_map(const GmLaunch& L, hipStream_t s) {
  if (L.n_kf > 0) {
    const int blocks = (L.n_kf + 255) / 256;
    hipLaunchKernelGGL(gba_map_prepare_kernel, dim3(blocks), dim3(256), 0, s, L);
    hipLaunchKernelGGL(gba_map_chain_kernel, dim3(1), dim3(GM_CHAIN_THREADS), 0, s, L);
    hipLaunchKernelGGL(gba_map_finish_kernel, dim3(blocks), dim3(256), 0, s, L);
  }
  if (L.n_points > 0) {
    const int blocks = (L.n_points + 255) / 256;
    hipLaunchKernelGGL(gba_map_points_kernel, dim3(blocks < 65535 ? blocks : 65535), dim3(256), 0, s, L);
  }
}
