// grid_kernels.hip -- the 64x48 keypoint grid of a frame in CSR form, for gfx950 (MI355X, wave64).
// Kernel              replaces (reference file:line, L/ = Source/Libraries/ORB_SLAM2/)
// grid_build          Frame::AssignFeaturesToGrid + PosInGrid                 L/src/Frame.cc:250-263,399-410
// grid_build_global   the same beyond GB_LDS_CAP keypoints, lists sorted in HBM   L/src/Frame.cc:250-263,399-410
// Compiled with -ffp-contract=off: every float expression is evaluated un-fused, as the reference does.
#include "search_device.h"   // the wave scan, cell_rec_pack

// One block per frame; cell = ix*48 + iy (Frame::PosInGrid, -1 outside the grid there), lists in ascending keypoint index.
#define GB_THREADS 1024   // one block per frame and one frame per CU: the block's own parallelism is all there is to hide latency with
#define GB_LDS_CAP 20000  // frames up to this capacity keep the per-keypoint state in LDS (6 bytes per keypoint)
// Exclusive scan of the kernel's cnt[] into start[] (L/src/Frame.cc:250-263 as offsets): CPT cells per thread, DPP wave scan, wave totals
// through tmp[]; uses tid and CPT.  A macro, and the cell of a keypoint written out at its three sites: as __forceinline__ functions (arrays
// by pointer, reference or LDS-typed pointer; the cell as a bool or a -1 sentinel) both changed the generated code of both kernels.
#define GRID_SCAN_CELLS() \
  { \
    int local = 0; \
    _Pragma("unroll") \
    for (int k = 0; k < CPT; k++) local += cnt[tid * CPT + k]; \
    const int v = wave_incl_scan_i(local); \
    if ((tid & 63) == 63) tmp[tid >> 6] = v; \
    __syncthreads(); \
    int off = 0; \
    for (int w = 0; w < (tid >> 6); w++) off += tmp[w]; \
    int run = off + v - local; \
    _Pragma("unroll") \
    for (int k = 0; k < CPT; k++) { \
      start[tid * CPT + k] = run; \
      run += cnt[tid * CPT + k]; \
    } \
    if (tid == GB_THREADS - 1) start[GRID_CELLS] = run; \
  }
// LDS-resident form: two global round trips (keypoints in, records out) instead of nine.  A keypoint's place inside its cell is
// its RANK among the cell's indices (cells hold a handful of keypoints), computed by the thread that owns the keypoint -- no sort,
// and the 16-byte record is written from the owner's registers instead of through the index -> keypoint -> mvuRight chain.
__global__ __launch_bounds__(GB_THREADS) void grid_build_kernel(FrameBatch F) {
  __shared__ int cnt[GRID_CELLS];
  __shared__ int start[GRID_CELLS + 1];
  __shared__ int tmp[GB_THREADS / 64];
  extern __shared__ __attribute__((aligned(16))) uint8_t gdyn[];
  static_assert(GRID_CELLS % GB_THREADS == 0 && GRID_CELLS <= 4096, "cells per thread; the cell id travels in 12 bits");
  constexpr int CPT = GRID_CELLS / GB_THREADS;   // consecutive cells per thread in the scan
  uint32_t* cellslot = reinterpret_cast<uint32_t*>(gdyn);            // per keypoint: cell | arrival slot << 12 (~0u: outside the grid)
  uint16_t* list = reinterpret_cast<uint16_t*>(cellslot + F.cap);    // per CSR entry: keypoint index, arrival order inside a cell
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = F.n[f];
  const orbfe_keypoint* keys = F.keys + (size_t)f * F.cap;
  const float* ur = F.u_right ? F.u_right + (size_t)f * F.cap : nullptr;
  int32_t* cs = F.cell_start + (size_t)f * (GRID_CELLS + 1);
  int32_t* ci = F.cell_idx + (size_t)f * F.cap;
  uint4* cr = reinterpret_cast<uint4*>(F.cell_rec) + (size_t)f * F.cap;
  for (int c = tid; c < GRID_CELLS; c += GB_THREADS) cnt[c] = 0;
  __syncthreads();
  for (int i0 = tid; i0 < n; i0 += 2 * GB_THREADS) {   // two keypoints per thread and round trip
    const int i1 = i0 + GB_THREADS;
    const float x0 = keys[i0].x, y0 = keys[i0].y;
    float x1 = 0.f, y1 = 0.f;
    if (i1 < n) { x1 = keys[i1].x; y1 = keys[i1].y; }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int i = k ? i1 : i0;
      if (i >= n) break;
      const int px = (int)roundf(((k ? x1 : x0) - F.min_x) * F.gw_inv);
      const int py = (int)roundf(((k ? y1 : y0) - F.min_y) * F.gh_inv);
      uint32_t v = ~0u;
      if (px >= 0 && px < ORBFE_GRID_COLS && py >= 0 && py < ORBFE_GRID_ROWS) {
        const int c = px * ORBFE_GRID_ROWS + py;
        v = (uint32_t)c | ((uint32_t)atomicAdd(&cnt[c], 1) << 12);
      }
      cellslot[i] = v;
    }
  }
  __syncthreads();
  GRID_SCAN_CELLS();
  __syncthreads();
  for (int c = tid; c <= GRID_CELLS; c += GB_THREADS) cs[c] = start[c];
  for (int i = tid; i < n; i += GB_THREADS) {
    const uint32_t v = cellslot[i];
    if (v != ~0u) list[start[v & 0xfffu] + (int)(v >> 12)] = (uint16_t)i;
  }
  __syncthreads();
  for (int i0 = tid; i0 < n; i0 += 2 * GB_THREADS) {
    const int i1 = i0 + GB_THREADS;
    const orbfe_keypoint k0 = keys[i0];
    const float u0 = ur ? ur[i0] : -1.0f;
    orbfe_keypoint k1 = k0;
    float u1 = -1.0f;
    if (i1 < n) { k1 = keys[i1]; u1 = ur ? ur[i1] : -1.0f; }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int i = k ? i1 : i0;
      if (i >= n) break;
      const uint32_t v = cellslot[i];
      if (v == ~0u) continue;
      const int c = (int)(v & 0xfffu);
      const int s0 = start[c], s1 = start[c + 1];
      int pos = s0;
      for (int j = s0; j < s1; j++) pos += (int)list[j] < i;   // insertion order of the reference = ascending index
      const orbfe_keypoint& kp = k ? k1 : k0;
      ci[pos] = i;
      cr[pos] = cell_rec_pack(i, kp.octave, kp.x, kp.y, k ? u1 : u0);
    }
  }
}

__global__ __launch_bounds__(GB_THREADS) void grid_build_global_kernel(FrameBatch F) {
  __shared__ int cnt[GRID_CELLS];
  __shared__ int start[GRID_CELLS + 1];
  __shared__ int tmp[GB_THREADS / 64];
  static_assert(GRID_CELLS % GB_THREADS == 0, "cells per thread");
  constexpr int CPT = GRID_CELLS / GB_THREADS;   // consecutive cells per thread in the scan
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = F.n[f];
  const orbfe_keypoint* keys = F.keys + (size_t)f * F.cap;
  int32_t* cs = F.cell_start + (size_t)f * (GRID_CELLS + 1);
  int32_t* ci = F.cell_idx + (size_t)f * F.cap;
  for (int c = tid; c < GRID_CELLS; c += GB_THREADS) cnt[c] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += GB_THREADS) {
    const int px = (int)roundf((keys[i].x - F.min_x) * F.gw_inv);
    const int py = (int)roundf((keys[i].y - F.min_y) * F.gh_inv);
    if (px >= 0 && px < ORBFE_GRID_COLS && py >= 0 && py < ORBFE_GRID_ROWS) atomicAdd(&cnt[px * ORBFE_GRID_ROWS + py], 1);
  }
  __syncthreads();
  GRID_SCAN_CELLS();
  __syncthreads();
  for (int c = tid; c <= GRID_CELLS; c += GB_THREADS) cs[c] = start[c];
  for (int c = tid; c < GRID_CELLS; c += GB_THREADS) cnt[c] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += GB_THREADS) {
    const int px = (int)roundf((keys[i].x - F.min_x) * F.gw_inv);
    const int py = (int)roundf((keys[i].y - F.min_y) * F.gh_inv);
    if (px >= 0 && px < ORBFE_GRID_COLS && py >= 0 && py < ORBFE_GRID_ROWS) {
      const int c = px * ORBFE_GRID_ROWS + py;
      ci[start[c] + atomicAdd(&cnt[c], 1)] = i;
    }
  }
  __syncthreads();
  // insertion order of the reference = ascending index: sort each (tiny) cell list
  for (int c = tid; c < GRID_CELLS; c += GB_THREADS) {
    const int s = start[c], e = start[c + 1];
    for (int i = s + 1; i < e; i++) {
      const int v = ci[i];
      int j = i - 1;
      while (j >= s && ci[j] > v) { ci[j + 1] = ci[j]; j--; }
      ci[j + 1] = v;
    }
  }
  __syncthreads();
  // everything a window walk tests per entry, in CSR order: one 16-byte record instead of the index -> keypoint -> mvuRight chain
  const float* ur = F.u_right ? F.u_right + (size_t)f * F.cap : nullptr;
  uint4* cr = reinterpret_cast<uint4*>(F.cell_rec) + (size_t)f * F.cap;
  const int total = start[GRID_CELLS];
  for (int e = tid; e < total; e += GB_THREADS) {
    const int i = ci[e];
    const orbfe_keypoint kp = keys[i];
    // cell_rec_pack (search_device.h) by hand: through the helper the mvuRight load leaves the keypoint's round trip
    cr[e] = make_uint4((uint32_t)i | ((uint32_t)kp.octave << 24), (uint32_t)__float_as_int(kp.x), (uint32_t)__float_as_int(kp.y),
                       (uint32_t)__float_as_int(ur ? ur[i] : -1.0f));
  }
}
void orbfe_launch_grid_build(const FrameBatch& f, int n_frames, hipStream_t s) {
  if (f.cap > GB_LDS_CAP) {
    hipLaunchKernelGGL(grid_build_global_kernel, dim3(n_frames), dim3(GB_THREADS), 0, s, f);
    return;
  }
  static std::atomic<unsigned long long> raised{0};
  raise_dynamic_lds(reinterpret_cast<const void*>(grid_build_kernel), 6 * GB_LDS_CAP + 16, raised);
  hipLaunchKernelGGL(grid_build_kernel, dim3(n_frames), dim3(GB_THREADS), (size_t)6 * (size_t)f.cap + 16, s, f);
}
