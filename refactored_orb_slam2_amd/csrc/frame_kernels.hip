// frame_kernels.hip -- the per-keypoint tail of Frame::Frame for a batch of frames: UndistortKeyPoints (L/src/Frame.cc:419-445) and,
// for RGB-D frames, ComputeStereoFromRGBD (:648-666) on the depth map GrabImageRGBD scales (L/src/Tracking.cc:210-211).  The
// arithmetic is frame_internal.h's, shared with the host helpers of frame.cpp.
//
// One workgroup of 1 024 threads per frame: one keypoint row per lane up to 1 024 rows (seven dwords in, seven out, plus one 2- or
// 4-byte gather from the pitched depth map), and the count of keypoints with depth is a workgroup reduction -- no atomics, no memset
// launch.  The five iterations are a chain of dependent double divisions: with 256 threads a lane walked four rows one after the other
// and a CU held one wave per SIMD (37 us per 256 TUM frames); sixteen waves per CU hide that latency (profiles/rgbd_step.md).
// The camera is a by-value kernel argument read by field name only, so nothing lands in scratch memory.  k1 == 0 is a wave-uniform
// copy path.
#include "frame_internal.h"

#define UF_THREADS 1024

template <int FORMAT>
__global__ __launch_bounds__(UF_THREADS) void undistort_frames_kernel(const orbfe_keypoint* kps, const int32_t* __restrict__ n_rows,
                                                                      int cap, FrameCam cam, const uint8_t* __restrict__ depth,
                                                                      int width, int height, int pitch, size_t image_bytes,
                                                                      orbfe_keypoint* kps_un, float* __restrict__ u_right,
                                                                      float* __restrict__ depth_out, int32_t* __restrict__ n_depth) {
  __shared__ int wave_cnt[UF_THREADS / 64];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(n_rows[f], 0), cap);
  const size_t row0 = (size_t)f * cap;
  const uint8_t* map = FORMAT != ORBFE_DEPTH_NONE ? depth + (size_t)f * image_bytes : nullptr;
  int cnt = 0;
  for (int i = tid; i < n; i += UF_THREADS) {
    // in place (kps_un == kps) is safe: every row is read and written by the same thread only
    const orbfe_keypoint kp = kps[row0 + i];
    orbfe_keypoint ku = kp;
    orbfe_key_un(cam, kp.x, kp.y, &ku.x, &ku.y);
    kps_un[row0 + i] = ku;
    if (FORMAT == ORBFE_DEPTH_NONE) {
      if (u_right) u_right[row0 + i] = -1.0f;
      if (depth_out) depth_out[row0 + i] = -1.0f;
      continue;
    }
    float d = 0.0f;   // outside the map: no depth
    int xi, yi;
    if (orbfe_depth_cell(kp.x, kp.y, width, height, &xi, &yi)) {
      if (FORMAT == ORBFE_DEPTH_U16)
        d = orbfe_depth_value_u16(cam, *reinterpret_cast<const uint16_t*>(map + (size_t)yi * pitch + (size_t)xi * 2));
      else
        d = orbfe_depth_value_f32(cam, *reinterpret_cast<const float*>(map + (size_t)yi * pitch + (size_t)xi * 4));
    }
    float ur, dz;
    cnt += orbfe_rgbd_stereo(cam, ku.x, d, &ur, &dz) ? 1 : 0;
    u_right[row0 + i] = ur;
    depth_out[row0 + i] = dz;
  }
  if (!n_depth) return;   // uniform: a kernel argument
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if ((tid & 63) == 0) wave_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < UF_THREADS / 64; w++) total += wave_cnt[w];
    n_depth[f] = total;
  }
}

void orbfe_launch_undistort_frames(int n_frames, const orbfe_keypoint* kps, const int32_t* n, int cap, const FrameCam& cam,
                                   int depth_format, const uint8_t* depth, int width, int height, int depth_pitch,
                                   size_t depth_image_bytes, orbfe_keypoint* kps_un, float* u_right, float* depth_out,
                                   int32_t* n_depth, hipStream_t s) {
  if (n_frames < 1) return;
  const dim3 grid(n_frames), block(UF_THREADS);
  if (depth_format == ORBFE_DEPTH_U16)
    hipLaunchKernelGGL(undistort_frames_kernel<ORBFE_DEPTH_U16>, grid, block, 0, s, kps, n, cap, cam, depth, width, height, depth_pitch,
                       depth_image_bytes, kps_un, u_right, depth_out, n_depth);
  else if (depth_format == ORBFE_DEPTH_F32)
    hipLaunchKernelGGL(undistort_frames_kernel<ORBFE_DEPTH_F32>, grid, block, 0, s, kps, n, cap, cam, depth, width, height, depth_pitch,
                       depth_image_bytes, kps_un, u_right, depth_out, n_depth);
  else
    hipLaunchKernelGGL(undistort_frames_kernel<ORBFE_DEPTH_NONE>, grid, block, 0, s, kps, n, cap, cam, depth, width, height, depth_pitch,
                       depth_image_bytes, kps_un, u_right, depth_out, n_depth);
}
