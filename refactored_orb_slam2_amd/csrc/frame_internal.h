// frame_internal.h -- the per-keypoint arithmetic of Frame::Frame that the undistortion / RGB-D kernel (frame_kernels.hip) and the
// host helpers (frame.cpp: orbfe_image_bounds, orbfe_undistort_points) share.  One definition, compiled for both sides with
// -ffp-contract=off: no a*b+c is fused on either side, so host and device produce the same bits.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/):
//   Frame::UndistortKeyPoints     L/src/Frame.cc:419-445   cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK)
//   Frame::ComputeImageBounds     L/src/Frame.cc:447-476
//   Frame::ComputeStereoFromRGBD  L/src/Frame.cc:648-666
//   Tracking::GrabImageRGBD       L/src/Tracking.cc:210-211 (depth map scaling), factor from :141-147
// cv::undistortPoints is OpenCV's cvUndistortPointsInternal (4.5.4 - 4.6, generic path): double arithmetic, the default criterion
// of exactly five iterations (COUNT only), R = I, P = K.  With R = I and P = K every term the generic code adds beyond the ones below
// is a product with 0 / 1 or an addition of 0 -- exact for finite input -- so the simplified form gives the same bits; the order of
// the non-zero terms is the reference's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbfe.h"

// The camera as the undistortion reads it: mK and mDistCoef widened to double (cvConvert of the CV_32F matrices), plus the two floats
// of the RGB-D tail.  Passed to the kernel by value and read with uniform field names only (never indexed per lane).
struct FrameCam {
  double fx, fy, cx, cy;        // K
  double ifx, ify;              // 1./fx, 1./fy
  double k1, k2, p1, p2, k3;    // k[0..4]; k[5..11] = 0
  float mbf;                    // Camera.bf
  float depth_factor;           // mDepthMapFactor
  int32_t undistort;            // mDistCoef.at<float>(0) != 0  (Frame.cc:420, :448)
  int32_t scale_depth;          // GrabImageRGBD's convertTo applies: 16-bit map, or |factor - 1| > 1e-5 (Tracking.cc:210)
};

__host__ __device__ inline FrameCam orbfe_frame_cam(const orbfe_calibration& c, int depth_format) {
  FrameCam k;
  k.fx = (double)c.fx;
  k.fy = (double)c.fy;
  k.cx = (double)c.cx;
  k.cy = (double)c.cy;
  k.ifx = 1. / k.fx;
  k.ify = 1. / k.fy;
  k.k1 = (double)c.k1;
  k.k2 = (double)c.k2;
  k.p1 = (double)c.p1;
  k.p2 = (double)c.p2;
  k.k3 = (double)c.k3;
  k.mbf = c.mbf;
  k.depth_factor = c.depth_factor;
  k.undistort = c.k1 != 0.0f;
  // fabs(mDepthMapFactor - 1.0f) > 1e-5: a float difference compared against the double 1e-5
  k.scale_depth = depth_format == ORBFE_DEPTH_U16 || (double)fabsf(c.depth_factor - 1.0f) > 1e-5;
  return k;
}

// cv::undistortPoints of one point (u, v) = the float keypoint coordinates; *icdist_neg (optional) reports the icdist < 0 exit
__host__ __device__ inline void orbfe_undistort_point(const FrameCam& k, float uf, float vf, float* xo, float* yo,
                                                      int* icdist_neg = nullptr) {
  const double u = (double)uf, v = (double)vf;
  double x = (u - k.cx) * k.ifx;
  double y = (v - k.cy) * k.ify;
  const double x0 = x, y0 = y;
  int neg = 0;
  for (int j = 0; j < 5; j++) {
    const double r2 = x * x + y * y;
    const double icdist = 1. / (1 + ((k.k3 * r2 + k.k2) * r2 + k.k1) * r2);
    if (icdist < 0) {   // OpenCV regression_14583: give up on the point
      x = (u - k.cx) * k.ifx;
      y = (v - k.cy) * k.ify;
      neg = 1;
      break;
    }
    const double deltaX = 2 * k.p1 * x * y + k.p2 * (r2 + 2 * x * x);
    const double deltaY = k.p1 * (r2 + 2 * y * y) + 2 * k.p2 * x * y;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  // RR = P * R = K: xx = fx*x + cx, yy = fy*y + cy, ww = 1
  *xo = (float)(k.fx * x + k.cx);
  *yo = (float)(k.fy * y + k.cy);
  if (icdist_neg) *icdist_neg = neg;
}

// mvKeysUn[i].pt of keypoint (x, y): the keypoint itself when k1 == 0 (Frame.cc:420-423)
__host__ __device__ inline void orbfe_key_un(const FrameCam& k, float x, float y, float* xo, float* yo) {
  if (k.undistort) {
    orbfe_undistort_point(k, x, y, xo, yo);
  } else {
    *xo = x;
    *yo = y;
  }
}

// The depth map sample ComputeStereoFromRGBD reads for keypoint (x, y): imDepth.at<float>((int)y, (int)x) after GrabImageRGBD's
// convertTo.  in_map = 0 when the truncated coordinates fall outside the w x h map (the extractor never produces such a keypoint;
// the library reads nothing then and reports no depth).
__host__ __device__ inline bool orbfe_depth_cell(float x, float y, int w, int h, int* xi, int* yi) {
  // -1 < x < w  <=>  0 <= (int)x < w for the truncation toward zero; NaN fails both
  if (!(x > -1.0f && x < (float)w && y > -1.0f && y < (float)h)) return false;
  *xi = (int)x;
  *yi = (int)y;
  return true;
}
__host__ __device__ inline float orbfe_depth_value_u16(const FrameCam& k, uint16_t raw) {
  return (float)raw * k.depth_factor;   // convertTo(CV_32F, alpha): one rounding
}
__host__ __device__ inline float orbfe_depth_value_f32(const FrameCam& k, float raw) {
  return k.scale_depth ? raw * k.depth_factor : raw;
}
// mvDepth / mvuRight from the sample d (Frame.cc:659-663); returns whether the keypoint has depth
__host__ __device__ inline bool orbfe_rgbd_stereo(const FrameCam& k, float x_un, float d, float* u_right, float* depth) {
  if (d > 0) {
    *depth = d;
    *u_right = x_un - k.mbf / d;
    return true;
  }
  *depth = -1.0f;
  *u_right = -1.0f;
  return false;
}

void orbfe_launch_undistort_frames(int n_frames, const orbfe_keypoint* kps, const int32_t* n, int cap, const FrameCam& cam,
                                   int depth_format, const uint8_t* depth, int width, int height, int depth_pitch,
                                   size_t depth_image_bytes, orbfe_keypoint* kps_un, float* u_right, float* depth_out,
                                   int32_t* n_depth, hipStream_t s);
