// pose.cpp -- C ABI of Optimizer::PoseOptimization (include/orbfe.h: orbfe_pose_optimization*).  Both entry points validate and
// launch pose_kernels.hip; the host form stages one frame through device memory around the same launch.  No CPU fallback: without
// a device both are an error.
#include <string.h>

#include "host_internal.h"
#include "pose_internal.h"

#define POSE_MAX_ROWS 9500   // the frame limit of the projection searches (matcher.cpp), whose output this call reads

static bool stride_ok(int point_stride) {
  if (point_stride < 12 || (point_stride & 3)) {
    orbfe_set_error("pose optimisation: point_stride %d (at least 12 bytes -- three floats -- and a multiple of 4)", point_stride);
    return false;
  }
  return true;
}

extern "C" int orbfe_pose_optimization_batch_device(int n_frames, const orbfe_keypoint* d_keys_un, const float* d_u_right,
                                                    const int32_t* d_n, int cap, int32_t* d_assigned, const void* d_points,
                                                    int point_stride, const int32_t* d_n_points, int p_cap, int frame_shift,
                                                    const orbfe_pose_camera* d_camera, const float* d_Tcw_in, orbfe_pose_result* d_result,
                                                    uint8_t* d_outlier, int flags, void* stream) {
  if (!d_keys_un || !d_n || !d_assigned || !d_points || !d_n_points || !d_camera || !d_Tcw_in || !d_result || !d_outlier) {
    orbfe_set_error("pose optimisation batch: keypoints, counts, assignments, points, point counts, camera, poses, results and "
                    "outlier flags are required (only d_u_right may be NULL)");
    return ORBFE_ERR_INVALID;
  }
  if (n_frames < 0 || cap < 1 || cap > POSE_MAX_ROWS || p_cap < 1 || frame_shift < 0) {
    orbfe_set_error("pose optimisation batch: n_frames %d (>= 0), cap %d (1 .. %d), p_cap %d (>= 1), frame_shift %d (>= 0)", n_frames, cap,
                    POSE_MAX_ROWS, p_cap, frame_shift);
    return ORBFE_ERR_INVALID;
  }
  if (!stride_ok(point_stride)) return ORBFE_ERR_INVALID;
  if (flags & ~ORBFE_POSE_DISCARD) {
    orbfe_set_error("pose optimisation batch: unknown flags 0x%x", flags);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_keys_un & 3) || ((uintptr_t)d_u_right & 3) || ((uintptr_t)d_n & 3) || ((uintptr_t)d_assigned & 3) ||
      ((uintptr_t)d_points & 3) || ((uintptr_t)d_n_points & 3) || ((uintptr_t)d_camera & 3) || ((uintptr_t)d_Tcw_in & 3) ||
      ((uintptr_t)d_result & 3)) {
    orbfe_set_error("pose optimisation batch: records must be 4-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (n_frames == 0) return ORBFE_OK;
  orbfe_launch_pose_optimize(n_frames, d_keys_un, d_u_right, d_n, cap, d_assigned, (const uint8_t*)d_points, point_stride, d_n_points,
                             p_cap, frame_shift, d_camera, d_Tcw_in, d_result, d_outlier, flags, (hipStream_t)stream);
  return hip_status("kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_pose_optimization(const orbfe_frame_view* frame, const int32_t* assigned, const void* points, int point_stride,
                                       int n_points, const orbfe_pose_camera* camera, const float* Tcw_in, orbfe_pose_result* result,
                                       uint8_t* outlier) {
  if (!frame || !camera || !Tcw_in || !result) {
    orbfe_set_error("pose optimisation: frame, camera, input pose and result are required");
    return ORBFE_ERR_INVALID;
  }
  const int n = frame->n;
  if (n < 0 || n > POSE_MAX_ROWS || n_points < 0) {
    orbfe_set_error("pose optimisation: %d keypoints (0 .. %d), %d points (>= 0)", n, POSE_MAX_ROWS, n_points);
    return ORBFE_ERR_INVALID;
  }
  if (camera->n_levels < 1 || camera->n_levels > ORBFE_MAX_LEVELS) {
    orbfe_set_error("pose optimisation: n_levels %d (1 .. %d)", camera->n_levels, ORBFE_MAX_LEVELS);
    return ORBFE_ERR_INVALID;
  }
  if (!stride_ok(point_stride)) return ORBFE_ERR_INVALID;
  if ((n > 0 && (!frame->keys_un || !assigned || !outlier)) || (n_points > 0 && !points)) {
    orbfe_set_error("pose optimisation: keys_un, assigned and outlier are required for n > 0, points for n_points > 0");
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  const int cap = n > 0 ? n : 1, p_cap = n_points > 0 ? n_points : 1;
  // [input, uploaded | output, downloaded]; mvuRight has a region only when the frame has it, and reaches the kernel as NULL otherwise
  HostCall c("pose optimisation");
  const size_t o_hdr = c.in(16), o_cam = c.in(sizeof(orbfe_pose_camera)), o_T = c.in(12 * sizeof(float)),
               o_kps = c.in((size_t)cap * sizeof(orbfe_keypoint)), o_ur = c.in(frame->u_right ? (size_t)cap * sizeof(float) : 0),
               o_assigned = c.in((size_t)cap * sizeof(int32_t)), o_pts = c.in((size_t)p_cap * point_stride);
  const size_t o_res = c.out(sizeof(orbfe_pose_result)), o_out = c.out((size_t)cap);
  int rc;
  if ((rc = c.open())) return rc;
  c.host<int32_t>(o_hdr)[0] = n;
  c.host<int32_t>(o_hdr)[1] = n_points;
  memcpy(c.host(o_cam), camera, sizeof(orbfe_pose_camera));
  memcpy(c.host(o_T), Tcw_in, 12 * sizeof(float));
  if (n > 0) {
    memcpy(c.host(o_kps), frame->keys_un, (size_t)n * sizeof(orbfe_keypoint));
    if (frame->u_right) memcpy(c.host(o_ur), frame->u_right, (size_t)n * sizeof(float));
    memcpy(c.host(o_assigned), assigned, (size_t)n * sizeof(int32_t));
  }
  if (n_points > 0) memcpy(c.host(o_pts), points, (size_t)n_points * point_stride);
  if ((rc = c.upload())) return rc;
  orbfe_launch_pose_optimize(1, c.dev<const orbfe_keypoint>(o_kps), frame->u_right ? c.dev<const float>(o_ur) : nullptr, c.dev<const int32_t>(o_hdr),
                             cap, c.dev<int32_t>(o_assigned), c.dev(o_pts), point_stride, c.dev<const int32_t>(o_hdr) + 1, p_cap, 0,
                             c.dev<const orbfe_pose_camera>(o_cam), c.dev<const float>(o_T), c.dev<orbfe_pose_result>(o_res), c.dev(o_out), 0,
                             c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(result, c.host(o_res), sizeof(orbfe_pose_result));
  if (n > 0) memcpy(outlier, c.host(o_out), (size_t)n);
  return ORBFE_OK;
}
