// pose.cpp -- C ABI of Optimizer::PoseOptimization (include/orbfe.h: orbfe_pose_optimization*).  Both entry points validate and
// launch pose_kernels.hip; the host form stages one frame through device memory around the same launch.  No CPU fallback: without
// a device both are an error.
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
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) {
    orbfe_set_error("kernel launch failed: %s", hipGetErrorString(le));
    return ORBFE_ERR_HIP;
  }
  return ORBFE_OK;
}

namespace {
// one device allocation holding every array of the host form, released on every path
struct Staging {
  uint8_t* base = nullptr;
  size_t used = 0;
  ~Staging() {
    if (base) (void)hipFree(base);
  }
  static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
  template <class T>
  T* take(size_t bytes) {
    T* p = reinterpret_cast<T*>(base + used);
    used += pad(bytes);
    return p;
  }
};
}  // namespace

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
  const size_t b_kps = (size_t)cap * sizeof(orbfe_keypoint), b_f = (size_t)cap * sizeof(float), b_pts = (size_t)p_cap * point_stride;
  Staging st;
  const size_t total = Staging::pad(b_kps) + 2 * Staging::pad(b_f) + Staging::pad(b_pts) + Staging::pad((size_t)cap) + 5 * 256;
  hipError_t e = hipMalloc((void**)&st.base, total);
  if (e != hipSuccess) {
    st.base = nullptr;
    orbfe_set_error("pose optimisation: device allocation of %zu bytes failed: %s", total, hipGetErrorString(e));
    return ORBFE_ERR_HIP;
  }
  orbfe_keypoint* d_kps = st.take<orbfe_keypoint>(b_kps);
  float* d_ur = st.take<float>(b_f);
  int32_t* d_assigned = st.take<int32_t>(b_f);
  uint8_t* d_pts = st.take<uint8_t>(b_pts);
  uint8_t* d_out = st.take<uint8_t>((size_t)cap);
  int32_t* d_n = st.take<int32_t>(4);
  int32_t* d_np = st.take<int32_t>(4);
  orbfe_pose_camera* d_cam = st.take<orbfe_pose_camera>(sizeof(orbfe_pose_camera));
  float* d_T = st.take<float>(12 * sizeof(float));
  orbfe_pose_result* d_res = st.take<orbfe_pose_result>(sizeof(orbfe_pose_result));
  const int32_t hn = n, hnp = n_points;
  if (n > 0) {
    e = hipMemcpy(d_kps, frame->keys_un, (size_t)n * sizeof(orbfe_keypoint), hipMemcpyHostToDevice);
    if (e == hipSuccess && frame->u_right) e = hipMemcpy(d_ur, frame->u_right, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_assigned, assigned, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && n_points > 0) e = hipMemcpy(d_pts, points, (size_t)n_points * point_stride, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_n, &hn, 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_np, &hnp, 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_cam, camera, sizeof(orbfe_pose_camera), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_T, Tcw_in, 12 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    orbfe_launch_pose_optimize(1, d_kps, frame->u_right ? d_ur : nullptr, d_n, cap, d_assigned, d_pts, point_stride, d_np, p_cap, 0, d_cam,
                               d_T, d_res, d_out, 0, (hipStream_t) nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(result, d_res, sizeof(orbfe_pose_result), hipMemcpyDeviceToHost);   // waits for the kernel
  if (e == hipSuccess && n > 0) e = hipMemcpy(outlier, d_out, (size_t)n, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    orbfe_set_error("pose optimisation: %s", hipGetErrorString(e));
    return ORBFE_ERR_HIP;
  }
  return ORBFE_OK;
}
