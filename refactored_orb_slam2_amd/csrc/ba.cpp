// ba.cpp -- C ABI of Optimizer::BundleAdjustment (include/orbfe.h: orbfe_bundle_adjustment, orbfe_bundle_adjustment_batch_device).
// The graph, its records, its limits and its workspace are the local bundle adjustment's, so validating, sorting, staging (HostCall)
// and launching are lba.cpp's lba_host_entry and lba_batch_entry; this file names the schedule: ONE optimize(n_iterations) of
// ba_kernels.hip, robust or not.  No CPU fallback: without a device both forms are an error.
#include "host_internal.h"
#include "lba_internal.h"

static LbaSchedule schedule(int n_iterations) { return LbaSchedule{"bundle adjustment", n_iterations, ORBFE_BA_ROBUST, true}; }

extern "C" int orbfe_bundle_adjustment(const orbfe_pose_camera* camera, const float* poses, const uint8_t* fixed, int n_kf,
                                       const float* points, int n_points, const orbfe_lba_edge* edges, int n_edges, int n_iterations,
                                       int flags, float* poses_out, float* points_out, orbfe_ba_result* result) {
  return lba_host_entry(schedule(n_iterations), camera, poses, fixed, n_kf, points, n_points, edges, n_edges, flags, poses_out, points_out,
                        nullptr, result);
}

extern "C" int orbfe_bundle_adjustment_batch_device(int P, const orbfe_pose_camera* d_camera, const orbfe_lba_problem* d_problems,
                                                    const float* d_poses, const uint8_t* d_fixed, const uint8_t* d_points, int point_stride,
                                                    const orbfe_lba_edge* d_edges, int kf_cap, int point_cap, int edge_cap,
                                                    int n_iterations, int flags, float* d_poses_out, float* d_points_out,
                                                    orbfe_ba_result* d_result, void* d_workspace, size_t workspace_bytes, void* stream) {
  return lba_batch_entry(schedule(n_iterations), P, d_camera, d_problems, d_poses, d_fixed, d_points, point_stride, d_edges, kf_cap,
                         point_cap, edge_cap, flags, d_poses_out, d_points_out, nullptr, d_result, d_workspace, workspace_bytes, stream);
}
