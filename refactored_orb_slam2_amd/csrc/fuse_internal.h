// fuse_internal.h -- what fuse.cpp and fuse_kernels.hip share: the arguments of one row search of a resident fuse batch
#pragma once
#include "match_internal.h"

// Row (k, i) = point i of the resident table searched in target k.  A launch covers targets first_target .. K-1 and either every
// point (point_idx == nullptr, n_rows == n_points) or the points of an ascending index list.
struct FuseRows {
  FrameBatch F;                    // the K targets, grids built
  const orbfe_kf_camera* cams;     // [K]
  const float* inv_sigma2;         // [K][ORBFE_MAX_LEVELS], the first n_levels of a target read (nullptr: no table, ORBFE_KF_FUSE_SIM3)
  const float* geo;                // nullable, [K][4]: min_x, min_y, gw_inv, gh_inv of targets with image bounds of their own (else F's)
  const orbfe_kf_point* points;    // the resident table, [n_points]
  const int32_t* point_idx;        // nullable, [n_rows]
  const uint8_t* skip;             // nullable, [K][n_points]
  orbfe_kf_result* out;            // row (k, i) -> out[(k - out_first) * out_stride + (out_by_list ? j : i)]
  int out_first, out_stride, out_by_list;
  int n_points, n_rows, first_target, n_targets, mode;
};
void orbfe_launch_fuse_rows(const FuseRows& a, hipStream_t s);

// fuse.cpp: the validation and staging arithmetic of the host forms, which needs no device (tests/cpp_neighbors runs it under sanitizers)
struct FuseStage {   // offsets of the host search's staging block [records | index list | mask | results of the searched rows]
  size_t o_pts, o_idx, o_skip, o_res, total;
};
FuseStage orbfe_fuse_stage_layout(int K, int n_points, int n_rec, bool partial, bool with_skip, int first_target);
int orbfe_fuse_validate_rows(int K, int n_points);
int orbfe_fuse_validate_index(const int32_t* point_idx, int n_idx, int n_points);
int orbfe_fuse_validate_targets(int K, const orbfe_frame_view* targets, const orbfe_kf_camera* cams, const float* inv_level_sigma2, int mode,
                                int* cap_out);
void orbfe_fuse_release_spare();   // frees the stream and blocks the calling thread's last destroyed handle left for its next one
void orbfe_fuse_unstage_results(const orbfe_kf_result* staged, int K, int n_points, const int32_t* point_idx, int n_rec, int first_target,
                                orbfe_kf_result* results);
// table[idx[j]] = records[j], j < n (idx ascending: no two writers of one record); entries outside [0, n_points) are dropped
void orbfe_launch_fuse_scatter(orbfe_kf_point* table, int n_points, const orbfe_kf_point* records, const int32_t* idx, int n, hipStream_t s);
