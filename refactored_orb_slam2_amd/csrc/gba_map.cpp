// gba_map.cpp -- C ABI of the map update behind the global bundle adjustment (include/orbfe.h: orbfe_gba_update_map,
// orbfe_gba_update_map_device).  The entry points validate, stage and launch gba_map_kernels.hip.  No CPU fallback: without a device
// both forms are an error.
#include <string.h>

#include "gba_map_internal.h"
#include "host_internal.h"

// what both forms can check without reading an array: counts, null pointers, alignment, aliasing
static bool args_ok(const char* who, const GmLaunch& L) {
  if (L.n_kf < 0 || L.n_kf > ORBFE_GBA_MAP_MAX_KEYFRAMES || L.n_gba_kf < 0 || L.n_gba_kf > ORBFE_GBA_MAP_MAX_KEYFRAMES) {
    orbfe_set_error("%s: n_kf %d, n_gba_kf %d (0 .. %d)", who, L.n_kf, L.n_gba_kf, ORBFE_GBA_MAP_MAX_KEYFRAMES);
    return false;
  }
  if (L.n_points < 0 || L.n_points > ORBFE_GBA_MAP_MAX_POINTS || L.n_gba_points < 0 || L.n_gba_points > ORBFE_GBA_MAP_MAX_POINTS) {
    orbfe_set_error("%s: n_points %d, n_gba_points %d (0 .. %d)", who, L.n_points, L.n_gba_points, ORBFE_GBA_MAP_MAX_POINTS);
    return false;
  }
  if (L.point_stride < 12 || (L.point_stride & 3)) {
    orbfe_set_error("%s: point_stride %d (>= 12, a multiple of 4)", who, L.point_stride);
    return false;
  }
  if (!L.result || (L.n_kf > 0 && (!L.poses || !L.parent || !L.kf_gba_row || !L.kf_out)) || (L.n_gba_kf > 0 && !L.gba_poses) ||
      (L.n_points > 0 && (!L.points || !L.point_gba_row || !L.ref || !L.points_out)) || (L.n_gba_points > 0 && !L.gba_points)) {
    orbfe_set_error("%s: result and the arrays of a count > 0 are required", who);
    return false;
  }
  const void* in[8] = {L.poses, L.parent, L.kf_gba_row, L.gba_poses, L.points, L.point_gba_row, L.ref, L.gba_points};
  const void* out[3] = {L.kf_out, L.points_out, L.result};
  for (int i = 0; i < 8; i++)
    if ((uintptr_t)in[i] & 3) {
      orbfe_set_error("%s: every input array must be 4-byte aligned", who);
      return false;
    }
  if (((uintptr_t)L.kf_out & 7) || ((uintptr_t)L.result & 3) || ((uintptr_t)L.points_out & 3)) {
    orbfe_set_error("%s: kf_out must be 8-byte, points_out and result 4-byte aligned", who);
    return false;
  }
  for (int o = 0; o < 3; o++) {
    if (!out[o]) continue;
    for (int i = 0; i < 8; i++)
      if (out[o] == in[i]) {
        orbfe_set_error("%s: an output must not be an input", who);
        return false;
      }
    for (int q = 0; q < o; q++)
      if (out[o] == out[q]) {
        orbfe_set_error("%s: two outputs must not be the same array", who);
        return false;
      }
  }
  return true;
}

static bool rows_ok(const char* who, const char* name, const int32_t* v, int n, int rows) {
  for (int i = 0; i < n; i++)
    if (v[i] < -1 || v[i] >= rows) {
      orbfe_set_error("%s: %s[%d] = %d (-1 .. %d)", who, name, i, v[i], rows - 1);
      return false;
    }
  return true;
}

extern "C" int orbfe_gba_update_map_device(const float* d_poses, const int32_t* d_parent, const int32_t* d_kf_gba_row, int n_kf,
                                           const float* d_gba_poses, int n_gba_kf, float half_baseline, const uint8_t* d_points,
                                           int point_stride, const int32_t* d_point_gba_row, const int32_t* d_ref, int n_points,
                                           const float* d_gba_points, int n_gba_points, orbfe_gba_map_keyframe* d_kf_out,
                                           float* d_points_out, orbfe_gba_map_result* d_result, void* stream) {
  const char* who = "gba update map device";
  const GmLaunch L = {n_kf,     n_gba_kf,    n_points, point_stride,    n_gba_points, half_baseline, d_poses,  d_parent,     d_kf_gba_row,
                      d_gba_poses, d_points, d_point_gba_row, d_ref,    d_gba_points, d_kf_out,      d_points_out, d_result};
  if (!args_ok(who, L)) return ORBFE_ERR_INVALID;
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  HIPCHK(hipMemsetAsync(d_result, 0, sizeof(orbfe_gba_map_result), (hipStream_t)stream));
  orbfe_launch_gba_map(L, (hipStream_t)stream);
  return hip_status("gba update map device: kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_gba_update_map(const float* poses, const int32_t* parent, const int32_t* kf_gba_row, int n_kf, const float* gba_poses,
                                    int n_gba_kf, float half_baseline, const float* points, const int32_t* point_gba_row,
                                    const int32_t* ref, int n_points, const float* gba_points, int n_gba_points,
                                    orbfe_gba_map_keyframe* kf_out, float* points_out, orbfe_gba_map_result* result) {
  const char* who = "gba update map";
  const GmLaunch H = {n_kf,   n_gba_kf, n_points,      12,  n_gba_points, half_baseline, poses,  parent,     kf_gba_row,
                      gba_poses, (const uint8_t*)points, point_gba_row, ref, gba_points,  kf_out,        points_out, result};
  if (!args_ok(who, H)) return ORBFE_ERR_INVALID;
  if (!rows_ok(who, "parent", parent, n_kf, n_kf) || !rows_ok(who, "kf_gba_row", kf_gba_row, n_kf, n_gba_kf) ||
      !rows_ok(who, "point_gba_row", point_gba_row, n_points, n_gba_points) || !rows_ok(who, "ref", ref, n_points, n_kf))
    return ORBFE_ERR_INVALID;
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  memset(result, 0, sizeof(*result));
  if (n_kf == 0 && n_points == 0) return ORBFE_OK;
  HostCall c(who);
  const size_t b_kf = (size_t)n_kf, b_pt = (size_t)n_points;
  const size_t o_T = c.in(b_kf * 48), o_par = c.in(b_kf * 4), o_row = c.in(b_kf * 4), o_G = c.in((size_t)n_gba_kf * 48),
               o_X = c.in(b_pt * 12), o_prow = c.in(b_pt * 4), o_ref = c.in(b_pt * 4), o_GX = c.in((size_t)n_gba_points * 12);
  const size_t o_res = c.out(sizeof(orbfe_gba_map_result)), o_kf = c.out(b_kf * sizeof(orbfe_gba_map_keyframe)), o_out = c.out(b_pt * 12);
  int rc;
  if ((rc = c.open())) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  auto put = [h](size_t off, const void* src, size_t bytes) {
    if (bytes) memcpy(h + off, src, bytes);
  };
  put(o_T, poses, b_kf * 48);
  put(o_par, parent, b_kf * 4);
  put(o_row, kf_gba_row, b_kf * 4);
  put(o_G, gba_poses, (size_t)n_gba_kf * 48);
  put(o_X, points, b_pt * 12);
  put(o_prow, point_gba_row, b_pt * 4);
  put(o_ref, ref, b_pt * 4);
  put(o_GX, gba_points, (size_t)n_gba_points * 12);
  if ((rc = c.upload())) return rc;
  GmLaunch L = H;
  L.poses = (const float*)(d + o_T);
  L.parent = (const int32_t*)(d + o_par);
  L.kf_gba_row = (const int32_t*)(d + o_row);
  L.gba_poses = (const float*)(d + o_G);
  L.points = d + o_X;
  L.point_gba_row = (const int32_t*)(d + o_prow);
  L.ref = (const int32_t*)(d + o_ref);
  L.gba_points = (const float*)(d + o_GX);
  L.result = (orbfe_gba_map_result*)(d + o_res);
  L.kf_out = (orbfe_gba_map_keyframe*)(d + o_kf);
  L.points_out = (float*)(d + o_out);
  if ((rc = c.status(hipMemsetAsync(L.result, 0, sizeof(orbfe_gba_map_result), c.stream)))) return rc;
  orbfe_launch_gba_map(L, c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(result, h + o_res, sizeof(*result));
  if (n_kf) memcpy(kf_out, h + o_kf, b_kf * sizeof(orbfe_gba_map_keyframe));
  if (n_points) memcpy(points_out, h + o_out, b_pt * 12);
  return ORBFE_OK;
}
