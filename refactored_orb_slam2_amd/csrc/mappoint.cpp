// mappoint.cpp -- C ABI of MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (include/orbfe.h:
// orbfe_refresh_map_points*).  The entry points validate, stage and launch mappoint_kernels.hip.  No CPU fallback: without a device
// both are an error.
#include <string.h>

#include "host_internal.h"
#include "mappoint_internal.h"

namespace {

// what both forms check before any device call
bool counts_ok(const char* where, int P, int n_kf, int n_obs_total, const float* scale_factors, int n_levels, int flags) {
  if (P < 0 || P > ORBFE_MP_MAX_POINTS || n_kf < 0 || n_kf > ORBFE_MP_MAX_KEYFRAMES || n_obs_total < 0 || n_obs_total > ORBFE_MP_MAX_TOTAL_OBS) {
    orbfe_set_error("%s: P %d (0 .. %d), n_kf %d (0 .. %d), n_obs_total %d (0 .. %d)", where, P, ORBFE_MP_MAX_POINTS, n_kf,
                    ORBFE_MP_MAX_KEYFRAMES, n_obs_total, ORBFE_MP_MAX_TOTAL_OBS);
    return false;
  }
  if (!scale_factors || n_levels < 1 || n_levels > ORBFE_MAX_LEVELS) {
    orbfe_set_error("%s: scale_factors are required, n_levels %d (1 .. %d)", where, n_levels, ORBFE_MAX_LEVELS);
    return false;
  }
  if (!(flags & (ORBFE_MP_DESCRIPTOR | ORBFE_MP_NORMAL_DEPTH)) || (flags & ~(ORBFE_MP_DESCRIPTOR | ORBFE_MP_NORMAL_DEPTH))) {
    orbfe_set_error("%s: flags %d (ORBFE_MP_DESCRIPTOR, ORBFE_MP_NORMAL_DEPTH or both)", where, flags);
    return false;
  }
  return true;
}

void fill(MpLaunch& L, int P, int n_kf, int n_obs_total, const float* scale_factors, int n_levels, int flags) {
  memset(&L, 0, sizeof(L));
  L.P = P; L.n_kf = n_kf; L.n_obs_total = n_obs_total; L.n_levels = n_levels; L.flags = flags;
  for (int l = 0; l < n_levels; l++) L.scale_factors[l] = scale_factors[l];
}

}  // namespace

extern "C" int orbfe_refresh_map_points_batch_device(int P, const orbfe_mp_keyframe* d_keyframes, int n_kf, const orbfe_mp_obs* d_obs,
                                                     int n_obs_total, const orbfe_mp_point* d_points, const void* d_points_pos,
                                                     int point_stride, const float* scale_factors, int n_levels, int flags,
                                                     orbfe_mp_update* d_updates, void* stream) {
  const char* where = "refresh map points batch";
  if (!counts_ok(where, P, n_kf, n_obs_total, scale_factors, n_levels, flags)) return ORBFE_ERR_INVALID;
  if (point_stride < 12 || (point_stride & 3)) {
    orbfe_set_error("%s: point_stride %d (at least 12 bytes -- three floats -- and a multiple of 4)", where, point_stride);
    return ORBFE_ERR_INVALID;
  }
  if ((P > 0 && (!d_points || !d_points_pos || !d_updates)) || (n_kf > 0 && !d_keyframes) || (n_obs_total > 0 && !d_obs)) {
    orbfe_set_error("%s: points, positions and updates are required for P > 0, the keyframe table for n_kf > 0, the observations for "
                    "n_obs_total > 0", where);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_keyframes & 7) || ((uintptr_t)d_obs & 3) || ((uintptr_t)d_points & 3) || ((uintptr_t)d_points_pos & 3) ||
      ((uintptr_t)d_updates & 3)) {
    orbfe_set_error("%s: records must be 4-byte aligned, the keyframe table 8-byte", where);
    return ORBFE_ERR_INVALID;
  }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;
  if (P == 0) return ORBFE_OK;
  MpLaunch L;
  fill(L, P, n_kf, n_obs_total, scale_factors, n_levels, flags);
  L.kfs = d_keyframes; L.obs = d_obs; L.points = d_points; L.pos = (const uint8_t*)d_points_pos; L.pos_stride = point_stride;
  L.out = d_updates;
  orbfe_launch_refresh_map_points(L, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_status("refresh map points batch: kernel launch failed", e);
  return ORBFE_OK;
}

extern "C" int orbfe_refresh_map_points(const orbfe_mp_keyframe* keyframes, int n_kf, const orbfe_mp_obs* obs, int n_obs_total,
                                        const orbfe_mp_point* points, const float* positions, int P, const float* scale_factors,
                                        int n_levels, int flags, orbfe_mp_update* updates) {
  const char* where = "refresh map points";
  if (!counts_ok(where, P, n_kf, n_obs_total, scale_factors, n_levels, flags)) return ORBFE_ERR_INVALID;
  if ((P > 0 && (!points || !positions || !updates)) || (n_kf > 0 && !keyframes) || (n_obs_total > 0 && !obs)) {
    orbfe_set_error("%s: points, positions and updates are required for P > 0, the keyframe table for n_kf > 0, the observations for "
                    "n_obs_total > 0", where);
    return ORBFE_ERR_INVALID;
  }
  if (P == 0) return have_device() ? ORBFE_OK : ORBFE_ERR_NO_DEVICE;   // nothing behind the counts is read
  for (int p = 0; p < P; p++)
    if (points[p].n_obs > ORBFE_MP_MAX_OBS) {
      orbfe_set_error("%s: point %d has %d observations (0 .. %d)", where, p, points[p].n_obs, ORBFE_MP_MAX_OBS);
      return ORBFE_ERR_INVALID;
    }
  const bool want_desc = (flags & ORBFE_MP_DESCRIPTOR) != 0;
  for (int k = 0; k < n_kf; k++)
    if (keyframes[k].n_keys < 0 || (want_desc && keyframes[k].n_keys > 0 && !keyframes[k].desc)) {
      orbfe_set_error("%s: keyframe %d has n_keys %d%s", where, k, keyframes[k].n_keys, keyframes[k].n_keys < 0 ? "" : " and no descriptors");
      return ORBFE_ERR_INVALID;
    }
  if (!have_device()) return ORBFE_ERR_NO_DEVICE;

  HostCall c(where);
  const size_t o_kf = c.in((size_t)n_kf * sizeof(orbfe_mp_keyframe)), o_obs = c.in((size_t)n_obs_total * sizeof(orbfe_mp_obs)),
               o_pts = c.in((size_t)P * sizeof(orbfe_mp_point)), o_pos = c.in((size_t)P * 12),
               o_desc = c.in(want_desc ? (size_t)n_obs_total * 32 : 0);
  const size_t o_out = c.out((size_t)P * sizeof(orbfe_mp_update));
  int rc;
  if ((rc = c.open())) return rc;
  uint8_t *const h = c.host(0), *const d = c.dev(0);
  if (n_kf) memcpy(h + o_kf, keyframes, (size_t)n_kf * sizeof(orbfe_mp_keyframe));
  if (n_obs_total) memcpy(h + o_obs, obs, (size_t)n_obs_total * sizeof(orbfe_mp_obs));
  memcpy(h + o_pts, points, (size_t)P * sizeof(orbfe_mp_point));
  memcpy(h + o_pos, positions, (size_t)P * 12);
  if (want_desc)   // the rows some observation names, by observation; a row the device will refuse stays zero
    for (int g = 0; g < n_obs_total; g++) {
      const orbfe_mp_obs o = obs[g];
      uint8_t* row = h + o_desc + (size_t)g * 32;
      if (mp_obs_kf_ok(o, n_kf) && mp_obs_idx_ok(o, keyframes[o.kf], false))
        memcpy(row, reinterpret_cast<const uint8_t*>((uintptr_t)keyframes[o.kf].desc) + (size_t)o.idx * 32, 32);
      else
        memset(row, 0, 32);
    }
  if ((rc = c.upload())) return rc;
  MpLaunch L;
  fill(L, P, n_kf, n_obs_total, scale_factors, n_levels, flags);
  L.kfs = (const orbfe_mp_keyframe*)(d + o_kf); L.obs = (const orbfe_mp_obs*)(d + o_obs); L.points = (const orbfe_mp_point*)(d + o_pts);
  L.pos = d + o_pos; L.pos_stride = 12;
  L.staged = d + o_desc;   // also without the descriptor half: the table's addresses are the host's and are never read
  L.out = (orbfe_mp_update*)(d + o_out);
  orbfe_launch_refresh_map_points(L, c.stream);
  if ((rc = c.finish((size_t)P * sizeof(orbfe_mp_update)))) return rc;
  const orbfe_mp_update* r = (const orbfe_mp_update*)(h + o_out);
  for (int p = 0; p < P; p++) {   // the status and the selected halves
    orbfe_mp_update& U = updates[p];
    U.status = r[p].status;
    if (want_desc) {
      U.best = r[p].best;
      U.n_live = r[p].n_live;
      memcpy(U.desc, r[p].desc, 32);
    }
    if (flags & ORBFE_MP_NORMAL_DEPTH) {
      memcpy(U.normal, r[p].normal, sizeof(U.normal));
      U.min_distance = r[p].min_distance;
      U.max_distance = r[p].max_distance;
    }
  }
  return ORBFE_OK;
}
