// search_device.h -- device code that more than one kernel unit of the searches states: the library is built with -fno-gpu-rdc, so
// what two units share lives here, once.
//   wave helpers, hamming256, load_desc           hamming_, grid_, projection_, bow_, stereo_kernels.hip, fuse_kernels.hip
//   cell_rec_pack / cell_rec_unpack               grid_kernels.hip writes the records; enumerate_window and proj_candidates read them
//   enumerate_window                              projection_kernels.hip (proj_best, proj_resolve, init_resolve), fuse_kernels.hip
//   rot_bin, three_maxima                         projection_kernels.hip, bow_kernels.hip
//   predict_scale, kf_project                     frustum_kernels.hip (frustum / kf queries), fuse_kernels.hip
// Compiled with -ffp-contract=off: every float expression is evaluated un-fused, as the reference does.
#pragma once
#include <hip/hip_runtime.h>

#include "match_internal.h"

#ifndef WAVE
#define WAVE 64
#endif

__device__ __forceinline__ int hamming256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
__device__ __forceinline__ void load_desc(const uint8_t* p, uint4& d0, uint4& d1) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  d0 = q[0];
  d1 = q[1];
}
// descriptors that are only 4-byte aligned (queries embedded in 68-byte records)
__device__ __forceinline__ void load_desc4(const uint8_t* p, uint4& d0, uint4& d1) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
  d0 = make_uint4(q[0], q[1], q[2], q[3]);
  d1 = make_uint4(q[4], q[5], q[6], q[7]);
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  // DPP reduction (row shifts, then row broadcasts): lane 63 ends up with the minimum of all 64 lanes
#define ORBFE_MIN_STEP(ctrl, rmask) v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)0xffffffff, (int)v, ctrl, rmask, 0xf, false))
  ORBFE_MIN_STEP(0x111, 0xf); ORBFE_MIN_STEP(0x112, 0xf); ORBFE_MIN_STEP(0x114, 0xf); ORBFE_MIN_STEP(0x118, 0xf);
  ORBFE_MIN_STEP(0x142, 0xa); ORBFE_MIN_STEP(0x143, 0xc);
#undef ORBFE_MIN_STEP
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ int wave_incl_scan_i(int v) {
  // DPP row shifts + row broadcasts (gfx9): six VALU adds, no LDS crossbar round trips (ds_bpermute) as with __shfl_up
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) { return __builtin_amdgcn_readlane(wave_incl_scan_i(v), 63); }

// Rotation-histogram bin of a match: `rot = angle1 - angle2; if (rot < 0) rot += 360; bin = round(rot * factor)` with the
// reference's factor (sic) 1 / HISTO_LENGTH (L/src/ORBmatcher.cc:174,232-237; again at :456, :574, :719, :1352, :1475)
__device__ __forceinline__ int rot_bin(float angle1, float angle2) {
  float rot = angle1 - angle2;
  if (rot < 0.0f) rot += 360.0f;
  const int bin = (int)roundf(rot * (1.0f / ORBFE_HISTO_LENGTH));
  return bin == ORBFE_HISTO_LENGTH ? 0 : bin;
}
// ComputeThreeMaxima (L/src/ORBmatcher.cc:1506-1538)
__device__ inline void three_maxima(const int* hs, int L, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0;
  ind1 = ind2 = ind3 = -1;
  for (int i = 0; i < L; i++) {
    const int s = hs[i];
    if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
    else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
    else if (s > max3) { max3 = s; ind3 = i; }
  }
  if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
  else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

// The 16-byte record of FrameBatch::cell_rec, one per grid entry in CSR order: everything a window walk tests per entry
// (L/src/Frame.cc:379-393 and the matcher's mvuRight gate) instead of the index -> keypoint -> mvuRight chain.  A second writer
// states this layout by hand: the record loop of grid_build_global_kernel (grid_kernels.hip) -- change both together.
__device__ __forceinline__ uint4 cell_rec_pack(int i, int octave, float x, float y, float ur) {
  return make_uint4((uint32_t)i | ((uint32_t)octave << 24), (uint32_t)__float_as_int(x), (uint32_t)__float_as_int(y), (uint32_t)__float_as_int(ur));
}
struct CellRec { int idx, oct; float x, y, ur; };
__device__ __forceinline__ CellRec cell_rec_unpack(const uint4 rec) {
  return {(int)(rec.x & 0xFFFFFFu), (int)(rec.x >> 24), __int_as_float((int)rec.y), __int_as_float((int)rec.z), __int_as_float((int)rec.w)};
}

// Enumerates, in the reference's order, the keypoints GetFeaturesInArea returns for query q that also pass the
// matcher's stereo gate, and calls fn(rank, idx, dist) for each, wave-cooperatively: a chunk of up to 64
// consecutive grid entries is tested per step, survivors get consecutive ranks.  Returns the survivor count.
// GATE 0: the matcher's stereo gate |u_r - mvuRight| <= radius (SearchByProjection); 1: none (Fuse(Sim3), SearchBySim3);
// 2: Fuse's chi-square reprojection gate (L/src/ORBmatcher.cc:833-854) with inv_sigma2 = mvInvLevelSigma2
template <int GATE = 0, typename Fn>
__device__ __forceinline__ int enumerate_window(const FrameBatch& F, int f, const orbfe_query& q, const uint4 q0,
                                                const uint4 q1, Fn fn, const float* inv_sigma2 = nullptr) {
  const int lane = threadIdx.x & (WAVE - 1);
  const float x = q.u, y = q.v, r = q.radius;
  const int nMinCellX = max(0, (int)floorf((x - F.min_x - r) * F.gw_inv));
  if (nMinCellX >= ORBFE_GRID_COLS) return 0;
  const int nMaxCellX = min(ORBFE_GRID_COLS - 1, (int)ceilf((x - F.min_x + r) * F.gw_inv));
  if (nMaxCellX < 0) return 0;
  const int nMinCellY = max(0, (int)floorf((y - F.min_y - r) * F.gh_inv));
  if (nMinCellY >= ORBFE_GRID_ROWS) return 0;
  const int nMaxCellY = min(ORBFE_GRID_ROWS - 1, (int)ceilf((y - F.min_y + r) * F.gh_inv));
  if (nMaxCellY < 0) return 0;
  const bool bCheckLevels = (q.min_level > 0) || (q.max_level >= 0);
  const uint8_t* desc = F.desc + (size_t)f * F.cap * 32;
  const bool has_ur = F.u_right != nullptr;
  const int32_t* cs = F.cell_start + (size_t)f * (GRID_CELLS + 1);
  const uint4* cr = reinterpret_cast<const uint4*>(F.cell_rec) + (size_t)f * F.cap;
  // The window's cells of one grid column (ix, nMinCellY..nMaxCellY) are adjacent in CSR order.  Lane c fetches
  // column c's range; the ranges are concatenated (prefix sum) into one flat candidate sequence -- column-major, then
  // cell row, then ascending index: the reference's enumeration order -- that the wave consumes 64 entries at a time.
  const int ncol = __builtin_amdgcn_readfirstlane(nMaxCellX - nMinCellX + 1);  // <= 64; the query is wave-uniform
  int e0c = 0, cntc = 0;
  if (lane < ncol) {
    const int ix = nMinCellX + lane;
    e0c = cs[ix * ORBFE_GRID_ROWS + nMinCellY];
    cntc = cs[ix * ORBFE_GRID_ROWS + nMaxCellY + 1] - e0c;
  }
  const int inclc = wave_incl_scan_i(cntc);
  const int exclc = inclc - cntc;
  const int n_entries = __builtin_amdgcn_readlane(inclc, WAVE - 1);
  int rank0 = 0;
  for (int base = 0; base < n_entries; base += WAVE) {
    const int t = base + lane;
    int ent = -1;
    for (int c = 0; c < ncol; c++) {
      const int oc = __builtin_amdgcn_readlane(exclc, c), nc = __builtin_amdgcn_readlane(cntc, c), ec = __builtin_amdgcn_readlane(e0c, c);
      if (t >= oc && t < oc + nc) ent = ec + (t - oc);
    }
    bool ok = false;
    int idx = 0, oct = 0;
    if (ent >= 0) {
      const CellRec k = cell_rec_unpack(cr[ent]);
      idx = k.idx;
      oct = k.oct;
      const float kx = k.x, ky = k.y, kur = k.ur;
      ok = true;
      if (bCheckLevels) {
        if (oct < q.min_level) ok = false;
        if (q.max_level >= 0 && oct > q.max_level) ok = false;
      }
      const float distx = kx - x, disty = ky - y;
      if (!(fabsf(distx) < r && fabsf(disty) < r)) ok = false;
      if (GATE == 0) {
        if (ok && has_ur) {
          const float u = kur;
          if (u > 0) {
            const float er = fabsf(q.u_r - u);
            if (er > r) ok = false;
          }
        }
      } else if (GATE == 2) {
        if (ok) {
          const float kpr = kur;   // -1 without mvuRight
          const float ex = x - kx, ey = y - ky;
          const float invs = inv_sigma2[oct & (ORBFE_MAX_LEVELS - 1)];   // the mask only guards memory
          if (kpr >= 0) {
            const float er = q.u_r - kpr;
            const float e2 = ex * ex + ey * ey + er * er;
            if ((double)(e2 * invs) > 7.8) ok = false;
          } else {
            const float e2 = ex * ex + ey * ey;
            if ((double)(e2 * invs) > 5.99) ok = false;
          }
        }
      }
    }
    const unsigned long long m = __ballot(ok);
    if (ok) {
      uint4 d0, d1;
      load_desc(desc + (size_t)idx * 32, d0, d1);
      const int rank = rank0 + __popcll(m & ((1ull << lane) - 1ull));
      fn(rank, idx, hamming256(q0, q1, d0, d1), oct);
    }
    rank0 += __popcll(m);
  }
  return rank0;
}

// glibc 2.35 logf (__logf_data, LOGF_TABLE_BITS = 4): {invc, logc} pairs.  Same constants as the oracle's oo_logf; the
// arithmetic below is the same double sequence (compiled with -ffp-contract=off).
static __device__ const double g_logf_tab[32] = {
    0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2, 0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2,
    0x1.49539f0f010b0p+0, -0x1.01eae7f513a67p-2, 0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3,
    0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3, 0x1.25e227b0b8ea0p+0, -0x1.1aa2bc79c8100p-3,
    0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4, 0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4,
    0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5, 0x1.0000000000000p+0, 0x0.0p+0,
    0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5,  0x1.ca4b31f026aa0p-1, 0x1.c5e53aa362eb4p-4,
    0x1.b2036576afce6p-1, 0x1.526e57720db08p-3,  0x1.9c2d163a1aa2dp-1, 0x1.bc2860d224770p-3,
    0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2,  0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2};

// MapPoint::PredictScale.  Inputs logf does not map to a finite value (ratio 0, subnormal, inf, nan, negative) make the
// reference's float->int conversion produce INT_MIN on x86-64 (cvttss2si), hence level 0 after the clamp.
__device__ __forceinline__ int predict_scale(float max_distance, float dist, float log_scale_factor, int n_levels) {
  const float ratio = max_distance / dist;
  const uint32_t ix = __float_as_uint(ratio);
  float l;
  if (ix == 0x3f800000u) {
    l = 0.0f;
  } else if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
    return 0;
  } else {
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> 19) & 15u);
    const int k = (int32_t)tmp >> 23;
    const uint32_t iz = ix - (tmp & (0x1ffu << 23));
    const double z = (double)__uint_as_float(iz);
    const double r = z * g_logf_tab[2 * i] - 1.0;
    const double y0 = g_logf_tab[2 * i + 1] + (double)k * 0x1.62e42fefa39efp-1;
    const double r2 = r * r;
    double y = 0x1.5575b0be00b6ap-2 * r + -0x1.ffffef20a4123p-2;
    y = -0x1.00ea348b88334p-2 * r2 + y;
    y = y * r2 + (y0 + r);
    l = (float)y;
  }
  const float c = ceilf(l / log_scale_factor);
  if (!(c >= -2147483648.0f && c < 2147483648.0f)) return 0;  // INT_MIN -> clamped to 0
  int nScale = (int)c;
  if (nScale < 0) nScale = 0;
  else if (nScale >= n_levels) nScale = n_levels - 1;
  return nScale;
}

// ---- projection prologue of Fuse / Fuse(Sim3) / SearchBySim3 / SearchByProjection(KF,Scw) / SearchByProjection(Frame,KF,...)
// (L/src/ORBmatcher.cc:785-816, 925-977, 1075-1113 & 1155-1192, 296-345, 1406-1437) for one candidate map point.  Every
// float expression is written in the operation order of the mode's reference lines (`1 / z` is a float division, `1.0 / z` a
// double one; Fuse multiplies X * invz first, the relocalisation search fx * xc first); cv::Mat products are the small-matrix
// gemm (float dot, double alpha/beta epilogue), cv::norm / Mat::dot accumulate in double -- as in frustum_queries_kernel.
// `cam` is the caller's LDS copy of the record: a by-value copy indexed with the per-lane level lives in scratch memory (DESIGN
// lesson 58).  q comes in zeroed and res as a skipped point's row (-1, 256, -1, 0, 0, 0); a point that no gate rejects fills both.
__device__ __forceinline__ void kf_project(const orbfe_kf_camera& cam, const orbfe_kf_point& mp, int mode, orbfe_query& q,
                                           orbfe_kf_result& res) {
  if (mp.skip) return;
  float Pc[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float t = cam.R[3 * r] * mp.pos[0] + cam.R[3 * r + 1] * mp.pos[1] + cam.R[3 * r + 2] * mp.pos[2];
    Pc[r] = (float)((double)t * 1.0 + (double)cam.t[r] * 1.0);
  }
  if (mode == ORBFE_KF_SIM3) {   // p3Dc2 = sR21 * p3Dc1 + t21 (:1075) / p3Dc1 = sR12 * p3Dc2 + t12 (:1155)
    float P2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const float t = cam.R2[3 * r] * Pc[0] + cam.R2[3 * r + 1] * Pc[1] + cam.R2[3 * r + 2] * Pc[2];
      P2[r] = (float)((double)t * 1.0 + (double)cam.t2[r] * 1.0);
    }
    Pc[0] = P2[0]; Pc[1] = P2[1]; Pc[2] = P2[2];
  }
  bool ok = mode == ORBFE_KF_RELOC || !(Pc[2] < 0.0f);   // "Depth must be positive"; the relocalisation search has no such test
  float invz = 0.f, u = 0.f, v = 0.f;
  if (ok) {
    if (mode == ORBFE_KF_FUSE || mode == ORBFE_KF_LOOP) invz = 1.0f / Pc[2];        // `1 / z`   (:797, :317)
    else invz = (float)(1.0 / (double)Pc[2]);                                        // `1.0 / z` (:945, :1083, :1163, :1413)
    if (mode == ORBFE_KF_RELOC) {                                                    // fx * xc * invzc + cx (:1415-1416)
      u = cam.fx * Pc[0] * invz + cam.cx;
      v = cam.fy * Pc[1] * invz + cam.cy;
      ok = !(u < cam.min_x || u > cam.max_x) && !(v < cam.min_y || v > cam.max_y);   // :1418-1421
    } else {                                                                         // x = X * invz; u = fx * x + cx
      const float x = Pc[0] * invz, y = Pc[1] * invz;
      u = cam.fx * x + cam.cx;
      v = cam.fy * y + cam.cy;
      ok = u >= cam.min_x && u < cam.max_x && v >= cam.min_y && v < cam.max_y;       // KeyFrame::IsInImage (KeyFrame.cc:569-571)
    }
  }
  if (!ok) return;
  const float maxDistance = 1.2f * mp.max_distance, minDistance = 0.8f * mp.min_distance;   // Get{Max,Min}DistanceInvariance
  double s = 0.0, dot = 0.0;
  if (mode == ORBFE_KF_SIM3) {
#pragma unroll
    for (int k = 0; k < 3; k++) s += (double)Pc[k] * (double)Pc[k];   // cv::norm(p3Dc2) (:1097)
  } else {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float PO = mp.pos[k] - cam.Ow[k];
      s += (double)PO * (double)PO;
      dot += (double)PO * (double)mp.normal[k];
    }
  }
  const float dist3D = (float)sqrt(s);
  ok = !(dist3D < minDistance || dist3D > maxDistance);
  if (ok && (mode == ORBFE_KF_FUSE || mode == ORBFE_KF_FUSE_SIM3 || mode == ORBFE_KF_LOOP))
    ok = !(dot < 0.5 * (double)dist3D);   // "Viewing angle must be less than 60 deg": PO.dot(Pn) < 0.5 * dist
  if (!ok) return;
  const int level = predict_scale(mp.max_distance, dist3D, cam.log_scale_factor, cam.n_levels);
  q.u = u; q.v = v;
  q.u_r = u - cam.mbf * invz;   // Fuse :808
  q.radius = cam.th * cam.scale_factors[level];
  q.min_level = level - 1;
  q.max_level = mode == ORBFE_KF_RELOC ? level + 1 : level;
  q.valid = 1;
  q.blocks = 1;
  q.angle = mp.angle;
#pragma unroll
  for (int j = 0; j < 8; j++) reinterpret_cast<uint32_t*>(q.desc)[j] = reinterpret_cast<const uint32_t*>(mp.desc)[j];
  res.level = level; res.u = u; res.v = v; res.u_r = q.u_r;
}
