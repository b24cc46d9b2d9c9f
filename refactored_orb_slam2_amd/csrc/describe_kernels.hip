// describe_kernels.hip -- the orientation and descriptor stage of the ORB extractor for gfx950 (MI355X, wave64).
//
// orient_describe   IC_Angle + computeOrbDescriptor + pt*=scale          L/src/ORBextractor.cc:76-146,1028-1035
// (reference file:line, L/ = Source/Libraries/ORB_SLAM2/)
//
// All arithmetic that decides an output bit is integer, or float/double evaluated exactly as the x86-64
// reference build does (no FMA contraction: this file is compiled with -ffp-contract=off; IEEE divide).
#include <stdlib.h>
#include <string.h>

#include "orbfe_internal.h"
#include "extract_device.h"
#include "../../include/orb_pattern_data.h"

// ------------------------------------------------------------------------------------------------ describe
// the same pattern as floats, one (x0, y0, x1, y1) record per test pair (filled at start-up by the host)
__device__ __attribute__((aligned(16))) float g_pattern_f[1024];

// cv::fastAtan2 (degrees), scalar OpenCV path, float, un-fused
__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
  const float scale = (float)(180.0 / 3.1415926535897932384626433832795);
  const float p1 = 0.9997878412794807f * scale;
  const float p3 = -0.3258083974640975f * scale;
  const float p5 = 0.1555786518463281f * scale;
  const float p7 = -0.04432655554792128f * scale;
  const float eps = (float)2.2204460492503131e-16;
  const float ax = fabsf(x), ay = fabsf(y);
  float a, c, c2;
  if (ax >= ay) {
    c = ay / (ax + eps);
    c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    c = ax / (ay + eps);
    c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

// glibc 2.35 sinf/cosf (flt-32/s_sincosf.h) restated: double reduction by pi/2, two double polynomials,
// one rounding to float.  Valid for |x| < 120 (angles here are in [0, 2*pi]).
__device__ __forceinline__ float sc_poly(double x, double x2, int n, bool flip) {
  const double C0 = 0x1p0, C1 = -0x1.ffffffd0c621cp-2, C2 = 0x1.55553e1068f19p-5, C3 = -0x1.6c087e89a359dp-10,
               C4 = 0x1.99343027bf8c3p-16;
  const double S1 = -0x1.555545995a603p-3, S2 = 0x1.1107605230bc4p-7, S3 = -0x1.994eb3774cf24p-13;
  if ((n & 1) == 0) {
    const double x3 = x * x2;
    const double s1 = S2 + x2 * S3;
    const double x7 = x3 * x2;
    const double s = x + x3 * S1;
    return (float)(s + x7 * s1);
  } else {
    const double sg = flip ? -1.0 : 1.0;
    const double x4 = x2 * x2;
    const double c2 = sg * C3 + x2 * (sg * C4);
    const double c1 = sg * C1 + x2 * (sg * C2);
    const double x6 = x4 * x2;
    const double c = sg * C0 + x2 * c1;
    return (float)(c + x6 * c2);
  }
}
__device__ __forceinline__ void glibc_sincosf(float y, float* sn, float* cs) {
  double x = (double)y;
  const uint32_t top = (__float_as_uint(y) >> 20) & 0x7ff;
  if (top < 0x3f4) {  // |y| < pi/4  (abstop12(0x1.921FB6p-1f) = 0x3f4)
    const double x2 = x * x;
    if (top < 0x398) {  // |y| < 2^-12
      *sn = y;
      *cs = 1.0f;
      return;
    }
    *sn = sc_poly(x, x2, 0, false);
    *cs = sc_poly(x, x2, 1, false);
    return;
  }
  const double r = x * 0x1.45F306DC9C883p+23;
  const int n = ((int32_t)r + 0x800000) >> 24;
  x = x - (double)n * 0x1.921FB54442D18p0;
  const double s = ((n + 1) & 2) ? -1.0 : 1.0;  // sign table {1,-1,-1,1}[n&3]
  const bool flip = (n & 2) != 0;
  const double xs = x * s, x2 = x * x;
  *sn = sc_poly(xs, x2, n, flip);
  *cs = sc_poly(xs, x2, n ^ 1, flip);
}

// LDS staging of a keypoint's two patches: the raw 31 x 31 window of IC_Angle and the blurred 37 x 37 window of the pattern
#ifndef ORI_PITCH
#define ORI_PITCH 48   // 3 x 16 B: (cx - 15) & 15 <= 15, 15 + 31 <= 48
#endif
#ifndef DSC_PITCH
#define DSC_PITCH 64   // 4 x 16 B: 15 + 37 <= 64
#endif
// The windows go global -> LDS directly (global_load_lds_dwordx4), two buffers per wave.
#define OD_BUF (37 * DSC_PITCH)                            // 2368: one LDS buffer holds either window
#define PATCH_BYTES (2 * OD_BUF)                           // 4736
// lane l's 16 bytes land at lds_dst + 16 l: the windows' LDS images are exactly that order -- raw patch 31 rows x 3 pieces at pitch 48,
// blurred patch 37 rows x 4 pieces at pitch 64 or x 3 pieces at pitch 48 (piece i = row * pieces + column at byte 16 i).  The compiler
// does not count these loads: every wait for them is an explicit s_waitcnt vmcnt below.
// The address is a 32-bit byte offset per lane on a wave-uniform 64-bit plane address (no 64-bit vector add per piece).  M0 is
// written and not restored -- the compiler keeps nothing in M0 in this kernel (tests/test_describe_isa.py reads the listing for that) --
// and, in the second form, only the lanes of `mask` requesting: EXEC is narrowed around the load, without a branch.  The padding
// gives the five wait states a plane address fresh from v_readlane needs before a memory instruction reads it (the M0 write and the
// EXEC write count as one each; the M0 write needs one before the load).
#define OD_DMA_S(voff, sbase, lds_dst) \
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory")
#define OD_DMA_SM(voff, sbase, lds_dst, mask) do { \
    unsigned long long keep_exec; \
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 2\n\ts_and_saveexec_b64 %0, %4\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b64 exec, %0" \
                 : "=&s"(keep_exec) : "v"(voff), "s"(sbase), "s"(lds_dst), "s"(mask) : "memory", "scc"); \
  } while (0)

// ---- orientation + description, eight keypoints per wave ------------------------------------------------------------------
// The per-keypoint work has two kinds of instructions: cooperative ones (patch staging, the 749-pixel moment sums, the 256
// rotated comparisons) and wave-uniform ones (level bookkeeping, fastAtan2, the double-precision sin / cos: ~130 of the ~380
// instructions of a wave-per-keypoint kernel, each of them computing ONE value on 64 lanes).  Here a wave takes eight consecutive
// keypoint slots: phase 1 stages each raw 31 x 31 patch and leaves the keypoint's moments in lane k; phase 2 evaluates
// fastAtan2 / sinf / cosf once, lane k for keypoint k; phase 3 stages each blurred 37 x 37 patch and samples the pattern with
// (a, b) read from lane k.  The moments use v_dot4_i32_i8: a lane owns four (row, 4-column) items of the disc, the per-item
// weights (u and v as signed bytes, 0 outside the disc; a host-filled table) stay in registers for all eight keypoints, and the
// pixels enter as I - 128 (one xor per dword).  The disc is symmetric, sum u = sum v = 0, so sum u (I - 128) = sum u I = m10
// exactly -- integer, hence the same moments as the reference's loops -- and no sum of I is needed: two sums per keypoint instead
// of three, folded to eight-lane groups per keypoint and finished for all eight keypoints together (profiles/r07_describe.md).
// Nothing a loop iteration needs of its keypoint is looked up in it: lane k resolves slot k's planes, window origins and LDS
// geometry once per wave, and the loops read them with v_readlane (DESIGN lesson 60).
#ifndef OD_K
#define OD_K 8
#endif
#if FC_TIMING
__device__ unsigned long long g_od_prof[4096 * 8];
extern "C" int orbfe_debug_od_profile(unsigned long long* out, int reset) {
  static unsigned long long h[4096 * 8];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_od_prof), sizeof(h)) != hipSuccess) return 1;
  for (int i = 0; i < 8; i++) out[i] = 0;
  for (int sl = 0; sl < 4096; sl++)
    for (int i = 0; i < 8; i++) out[i] += h[sl * 8 + i];
  if (reset) { memset(h, 0, sizeof(h)); if (hipMemcpyToSymbol(HIP_SYMBOL(g_od_prof), h, sizeof(h)) != hipSuccess) return 1; }
  return 0;
}
#endif
__device__ __attribute__((aligned(16))) uint32_t g_ic_w[256 * 2];   // [item][u-weights | v-weights] (int8 x 4), item = row * 8 + 4-column group
#ifndef OD_WGS
#define OD_WGS 7   // workgroups (= waves per SIMD) resident per CU: the register budget the compiler is given and the LDS padding below
#endif
__global__ __launch_bounds__(256, OD_WGS) void orient_describe8_kernel(DescribeParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t patch[4][PATCH_BYTES];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv_id = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int bx = blockIdx.x, img = blockIdx.y;
  if (P.xcd_images) {   // whole images per XCD (XCD k takes images k, k + 8, ...): the planes one image's patches are gathered from stay in one L2
    const unsigned gx = gridDim.x;
    const unsigned lin = blockIdx.y * gx + blockIdx.x;
    const unsigned grp = lin / (8u * gx);
    if (8u * grp + 8u <= gridDim.y) {
      const unsigned within = lin - grp * 8u * gx;
      img = (int)(8u * grp + (within & 7u));
      bx = (int)(within >> 3);
    }
  }
#if FC_TIMING
  uint32_t tacc0 = 0, tacc1 = 0, tacc2 = 0, tacc3 = 0, tacc4 = 0, tacc5 = 0, tprev = (uint32_t)__builtin_readcyclecounter();
#endif
  const int s0 = (bx * 4 + wv_id) * OD_K;
  const int32_t* ln = P.lvl_n + (size_t)img * ORBFE_MAX_LEVELS;
  if (s0 >= P.kp_per_image) return;
  // Everything the prologue needs is requested before anything is waited for: the level counts (lane l holds ln[l]), the
  // slot's packed record, the pattern and the moment weights.  (A store in front of these loads, or a load per loop
  // iteration, serialised four or five memory round trips here: a fifth of the kernel's time, tools/fc_phase_profile.py.)
  const int ln_lane = lane < P.n_levels ? ln[lane] : 0;
  const int slot_c = min(s0 + (lane & (OD_K - 1)), P.kp_per_image - 1);
  const uint32_t e_lane = P.lvl_kp[(size_t)img * P.kp_per_image + slot_c];
  float4 pk[4];
#pragma unroll
  for (int r = 0; r < 4; r++) pk[r] = *reinterpret_cast<const float4*>(&g_pattern_f[(r * 64 + lane) * 4]);
  uint32_t wu[4], wv[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int it = lane + WAVE * j;   // items >= 248 carry zero weights
    const uint2 w2 = reinterpret_cast<const uint2*>(g_ic_w)[it];
    wu[j] = w2.x; wv[j] = w2.y;
  }

  // slot bookkeeping, lane k for slot s0 + k: level, position, score and output index (-1 = no keypoint in this slot)
  int i_out = -1, i_level = 0, i_cx = 0, i_cy = 0, i_score = 0;
  unsigned long long pl_rbase, pl_bbase;   // this image's raw / blurred plane of that level
  int pl_rpitch, pl_bpitch;
  uint32_t pl_rtiled;
  float pl_scale, pl_size;
  {
    const int slot = s0 + lane;
    int level = 0, off_level = 0;
    for (int l = 1; l < P.n_levels; l++) {   // kp_off ascends; it lives in the kernel arguments (scalar registers)
      const bool ge = slot >= P.kp_off[l];
      level += ge ? 1 : 0;
      off_level = ge ? P.kp_off[l] : off_level;
    }
    // Plane lookup, once per wave: lane k fetches what slot k's two windows and its keypoint record need of its level -- vector loads
    // from the kernel-argument segment, requested with the batch above.  The loops below read them with v_readlane: no scalar load,
    // no wait for one and no 64-bit image multiply per keypoint (they were redone for every window, sixteen times per wave).
    pl_rbase = reinterpret_cast<unsigned long long>(P.pyr.base[level]) + (unsigned long long)img * P.pyr.img_stride[level];
    pl_bbase = reinterpret_cast<unsigned long long>(P.blur.base[level]) + (unsigned long long)img * P.blur.img_stride[level];
    pl_rpitch = P.pyr.pitch[level];
    pl_bpitch = P.blur.pitch[level];
    pl_rtiled = (P.pyr.tiled >> level) & 1u;
    pl_scale = P.scale[level];
    pl_size = P.kp_size[level];
    const int idx = slot - off_level;
    int out = idx, ln_level = 0;
    for (int l = 0; l < P.n_levels; l++) {
      const int lnl = __builtin_amdgcn_readlane(ln_lane, l);
      out += l < level ? lnl : 0;
      ln_level = l == level ? lnl : ln_level;
    }
    if (lane < OD_K && slot < P.kp_per_image && idx < ln_level && out < P.cap) {
      const uint32_t e = e_lane;
      i_out = out; i_level = level;
      i_cx = (int)(e & 0xfff) + ORBFE_EDGE; i_cy = (int)((e >> 12) & 0xfff) + ORBFE_EDGE; i_score = (int)(e >> 24);
    }
    if (s0 == 0 && lane == 0) {   // the image's keypoint count = sum of the level counts
      int tot = 0;
      for (int l = 0; l < P.n_levels; l++) tot += __builtin_amdgcn_readlane(ln_lane, l);
      P.out_n[img] = tot;
    }
  }
  const unsigned valid_mask = (unsigned)(__ballot(i_out >= 0) & ((1ull << OD_K) - 1ull));
  if (valid_mask == 0) return;
  FC_T(0);   // tables + slot bookkeeping
  const int k_first = __ffs((int)valid_mask) - 1;

  // Everything a window request needs of its keypoint is wave-uniform, so lane k works it out for slot k here, eight slots at the
  // price of one, and the loops fetch it with v_readlane.
  //   raw window: pieces (row r, 16-byte column c) at  base + (y >> 3) * mA + (y & 7) * mB + c * cs,  y = cy - 15 + r,  one form for both
  //   storages -- tiled (16 x 8-pixel tiles of 128 bytes): mA = 128 * tiles per tile row, mB = 16, cs = 128; row-major: mA = 8 * pitch,
  //   mB = pitch, cs = 16 -- with the window's first column already in the base.
  //   blurred window (always tiled): base + (y >> 3) * mA + (y & 7) * 16 + x16 * 128, y and x16 clamped at 0 (the window may begin two
  //   rows above and one piece left of the plane; those bytes are never sampled).
  const uint32_t r_mA = pl_rtiled ? (uint32_t)(pl_rpitch >> 4) << 7 : (uint32_t)pl_rpitch << 3;
  const uint32_t r_mB = pl_rtiled ? 16u : (uint32_t)pl_rpitch;
  const uint32_t r_cs = pl_rtiled ? 128u : 16u;
  const unsigned long long r_base = pl_rbase + (unsigned long long)((uint32_t)((i_cx - 15) >> 4) * r_cs);
  const int r_blo = (int)(uint32_t)r_base, r_bhi = (int)(uint32_t)(r_base >> 32);
  const int r_y0 = i_cy - 15;
  const int r_m = (i_cx - 15) & 15;   // the window's first column inside its first piece
  const int b_lo = (int)(uint32_t)pl_bbase, b_hi = (int)(uint32_t)(pl_bbase >> 32);
  const uint32_t b_mA = (uint32_t)(pl_bpitch >> 4) << 7;
  const int b_x16 = (i_cx - 18) >> 4, b_y0 = i_cy - 18;
  const int b_wide = ((i_cx - 18) & 15) > 11 ? 1 : 0;   // 37 columns from there need a fourth piece
  // lane -> (row, piece) of a window of three pieces per row (rounds 0 and 1) and of four (row + 16 per round)
  const int rN0 = (lane * 43) >> 7, cN0 = lane - 3 * rN0;                  // i / 3, i % 3 for i < 128
  const int rN1 = ((lane + WAVE) * 43) >> 7, cN1 = lane + WAVE - 3 * rN1;
  const int rW = lane >> 2, cW = lane & 3;
#define OD_RL(v, k) __builtin_amdgcn_readlane((v), (k))
#define OD_RL64(lo, hi, k) (((unsigned long long)(uint32_t)OD_RL(hi, k) << 32) | (unsigned long long)(uint32_t)OD_RL(lo, k))
  const uint32_t lds_buf = (uint32_t)(uintptr_t)&patch[wv_id][0];
  // ---- phase 1: moments of the keypoints, keypoint k's in lane k.  The window of keypoint k + 1 travels global -> LDS (the other
  // buffer) while k's is summed: no staging registers, no LDS store instructions, no wait between a load's arrival and its store.
  auto dma_ori = [&](int k, uint32_t lds) {   // 31 x 3 pieces: one full round, 29 lanes of a second
    const unsigned long long base = OD_RL64(r_blo, r_bhi, k);
    const uint32_t mA = (uint32_t)OD_RL((int)r_mA, k), mB = (uint32_t)OD_RL((int)r_mB, k), cs = (uint32_t)OD_RL((int)r_cs, k);
    const int y0 = OD_RL(r_y0, k);
    const uint32_t ya = (uint32_t)(y0 + rN0), yb = (uint32_t)(y0 + rN1);
    const uint32_t oa = __umul24(ya >> 3, mA) + __umul24(ya & 7u, mB) + __umul24((uint32_t)cN0, cs);
    const uint32_t ob = __umul24(yb >> 3, mA) + __umul24(yb & 7u, mB) + __umul24((uint32_t)cN1, cs);
    OD_DMA_S(oa, base, lds);
    OD_DMA_SM(ob, base, lds + 1024u, (1ull << (31 * 3 - WAVE)) - 1ull);
  };
  // The moment sums, batched: a keypoint's 64 lane-local partial sums are only folded to one per group of eight lanes (three
  // v_add_dpp per sum; every step leaves all lanes of the group holding the group's total) and lane 8 g + k keeps group g's total of
  // keypoint k.  The eight keypoints' groups are added up together behind the loop.  (A six-step scan and a v_readlane per sum, twice
  // per keypoint, were 28 instructions that produced one value each.)  Integer sums: the same integers in any order.
  int accA = 0, accB = 0;
  {
    // every load the compiler knows of (pattern, weights, slot records, plane constants) has arrived before the loop: it does not see
    // the LDS-DMA loads, and would otherwise wait for "its" loads inside the loops below -- with a count that also drains the
    // window that was just requested (s_waitcnt vmcnt(0), expcnt / lgkmcnt untouched)
    dma_ori(k_first, lds_buf);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    unsigned rem = valid_mask & (valid_mask - 1u);   // the slots behind k
    uint32_t par = 0;
    for (int k = k_first;; par ^= 1u) {
      const int kn = __builtin_ctz(rem | (1u << OD_K));   // the next slot that holds a keypoint (OD_K: none)
      const bool more = kn < OD_K;
      rem &= rem - 1u;
      // (the buffer the next window lands in was last read two keypoints ago; those reads were consumed before that iteration ended.
      //  Three buffers with the windows of k + 1 AND k + 2 in flight: 0.269 ms against 0.262 -- more requests in flight are not faster)
      if (more) {
        dma_ori(kn, lds_buf + (par ^ 1u) * OD_BUF);
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");   // everything older than the two loads just issued: this keypoint's window
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      FC_T(1);   // wait for the raw patch
      const uint8_t* ob = &patch[wv_id][0] + par * OD_BUF;
      const int m = OD_RL(r_m, k);
      int A = 0, B = 0;
      const uint32_t sh = (uint32_t)(m & 3);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int it = lane + WAVE * j;
        const int r = it >> 3, c = it & 7;
        const uint32_t* q = reinterpret_cast<const uint32_t*>(ob + (r < 31 ? r : 30) * ORI_PITCH + ((m + 4 * c) & ~3));
        // the four pixels u = -15 + 4c .. -12 + 4c of row v = r - 15, as I - 128
        const int px = (int)(__builtin_amdgcn_alignbyte(q[1], q[0], sh) ^ 0x80808080u);
        A = __builtin_amdgcn_sdot4(px, (int)wu[j], A, false);
        B = __builtin_amdgcn_sdot4(px, (int)wv[j], B, false);
      }
      A += __builtin_amdgcn_update_dpp(0, A, 0xB1, 0xf, 0xf, false);    // quad_perm:[1,0,3,2]
      B += __builtin_amdgcn_update_dpp(0, B, 0xB1, 0xf, 0xf, false);
      A += __builtin_amdgcn_update_dpp(0, A, 0x4E, 0xf, 0xf, false);    // quad_perm:[2,3,0,1]: every lane holds its quad's sum
      B += __builtin_amdgcn_update_dpp(0, B, 0x4E, 0xf, 0xf, false);
      A += __builtin_amdgcn_update_dpp(0, A, 0x141, 0xf, 0xf, false);   // row_half_mirror: a lane of the group's other quad
      B += __builtin_amdgcn_update_dpp(0, B, 0x141, 0xf, 0xf, false);
      const bool mine = (lane & 7) == k;
      accA = mine ? A : accA;
      accB = mine ? B : accB;
      FC_T(2);   // moments
      if (!more) break;
      k = kn;
    }
  }
  // ---- phase 2: lane k computes keypoint k's angle and rotation; the first blurred patch is already on its way
  auto dma_dsc = [&](int k, uint32_t lds, bool wide) {
    // 37 x 3 pieces (one round and 47 lanes) where the window's 37 columns end inside the third 16-byte piece, 37 x 4 (two rounds and 20
    // lanes) otherwise -- the kernel is bound by the texture addresser (TA / TD / TCP 0.95-0.99 busy), i.e. by pieces requested, and three
    // keypoints of four take the narrow form.  One code path for the first two rounds: the lane -> (row, piece) map is selected by the
    // wave-uniform flag
    const unsigned long long base = OD_RL64(b_lo, b_hi, k);
    const uint32_t mA = (uint32_t)OD_RL((int)b_mA, k);
    const int x16 = OD_RL(b_x16, k), y0 = OD_RL(b_y0, k);
    const uint32_t xc = (uint32_t)max(x16 + (wide ? cW : cN0), 0), xd = (uint32_t)max(x16 + (wide ? cW : cN1), 0);
    const uint32_t ya = (uint32_t)max(y0 + (wide ? rW : rN0), 0), yb = (uint32_t)max(y0 + (wide ? rW + 16 : rN1), 0);
    const uint32_t oa = __umul24(ya >> 3, mA) + ((ya & 7u) << 4) + (xc << 7);
    const uint32_t ob = __umul24(yb >> 3, mA) + ((yb & 7u) << 4) + (xd << 7);
    OD_DMA_S(oa, base, lds);
    OD_DMA_SM(ob, base, lds + 1024u, wide ? ~0ull : (1ull << (37 * 3 - WAVE)) - 1ull);
    if (wide) {   // (wave-uniform: the third round exists only for the wide window)
      const uint32_t ye = (uint32_t)max(y0 + rW + 32, 0);
      const uint32_t oe = __umul24(ye >> 3, mA) + ((ye & 7u) << 4) + (xc << 7);
      OD_DMA_SM(oe, base, lds + 2048u, (1ull << (37 * 4 - 2 * WAVE)) - 1ull);
    }
  };
  bool wide_k = OD_RL(b_wide, k_first) != 0;
  dma_dsc(k_first, lds_buf, wide_k);
  // the four row groups of a keypoint's eight-lane totals: the other group of the row, then the other rows (through the LDS crossbar,
  // no LDS memory).  Once per wave, for all eight keypoints and both sums
  accA += __builtin_amdgcn_update_dpp(0, accA, 0x128, 0xf, 0xf, false);   // row_ror:8
  accB += __builtin_amdgcn_update_dpp(0, accB, 0x128, 0xf, 0xf, false);
  accA += __builtin_amdgcn_ds_bpermute((lane ^ 16) << 2, accA);
  accB += __builtin_amdgcn_ds_bpermute((lane ^ 16) << 2, accB);
  accA += __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, accA);
  accB += __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, accB);
  const int m10v = accA, m01v = accB;   // lane k (and every lane 8 g + k): keypoint k's moments
  const float angle_v = fast_atan2_deg((float)m01v, (float)m10v);
  const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
  float a_v, b_v;
  glibc_sincosf(angle_v * factorPI, &b_v, &a_v);
  // the keypoint record: lane k writes keypoint k's seven words here, not seven lanes behind every descriptor (a switch over the lane
  // and two scalar loads per keypoint)
  if (i_out >= 0) {
    float fx = (float)i_cx, fy = (float)i_cy;
    if (i_level != 0) {
      fx *= pl_scale;
      fy *= pl_scale;
    }
    uint32_t* o = reinterpret_cast<uint32_t*>(P.out_kps + (size_t)img * P.cap + i_out);
    o[0] = __float_as_uint(fx);
    o[1] = __float_as_uint(fy);
    o[2] = __float_as_uint(pl_size);
    o[3] = __float_as_uint(angle_v);
    o[4] = __float_as_uint((float)i_score);
    o[5] = (uint32_t)i_level;
    o[6] = 0xFFFFFFFFu;
  }
  // the descriptor's address and the window's LDS geometry, lane k for keypoint k.
  // cvRound of the rotated coordinates (L/src/ORBextractor.cc:119-121) by the magic-number addition: v + 1.5 * 2^23 rounds |v| < 2^22
  // to nearest-even in the mantissa's low bits -- one v_add_f32 where v_rndne_f32 + v_cvt_i32_f32 were two.  The integers are never
  // separated from the magic word: its low 24 bits are 2^22 + v, so v_mad_u32_u24 gives (2^22 + ry) * PITCH + (M + rx), the patch index
  // plus a constant that goes into the wave-uniform base.  PITCH, 64 for the wide window and 48 for the narrow one, is an operand of
  // that one instruction: one code path for both.
  const uint32_t MB = 0x4B400000u;   // the magic number's bit pattern
  const uint32_t d_pitch = b_wide ? 64u : 48u;
  const uint32_t d_bc = 18u * d_pitch + 18u + (uint32_t)((i_cx - 18) & 15) - ((1u << 22) * d_pitch + MB);
  const unsigned long long d_out = ((unsigned long long)img * (unsigned)P.cap + (unsigned)max(i_out, 0)) * 32ull;   // byte offset in out_desc
  const int d_olo = (int)(uint32_t)d_out, d_ohi = (int)(uint32_t)(d_out >> 32);
  FC_T(3);   // angle, sin / cos
  // ---- phase 3: steered BRIEF on the blurred level
  {
    const float MAGIC = 12582912.0f;
    const uint32_t sel0 = lane == 0 ? ~0u : 0u, sel1 = lane == 1 ? ~0u : 0u, sel2 = lane == 2 ? ~0u : 0u, sel3 = lane == 3 ? ~0u : 0u;
    unsigned rem = valid_mask & (valid_mask - 1u);
    uint32_t par = 0;
    for (int k = k_first;; par ^= 1u) {
      const int kn = __builtin_ctz(rem | (1u << OD_K));   // the next slot that holds a keypoint (OD_K: none)
      const bool more = kn < OD_K;
      rem &= rem - 1u;
      const float a = __int_as_float(OD_RL(__float_as_int(a_v), k)), b = __int_as_float(OD_RL(__float_as_int(b_v), k));
      const uint32_t pitch = wide_k ? 64u : 48u;
      // the queue holds, oldest first: this keypoint's window, the previous keypoint's descriptor store, then the loads issued here
      if (more) {
        wide_k = OD_RL(b_wide, kn) != 0;
        dma_dsc(kn, lds_buf + (par ^ 1u) * OD_BUF, wide_k);
        if (wide_k) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      FC_T(4);   // wait for the blurred patch
      const uint8_t* dsc = &patch[wv_id][0] + par * OD_BUF;
      const uint32_t bc0 = (uint32_t)OD_RL((int)d_bc, k);
      uint2* dout = reinterpret_cast<uint2*>(P.out_desc + OD_RL64(d_olo, d_ohi, k));
      // all eight samples requested before the first comparison, and the 32 descriptor bytes stored by lanes 0 .. 3 in one instruction
      int t0[4], t1[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float x0 = pk[r].x, y0 = pk[r].y, x1 = pk[r].z, y1 = pk[r].w;
        const uint32_t ry0 = __float_as_uint((x0 * b + y0 * a) + MAGIC), rx0 = __float_as_uint((x0 * a - y0 * b) + MAGIC);
        const uint32_t ry1 = __float_as_uint((x1 * b + y1 * a) + MAGIC), rx1 = __float_as_uint((x1 * a - y1 * b) + MAGIC);
        t0[r] = dsc[bc0 + __umul24(ry0, pitch) + rx0];
        t1[r] = dsc[bc0 + __umul24(ry1, pitch) + rx1];
      }
      {
        const unsigned long long b0 = __ballot(t0[0] < t1[0]), b1 = __ballot(t0[1] < t1[1]), b2 = __ballot(t0[2] < t1[2]), b3 = __ballot(t0[3] < t1[3]);
        // ballot r into lane r with per-lane masks (v_and_or_b32 on the scalar ballots): a conditional expression over the lane became
        // branches around vector moves
        uint2 mine;
        mine.x = ((uint32_t)b0 & sel0) | ((uint32_t)b1 & sel1) | ((uint32_t)b2 & sel2) | ((uint32_t)b3 & sel3);
        mine.y = ((uint32_t)(b0 >> 32) & sel0) | ((uint32_t)(b1 >> 32) & sel1) | ((uint32_t)(b2 >> 32) & sel2) | ((uint32_t)(b3 >> 32) & sel3);
        if (lane < 4) dout[lane] = mine;
      }
      FC_T(5);   // BRIEF + store
      if (!more) break;
      k = kn;
    }
  }
#undef OD_RL
#undef OD_RL64
#if FC_TIMING
  if (lane == 0) {
    unsigned long long* pr = g_od_prof + (size_t)((((unsigned)(bx * 4 + wv_id) + 977u * (unsigned)img) * 2654435761u) >> 20) * 8;
    atomicAdd(&pr[0], (unsigned long long)tacc0); atomicAdd(&pr[1], (unsigned long long)tacc1);
    atomicAdd(&pr[2], (unsigned long long)tacc2); atomicAdd(&pr[3], (unsigned long long)tacc3);
    atomicAdd(&pr[4], (unsigned long long)tacc4); atomicAdd(&pr[5], (unsigned long long)tacc5);
    atomicAdd(&pr[6], 1ull);
    atomicAdd(&pr[7], (unsigned long long)__popc(valid_mask));
  }
#endif
}

// ------------------------------------------------------------------------------------------------ launchers
void orbfe_launch_describe(const DescribeParams& p, int n_images, hipStream_t s) {
  DescribeParams pp = p;
  pp.xcd_images = 1;
  const int per_block = 4 * OD_K;
  dim3 block(256), grid((p.kp_per_image + per_block - 1) / per_block > 0 ? (p.kp_per_image + per_block - 1) / per_block : 1, n_images);
  // 63 VGPRs would let eight waves per SIMD run; the gather of 2 000 patches per image is L2-miss bound and an eighth wave
  // measured slower (0.352 against 0.341 ms per 256 images): unused dynamic LDS keeps a CU at seven workgroups
#ifndef OD_LDS_PAD
// dynamic LDS that brings a workgroup to (160 KB / (OD_WGS + 1) rounded up to 512 B) + 512: OD_WGS workgroups fit a CU, OD_WGS + 1 do not
#define OD_LDS_WG ((((163840 / (OD_WGS + 1)) + 511) & ~511) + 512)
#define OD_LDS_PAD (4 * PATCH_BYTES < OD_LDS_WG ? OD_LDS_WG - 4 * PATCH_BYTES : 0)
#endif
  hipLaunchKernelGGL(orient_describe8_kernel, grid, block, OD_LDS_PAD, s, pp);
}

// The one table upload extractor.cpp calls: the describe tables here, then the blur's band matrices beside their table
// (pyramid_kernels.hip: without relocatable device code a table and the copy that fills it share a unit).  Returns the first error.
int orbfe_upload_pattern_floats() {
  static const int8_t pat[1024] = {ORB_PATTERN_INT8_1024};
  float f[1024];
  for (int i = 0; i < 1024; i++) f[i] = (float)pat[i];
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_pattern_f), f, sizeof(f));
  if (e != hipSuccess) return (int)e;
  // weights of the moment sums: item = row * 8 + group, row v = r - 15, columns u = -15 + 4 * group + t
  // (umax of ORBextractor's constructor for HALF_PATCH_SIZE 15, L/src/ORBextractor.cc:449-463)
  static const int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
  uint32_t wtab[256 * 2];
  memset(wtab, 0, sizeof(wtab));
  for (int it = 0; it < 248; it++) {
    const int v = (it >> 3) - 15;
    for (int t = 0; t < 4; t++) {
      const int u = -15 + 4 * (it & 7) + t;
      const bool inside = u <= 15 && abs(u) <= umax[abs(v)];
      if (!inside) continue;
      wtab[it * 2] |= (uint32_t)(uint8_t)(int8_t)u << (8 * t);
      wtab[it * 2 + 1] |= (uint32_t)(uint8_t)(int8_t)v << (8 * t);
    }
  }
  e = hipMemcpyToSymbol(HIP_SYMBOL(g_ic_w), wtab, sizeof(wtab));
  if (e != hipSuccess) return (int)e;
  return orbfe_upload_blur_bands();
}
