// stereo_kernels.hip -- the stereo association of a rectified pair, for gfx950 (MI355X, wave64).
// Kernel              replaces (reference file:line, L/ = Source/Libraries/ORB_SLAM2/)
// stereo_bucket       the per-row candidate lists vRowIndices, as (row bucket, octave) runs   L/src/Frame.cc:484-502
// stereo_match        Frame::ComputeStereoMatches (Hamming + 11x11 SAD)        L/src/Frame.cc:504-632
// stereo_median       median-based outlier cut                                 L/src/Frame.cc:634-645
// Compiled with -ffp-contract=off: every float expression is evaluated un-fused, as the reference does.
#include "search_device.h"   // WAVE, hamming256, load_desc

// Right keypoints are first binned by the 8-row buckets their band [floor(y-r), ceil(y+r)], r = 2*scale[octave],
// overlaps (one block per pair).  A left keypoint then only visits the bucket of its row (int)vL and re-tests
// the exact band.  The reference walks its per-row lists in ascending right index with a strict "<"
// (L/src/Frame.cc:493-502,536-553): the (distance, index) lexicographic minimum reproduces that first-wins
// rule whatever order the candidates are visited in.
__global__ __launch_bounds__(256) void stereo_bucket_kernel(StereoParams P) {
  // keys = (row bucket, octave), row-bucket major: the entries a left keypoint of level l may match -- octaves l - 1 .. l + 1
  // of its row bucket -- are ONE contiguous run of the CSR array, a third as long as the whole row bucket (39 entries on
  // average at KITTI geometry instead of 104: one 64-lane chunk for 97 % of the left keypoints instead of two to four)
  extern __shared__ int sb_lds[];
  int* cnt = sb_lds;                 // [n_keys]
  int* start = sb_lds + P.n_keys;    // [n_keys + 1]
  __shared__ int part[256];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const int nR = P.nR[pair];
  const int nb = P.n_buckets, nl = P.n_levels, nk = P.n_keys;
  const orbfe_keypoint* kr = P.kpsR + (size_t)pair * P.cap;
  int32_t* bs = P.bucket_start + (size_t)pair * (nk + 1);
  int4* bi = reinterpret_cast<int4*>(P.bucket_idx) + (size_t)pair * P.cap * STEREO_BUCKET_SPAN;
  for (int b = tid; b < nk; b += 256) cnt[b] = 0;
  __syncthreads();
  for (int pass = 0; pass < 2; pass++) {
    for (int iR = tid; iR < nR; iR += 256) {
      const orbfe_keypoint kp = kr[iR];
      const int oct = min(max(kp.octave, 0), nl - 1);
      const float r = 2.0f * P.scale[oct];
      const int maxr = (int)ceilf(kp.y + r), minr = (int)floorf(kp.y - r);
      int b0 = max(minr, 0) >> 3, b1 = min(maxr >> 3, nb - 1);
      if (b1 - b0 >= STEREO_BUCKET_SPAN) b1 = b0 + STEREO_BUCKET_SPAN - 1;  // cannot happen for scale <= 12
      for (int b = b0; b <= b1; b++) {
        const int key = b * nl + oct;
        const int pos = atomicAdd(&cnt[key], 1);
        if (pass == 1) bi[start[key] + pos] = make_int4(iR, __float_as_int(kp.x), __float_as_int(kp.y), kp.octave);
      }
    }
    __syncthreads();
    if (pass == 0) {
      // exclusive prefix sum over the keys: every thread sums a contiguous slice, the 256 slice totals are scanned serially
      const int per = (nk + 255) / 256;
      const int k0 = min(tid * per, nk), k1 = min(k0 + per, nk);
      int sum = 0;
      for (int k = k0; k < k1; k++) sum += cnt[k];
      part[tid] = sum;
      __syncthreads();
      if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; i++) { const int v = part[i]; part[i] = run; run += v; }
        start[nk] = run;
      }
      __syncthreads();
      int run = part[tid];
      for (int k = k0; k < k1; k++) { start[k] = run; run += cnt[k]; }
      __syncthreads();
      for (int b = tid; b <= nk; b += 256) bs[b] = start[b];
      for (int b = tid; b < nk; b += 256) cnt[b] = 0;
      __syncthreads();
    }
  }
}

__device__ __forceinline__ unsigned sad_u32(unsigned a, unsigned b, unsigned c) {  // |a - b| + c
  unsigned r;
  asm("v_sad_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// DPP rotations inside a row of 16 lanes: every lane of the row ends up with the row's minimum / sum / or
#define ORBFE_ROW_ALL(op, v) do { \
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false)); /* row_ror:8 */ \
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false)); /* row_ror:4 */ \
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false)); /* row_ror:2 */ \
    v = op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false)); /* row_ror:1 */ \
  } while (0)
__device__ __forceinline__ unsigned op_min_u(unsigned a, unsigned b) { return min(a, b); }
__device__ __forceinline__ unsigned op_add_u(unsigned a, unsigned b) { return a + b; }
__device__ __forceinline__ unsigned op_or_u(unsigned a, unsigned b) { return a | b; }
__device__ __forceinline__ unsigned row_min_u32(unsigned v) { ORBFE_ROW_ALL(op_min_u, v); return v; }
__device__ __forceinline__ unsigned row_sum_u32(unsigned v) { ORBFE_ROW_ALL(op_add_u, v); return v; }
__device__ __forceinline__ unsigned row_or_u32(unsigned v) { ORBFE_ROW_ALL(op_or_u, v); return v; }

// Per-level constants a lane needs once its keypoint's level is a per-lane value (kernel arguments cannot be indexed by a VGPR)
struct SmLevel {
  const uint8_t* baseL; const uint8_t* baseR;
  unsigned long long strideL, strideR;
  int pitchL, pitchR, wL, hL, wR, hR;
  float scale, inv_scale;
  int tiledL, tiledR;   // the level lies in 16 x 8 tiles (orbfe_internal.h: written by the fused level kernel), not row-major
};
#define SM_G 16                      // lanes per left keypoint
#define SM_KPB (256 / SM_G)          // left keypoints per workgroup
#define SM_ROUNDS 2                  // bucket entries requested up front per keypoint: SM_ROUNDS * SM_G
#define SM_WIN_PIXELS (11 * 11)      // the SAD window (w = 5)
#define SM_SAD_T ((SM_WIN_PIXELS + SM_G - 1) / SM_G)   // rounds of 16 window pixels
static_assert(SM_SAD_T == 8, "ceil(121 / 16): the last round holds window pixels 112 .. 120 only");
#define SAD_LP 32   // LDS pitch of the staged left window: 11 pixels at byte offset <= 15 of two aligned 16-byte pieces
#define SAD_RP 48   // LDS pitch of the staged right window: 21 pixels at byte offset <= 15 of three aligned 16-byte pieces
#define SAD_WIN (11 * SAD_LP + 11 * SAD_RP + 16)   // a multiple of 16: every keypoint's slice starts 16-byte aligned
// Sixteen lanes per left keypoint, four keypoints per wave (L/src/Frame.cc:504-632).  What the whole-wave kernel paid once per
// keypoint -- the wave-uniform set-up, six 64-lane reductions, the scalar epilogue -- is paid once per FOUR here: the keypoint's
// own values live in the lanes of its DPP row, reductions are four row rotations, the first-minimum / parabola epilogue runs with
// lane k = shift k.  A keypoint that drops out (no candidate, window outside the level) only idles its row; the wave leaves when
// all four have.
__global__ __launch_bounds__(256) void stereo_match_kernel(StereoParams P) {
  int pair = blockIdx.y, bx = blockIdx.x;
  // whole pairs per XCD (workgroups go to the XCDs round-robin in linear order): XCD k works on pairs k, k + 8, ...: the two
  // pyramids a pair's SAD windows are cut from (3 MB) stay in one L2 instead of every pair passing through all eight
  {
    const unsigned gx = gridDim.x;
    const unsigned lin = blockIdx.y * gx + blockIdx.x;
    const unsigned g8 = lin / (8u * gx);
    if (8u * g8 + 8u <= gridDim.y) {
      const unsigned within = lin - g8 * 8u * gx;
      pair = (int)(8u * g8 + (within & 7u));
      bx = (int)(within >> 3);
    }
  }
  const int lane = threadIdx.x & (WAVE - 1);
  const int sub = lane & (SM_G - 1);
  const int grp = threadIdx.x / SM_G;
  const int iL = bx * SM_KPB + grp;
  __shared__ SmLevel s_lv[ORBFE_MAX_LEVELS];
  __shared__ float s_r[ORBFE_MAX_LEVELS];  // r = 2 * scale[octave] of a right keypoint (L/src/Frame.cc:496)
  __shared__ __attribute__((aligned(16))) uint8_t sad_win[SM_KPB][SAD_WIN];
  __shared__ uint16_t s_offL[128], s_offR[128];   // window pixel p = 11 * yy + xx -> byte offset inside the staged windows
  if (threadIdx.x >= 128) {
    const unsigned p = threadIdx.x - 128, yy = p / 11u, xx = p - yy * 11u;
    s_offL[p] = (uint16_t)(p < 121 ? yy * SAD_LP + xx : 0);
    s_offR[p] = (uint16_t)(p < 121 ? yy * SAD_RP + xx : 0);
  }
  if (threadIdx.x < ORBFE_MAX_LEVELS) {
    const int l = threadIdx.x;
    const bool in = l < P.n_levels;
    SmLevel v;
    v.baseL = P.pyrL.base[l] + (size_t)pair * P.pyrL.img_stride[l];
    v.baseR = P.pyrR.base[l] + (size_t)pair * P.pyrR.img_stride[l];
    v.strideL = 0; v.strideR = 0;
    v.pitchL = P.pyrL.pitch[l]; v.pitchR = P.pyrR.pitch[l];
    v.wL = in ? P.pyrL.w[l] : 0; v.hL = in ? P.pyrL.h[l] : 0;
    v.wR = in ? P.pyrR.w[l] : 0; v.hR = in ? P.pyrR.h[l] : 0;
    v.scale = P.scale[l]; v.inv_scale = P.inv_scale[l];
    v.tiledL = (int)((P.pyrL.tiled >> l) & 1u); v.tiledR = (int)((P.pyrR.tiled >> l) & 1u);
    s_lv[l] = v;
    s_r[l] = 2.0f * P.scale[l];
  }
  __syncthreads();
  const int cap = P.cap, nl = P.n_levels;
  float* out_ur = P.u_right + (size_t)pair * cap;
  float* out_depth = P.depth + (size_t)pair * cap;
  int32_t* out_sad = P.sad + (size_t)pair * cap;
  const orbfe_keypoint* kl = P.kpsL + (size_t)pair * cap;
  const uint8_t* dl = P.descL + (size_t)pair * cap * 32;
  const uint8_t* dr = P.descR + (size_t)pair * cap * 32;
  // first round trip: count, left keypoint record and left descriptor together (the slot is clamped into the array)
  const int nL = P.nL[pair];
  const int iLc = min(iL, cap - 1);
  const float uL = kl[iLc].x, vL = kl[iLc].y;
  const int octL = kl[iLc].octave;
  uint4 a0, a1;
  load_desc(dl + (size_t)iLc * 32, a0, a1);
  if (sub == 0 && iL < cap) { out_ur[iL] = -1.0f; out_depth[iL] = -1.0f; out_sad[iL] = -1; }
  const int levelL = min(max(octL, 0), nl - 1);
  const int nRows = P.pyrL.h[0];
  const int row = (int)vL;
  const float minD = 0, maxD = P.maxD;
  const float minU = uL - maxD, maxU = uL - minD;
  bool act = iL < nL && row >= 0 && row < nRows && !(maxU < 0);
  const int32_t* bs = P.bucket_start + (size_t)pair * (P.n_keys + 1);
  const int4* bent = reinterpret_cast<const int4*>(P.bucket_idx) + (size_t)pair * cap * STEREO_BUCKET_SPAN;
  // the run of this row bucket's entries with octave levelL - 1 .. levelL + 1 (L/src/Frame.cc:538-539 keeps nothing else)
  const int kb = act ? (row >> 3) * nl : 0;
  const int e0 = bs[kb + max(levelL - 1, 0)];
  const int e1 = act ? bs[kb + min(levelL + 1, nl - 1) + 1] : e0;
  unsigned best = ((unsigned)ORBFE_TH_HIGH << 16) | 0xffffu;  // bestDist starts at TH_HIGH; strict <
  float best_x = 0.f;                                         // x of this lane's best candidate
  const float rowm1 = (float)(row - 1), rowp1 = (float)(row + 1);   // exact: |row| < 2^24 where act
  // SM_ROUNDS x 16 entries of each keypoint per trip: all bucket records (index, x, y, octave) are requested together, then the
  // descriptors of the survivors of the band / disparity tests (the others read descriptor 0: one cached line), then the
  // distances -- two memory round trips for the four keypoints of the wave unless one of them has more than 64 entries
  for (int eb = e0; __ballot(eb < e1) != 0ull; eb += SM_ROUNDS * SM_G) {
    int4 rec[SM_ROUNDS];
    bool ok[SM_ROUNDS];
    float rx[SM_ROUNDS];
#pragma unroll
    for (int r = 0; r < SM_ROUNDS; r++) {
      const int e = eb + r * SM_G + sub;
      ok[r] = e < e1;
      rec[r] = bent[max(min(e, e1 - 1), 0)];
    }
    uint4 b0[SM_ROUNDS], b1[SM_ROUNDS];
#pragma unroll
    for (int r = 0; r < SM_ROUNDS; r++) {
      rx[r] = __int_as_float(rec[r].y);
      const float ry = __int_as_float(rec[r].z);
      const float rad = s_r[rec[r].w & (ORBFE_MAX_LEVELS - 1)];
      // minr = floor(ry - rad) <= row <= ceil(ry + rad) = maxr (L/src/Frame.cc:497-501) for the integer row:
      // ceil(t) >= row <=> t > row - 1, floor(t) <= row <=> t < row + 1, on the same rounded float sums
      ok[r] = ok[r] && (ry + rad > rowm1) && (ry - rad < rowp1) && (rx[r] >= minU && rx[r] <= maxU);
      load_desc(dr + (size_t)(ok[r] ? rec[r].x : 0) * 32, b0[r], b1[r]);
    }
#pragma unroll
    for (int r = 0; r < SM_ROUNDS; r++) {
      if (__ballot(ok[r]) != 0ull) {
        const unsigned key = ((unsigned)hamming256(a0, a1, b0[r], b1[r]) << 16) | (unsigned)rec[r].x;
        if (ok[r] && key < best) {   // (distance, index) minimum among distance < TH_HIGH (best starts at TH_HIGH << 16 | 0xffff)
          best = key;
          best_x = rx[r];
        }
      }
    }
  }
  // first minimum in index order; the winning lane also holds the right keypoint's x
  {
    const unsigned k = ((best >> 16) < (unsigned)ORBFE_TH_HIGH) ? best : 0xFFFFFFFFu;
    best = row_min_u32(k);
    best_x = __int_as_float((int)row_or_u32((k == best && k != 0xFFFFFFFFu) ? (unsigned)__float_as_int(best_x) : 0u));
  }
  const float uR0 = best_x;
  const int thOrbDist = (ORBFE_TH_HIGH + ORBFE_TH_LOW) / 2;
  act = act && best != 0xFFFFFFFFu && (int)(best >> 16) < thOrbDist;
  if (__ballot(act) == 0ull) return;

  // sub-pixel refinement by 11x11 SAD over 11 shifts (L/src/Frame.cc:557-631)
  const SmLevel lv = s_lv[levelL];
  const float sfac = lv.inv_scale;
  const float scaleduL = roundf(uL * sfac);
  const float scaledvL = roundf(vL * sfac);
  const float scaleduR0 = roundf(uR0 * sfac);
  const int w = 5, L = 5;
  const float iniu = scaleduR0 + L - w;
  const float endu = scaleduR0 + L + w + 1;
  act = act && !(iniu < 0 || endu >= (float)lv.wR);
  const int yW = (int)(scaledvL - w), xW = (int)(scaleduL - w), xRc = (int)scaleduR0;
  const int xR0 = xRc - L - w;
  // the reference reads these windows unchecked (cv::Mat::rowRange/colRange would throw); treat as no match
  act = act && !(yW < 0 || yW + 2 * w >= lv.hL || xW < 0 || xW + 2 * w >= lv.wL || xR0 < 0 || xRc + L + w >= lv.wR ||
                 yW + 2 * w >= lv.hR);
  if (__ballot(act) == 0ull) return;
  // stage the 11 x 11 left window and the 11 x 21 right window (all 11 shifts) of the row's keypoint in its LDS slice: lane r of
  // the row loads window row r as aligned 16-byte pieces -- two of the left level, three of the right one, from the piece that
  // holds the window's first column on -- five load instructions for the wave's four keypoints.  A piece is 16 bytes of a row
  // in a row-major level and one tile row in a tiled one (orbfe_level_offset): the same loads, another address.
  uint8_t* winL = &sad_win[grp][0];
  uint8_t* winR = winL + 11 * SAD_LP;
  const int axL = xW & ~15, axR = xR0 & ~15;
  if (act && sub < 11) {
    // (a pointer that comes out of LDS is a generic one to the compiler: say that it is global memory, or the loads are flat_load)
    typedef const __attribute__((address_space(1))) uint8_t* gptr_t;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const int y = yW + sub;
    u32x4 vl[2], vr[3];
#pragma unroll
    for (int k = 0; k < 2; k++) {   // a piece beyond the row's last one is not part of the window: the last one again
      const int x = min(axL + 16 * k, lv.pitchL - 16);
      vl[k] = *reinterpret_cast<const __attribute__((address_space(1))) u32x4*>((gptr_t)(uintptr_t)lv.baseL + orbfe_level_offset(x, y, lv.pitchL, lv.tiledL != 0));
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int x = min(axR + 16 * k, lv.pitchR - 16);
      vr[k] = *reinterpret_cast<const __attribute__((address_space(1))) u32x4*>((gptr_t)(uintptr_t)lv.baseR + orbfe_level_offset(x, y, lv.pitchR, lv.tiledR != 0));
    }
    u32x4* wl = reinterpret_cast<u32x4*>(winL + sub * SAD_LP);
    wl[0] = vl[0]; wl[1] = vl[1];
    u32x4* wr = reinterpret_cast<u32x4*>(winR + sub * SAD_RP);
    wr[0] = vr[0]; wr[1] = vr[1]; wr[2] = vr[2];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint8_t* WL = winL + (xW - axL);
  const uint8_t* WR = winR + (xR0 - axR);
  // |a - b| with a = IL - cL, b = IR - cR[k]: both biased by +255 so that v_sad_u32 (|x - y| + acc) applies
  const int cLm = (int)WL[w * SAD_LP + w] - 255;
  int cRm[11];
#pragma unroll
  for (int k = 0; k < 11; k++) cRm[k] = (int)WR[w * SAD_RP + w + k] - 255;
  unsigned acc[11];
#pragma unroll
  for (int k = 0; k < 11; k++) acc[k] = 0;
#pragma unroll
  for (int t = 0; t < SM_SAD_T; t++) {
    const int p = sub + SM_G * t;
    if (t < SM_SAD_T - 1 || p < SM_WIN_PIXELS) {
      const unsigned a = (unsigned)((int)WL[s_offL[p]] - cLm);
      const uint8_t* rrow = WR + s_offR[p];
#pragma unroll
      for (int k = 0; k < 11; k++) acc[k] = sad_u32(a, (unsigned)((int)rrow[k] - cRm[k]), acc[k]);
    }
  }
  // every sum is <= 121 * 510 < 65536: reduce two per register inside the row; every lane of the row gets the totals
  unsigned pk[6];
#pragma unroll
  for (int j = 0; j < 5; j++) pk[j] = acc[2 * j] | (acc[2 * j + 1] << 16);
  pk[5] = acc[10];
#pragma unroll
  for (int j = 0; j < 6; j++) pk[j] = row_sum_u32(pk[j]);
  // lane k of the row takes the sum of shift k (k < 11).  The reference's `dist < bestDist` walk over float distances
  // (L/src/Frame.cc:593-600; the sums are integers < 2^16, exact as floats) is an integer first-minimum: the minimum of
  // (sum, k) keys over the row.
  unsigned mine = pk[0];
  {
    const int t = sub >> 1;
    mine = t == 1 ? pk[1] : mine; mine = t == 2 ? pk[2] : mine; mine = t == 3 ? pk[3] : mine;
    mine = t == 4 ? pk[4] : mine; mine = t == 5 ? pk[5] : mine;
    mine = (sub & 1) ? (mine >> 16) : (mine & 0xffffu);
  }
  const unsigned kmin = row_min_u32(sub < 11 ? ((mine << 4) | (unsigned)sub) : 0xFFFFFFFFu);
  const int bk = (int)(kmin & 15u);
  const int sadBest = (int)(kmin >> 4);
  const int bestincR = bk - L;
  // the neighbours of the minimum, from the lanes that hold them (for bk = 0 / 10 the lane read is outside 0..10: no match anyway)
  const int rowbase = lane & ~(SM_G - 1);
  const int i1 = __builtin_amdgcn_ds_bpermute((rowbase + ((bk + 15) & 15)) << 2, (int)mine);
  const int i3 = __builtin_amdgcn_ds_bpermute((rowbase + ((bk + 1) & 15)) << 2, (int)mine);
  const int i2 = sadBest;
  if (!act || sub != 0 || bestincR == -L || bestincR == L) return;
  const float dist1 = (float)i1, dist2 = (float)i2, dist3 = (float)i3;
  const float deltaR = (dist1 - dist3) / (2.0f * (dist1 + dist3 - 2.0f * dist2));
  if (deltaR < -1 || deltaR > 1) return;
  float bestuR = lv.scale * ((float)scaleduR0 + (float)bestincR + deltaR);
  float disparity = (uL - bestuR);
  if (disparity >= minD && disparity < maxD) {
    if (disparity <= 0) {
      disparity = (float)0.01;
      bestuR = (float)((double)uL - 0.01);
    }
    out_depth[iL] = P.mbf / disparity;
    out_ur[iL] = bestuR;
    out_sad[iL] = sadBest;
  }
}

// One block per stereo pair: the reference sorts (SAD, iL) pairs, takes the element at size/2 as the
// median and drops every match with SAD >= 1.5*1.4*median (L/src/Frame.cc:634-645).  The order statistic
// is found by a two-level 256-bin radix select (SAD <= 121*510 < 65536).
__global__ __launch_bounds__(256) void stereo_median_kernel(StereoParams P) {
  __shared__ int hist[256];
  __shared__ int sh[4];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const int nL = P.nL[pair];
  float* out_ur = P.u_right + (size_t)pair * P.cap;
  float* out_depth = P.depth + (size_t)pair * P.cap;
  const int32_t* sad = P.sad + (size_t)pair * P.cap;
  hist[tid] = 0;
  if (tid == 0) sh[0] = 0;
  __syncthreads();
  int cntv = 0;
  for (int i = tid; i < nL; i += 256) {
    const int s = sad[i];
    if (s >= 0) { atomicAdd(&hist[(s >> 8) & 0xff], 1); cntv++; }
  }
  atomicAdd(&sh[0], cntv);
  __syncthreads();
  const int total = sh[0];
  if (total == 0) { if (tid == 0) P.n_matched[pair] = 0; return; }
  const int k = total / 2;  // 0-based rank
  if (tid == 0) {
    int run = 0, hb = 0;
    for (; hb < 256; hb++) { if (run + hist[hb] > k) break; run += hist[hb]; }
    sh[1] = hb;
    sh[2] = k - run;
  }
  __syncthreads();
  const int hb = sh[1], k2 = sh[2];
  __syncthreads();
  hist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < nL; i += 256) {
    const int s = sad[i];
    if (s >= 0 && ((s >> 8) & 0xff) == hb) atomicAdd(&hist[s & 0xff], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0, lb = 0;
    for (; lb < 256; lb++) { if (run + hist[lb] > k2) break; run += hist[lb]; }
    sh[3] = (hb << 8) | lb;
    sh[0] = 0;
  }
  __syncthreads();
  const float median = (float)sh[3];
  const float thDist = 1.5f * 1.4f * median;
  int kept = 0;
  for (int i = tid; i < nL; i += 256) {
    const int s = sad[i];
    if (s >= 0) {
      if ((float)s < thDist) kept++;
      else { out_ur[i] = -1; out_depth[i] = -1; }
    }
  }
  atomicAdd(&sh[0], kept);
  __syncthreads();
  if (tid == 0) P.n_matched[pair] = sh[0];
}

// ------------------------------------------------------------------------------------------------ launcher
void orbfe_launch_stereo(const StereoParams& p, int n_pairs, hipStream_t s) {
  const size_t bucket_lds = sizeof(int) * (size_t)(2 * p.n_keys + 1);
  if (bucket_lds > 48 * 1024) {   // tall images with many levels only (KITTI: 3 KB)
    static std::atomic<unsigned long long> raised{0};
    raise_dynamic_lds(reinterpret_cast<const void*>(stereo_bucket_kernel), (int)(sizeof(int) * (2 * STEREO_MAX_KEYS + 1)), raised);
  }
  hipLaunchKernelGGL(stereo_bucket_kernel, dim3(n_pairs), dim3(256), bucket_lds, s, p);
  dim3 grid((p.cap + SM_KPB - 1) / SM_KPB, n_pairs);
  hipLaunchKernelGGL(stereo_match_kernel, grid, dim3(256), 0, s, p);
  hipLaunchKernelGGL(stereo_median_kernel, dim3(n_pairs), dim3(256), 0, s, p);
}
