// pyramid_kernels.hip -- the image pyramid of the ORB extractor for gfx950 (MI355X, wave64): level 0, the level chain, the blur.
//
// Kernel            replaces (reference file:line, L/ = Source/Libraries/ORB_SLAM2/)
// copy_level0       copyMakeBorder of the input into mvImagePyramid[0]  L/src/ORBextractor.cc:1061
// pyr_resize        cv::resize(INTER_LINEAR) chained level to level      L/src/ORBextractor.cc:1054
// gauss_blur7       GaussianBlur(7x7, sigma 2, REFLECT_101)              L/src/ORBextractor.cc:1017-1019
//
// All arithmetic that decides an output bit is integer.
#include "orbfe_internal.h"

__device__ __forceinline__ int reflect101(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = (p < 0) ? -p : 2 * (len - 1) - p;
  return p;
}

// ------------------------------------------------------------------------------------------------ level 0
// Copies the caller's images (arbitrary stride/alignment) into the pitched, 256-byte aligned level-0 planes.
// 16 destination bytes per thread: five aligned source dwords + v_alignbyte instead of 16 byte loads (the source rows
// start at arbitrary alignment); the last chunk of a row takes the byte path and replicates the last pixel into the
// pitch padding.
__global__ __launch_bounds__(256) void copy_level0_kernel(const uint8_t* __restrict__ src, int sstride,
                                                           unsigned long long simg, uint8_t* __restrict__ dst,
                                                           int dpitch, unsigned long long dimg, int w, int h, int tiled) {
  const int nchunk = (w + 15) >> 4;  // 16-byte chunks per row; (row, chunk) pairs are dealt to threads in raster order
  const int item = blockIdx.x * 256 + threadIdx.x;
  const int y = (int)((item + 0.5f) * (1.0f / (float)nchunk));  // exact for item < 2^22
  const int x16 = (item - y * nchunk) * 16;
  if (y >= h) return;
  const uint8_t* S = src + (size_t)blockIdx.z * simg + (size_t)y * sstride;
  uint32_t out[4];
  if (x16 + 20 <= w) {
    const uintptr_t A = reinterpret_cast<uintptr_t>(S + x16);
    const uint32_t sh = (uint32_t)(A & 3);
    const uint32_t* B = reinterpret_cast<const uint32_t*>(A - sh);
    uint32_t d[5];
#pragma unroll
    for (int i = 0; i < 5; i++) d[i] = B[i];
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      out[i] = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int x = x16 + 4 * i + j < w ? x16 + 4 * i + j : w - 1;
        out[i] |= (uint32_t)S[x] << (8 * j);
      }
    }
  }
  if (tiled) {   // the copy is written in 16 x 8 tiles like the levels behind it (orbfe_internal.h): a chunk is one tile row
    uint8_t* D = dst + (size_t)blockIdx.z * dimg + orbfe_tiled_offset(x16, y, dpitch);   // dpitch is a multiple of 64: the chunk is whole
    *reinterpret_cast<uint4*>(D) = make_uint4(out[0], out[1], out[2], out[3]);
    return;
  }
  uint8_t* D = dst + (size_t)blockIdx.z * dimg + (size_t)y * dpitch + x16;
  if (x16 + 16 <= dpitch) *reinterpret_cast<uint4*>(D) = make_uint4(out[0], out[1], out[2], out[3]);
  else
    for (int i = 0; i < 4 && x16 + 4 * i < dpitch; i++) reinterpret_cast<uint32_t*>(D)[i] = out[i];
}

// ------------------------------------------------------------------------------------------------ resize
// cv::resize INTER_LINEAR 8UC1, fixed point: horizontal taps sum 2048 (int32 row), vertical
// ((b*(T>>4))>>16 summed, +2, >>2).  4 destination pixels per thread, one dword store.
__global__ __launch_bounds__(256) void pyr_resize_kernel(const uint8_t* __restrict__ src, int spitch,
                                                          unsigned long long simg, uint8_t* __restrict__ dst,
                                                          int dpitch, unsigned long long dimg, int dw, int dh,
                                                          const ResizeTap* __restrict__ xt,
                                                          const ResizeTap* __restrict__ yt) {
  const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int y = blockIdx.y * 4 + threadIdx.y;
  if (x4 >= dw || y >= dh) return;
  const uint8_t* S = src + (size_t)blockIdx.z * simg;
  const ResizeTap ty = yt[y];
  const uint8_t* S0 = S + (size_t)ty.s0 * spitch;
  const uint8_t* S1 = S + (size_t)ty.s1 * spitch;
  const int b0 = ty.c0, b1 = ty.c1;
  uint32_t out = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int dx = x4 + i < dw ? x4 + i : dw - 1;
    const ResizeTap tx = xt[dx];
    const int t0 = S0[tx.s0] * tx.c0 + S0[tx.s1] * tx.c1;
    const int t1 = S1[tx.s0] * tx.c0 + S1[tx.s1] * tx.c1;
    const int v = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2;
    out |= (uint32_t)(v & 0xff) << (8 * i);
  }
  *reinterpret_cast<uint32_t*>(dst + (size_t)blockIdx.z * dimg + (size_t)y * dpitch + x4) = out;
}

#define RS_COLS 560   // bytes of a staged source row: 256 destination pixels x scale <= 2, plus alignment slack
// LDS-staged resize: a workgroup produces a 256 x 16 destination tile; the source window it needs (at most RS2_ROWS rows x
// RS_COLS bytes for scale factors up to 2) is fetched with aligned 16-byte loads (one division per thread, all loads in
// flight before the first LDS store), the per-pixel taps then gather single bytes from LDS.  4 x 4 destination pixels per
// thread: the horizontal taps and all address arithmetic are loaded once and reused for four rows.  Same arithmetic and
// tables as pyr_resize_kernel (the direct-gather fallback for larger scale factors).
#define RS2_ROWS 34
__global__ __launch_bounds__(256) void pyr_resize_lds16_kernel(const uint8_t* __restrict__ src, int spitch,
                                                                unsigned long long simg, uint8_t* __restrict__ dst,
                                                                int dpitch, unsigned long long dimg, int dw, int dh,
                                                                const ResizeTap* __restrict__ xt,
                                                                const ResizeTap* __restrict__ yt) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[RS2_ROWS * RS_COLS];
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const int x0 = blockIdx.x * 256, y0 = blockIdx.y * 16;
  const int xl = min(x0 + 255, dw - 1), yl = min(y0 + 15, dh - 1);
  const int sxa = xt[x0].s0 & ~15;
  const int ncols16 = ((xt[xl].s1 - sxa) >> 4) + 1;  // <= 35
  const int sy_first = yt[y0].s0;
  const int nrows = yt[yl].s1 - sy_first + 1;        // <= 34
  const uint8_t* S = src + (size_t)blockIdx.z * simg;
  {
    const int rpp = 256 / ncols16;  // rows per pass, >= 7
    const int r0 = (int)((tid + 0.5f) * (1.0f / (float)ncols16));
    const int c = tid - r0 * ncols16;
    if (r0 < rpp) {
      const uint8_t* g = S + (size_t)sy_first * spitch + sxa + 16 * c;
      uint4 v[5];
#pragma unroll
      for (int k = 0; k < 5; k++) {
        const int r = r0 + k * rpp;
        v[k] = r < nrows ? *reinterpret_cast<const uint4*>(g + (size_t)r * spitch) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < 5; k++) {
        const int r = r0 + k * rpp;
        if (r < nrows) *reinterpret_cast<uint4*>(tile + r * RS_COLS + 16 * c) = v[k];
      }
    }
  }
  __syncthreads();
  const int x4 = x0 + threadIdx.x * 4;
  if (x4 >= dw) return;
  ResizeTap tx[4];
#pragma unroll
  for (int i = 0; i < 4; i++) tx[i] = xt[min(x4 + i, dw - 1)];
  uint8_t* D = dst + (size_t)blockIdx.z * dimg + x4;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int y = y0 + threadIdx.y * 4 + k;
    if (y >= dh) break;
    const ResizeTap ty = yt[y];
    const uint8_t* S0 = tile + (ty.s0 - sy_first) * RS_COLS - sxa;
    const uint8_t* S1 = tile + (ty.s1 - sy_first) * RS_COLS - sxa;
    const int b0 = ty.c0, b1 = ty.c1;
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int t0 = S0[tx[i].s0] * tx[i].c0 + S0[tx[i].s1] * tx[i].c1;
      const int t1 = S1[tx[i].s0] * tx[i].c0 + S1[tx[i].s1] * tx[i].c1;
      const int v = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2;
      out |= (uint32_t)(v & 0xff) << (8 * i);
    }
    *reinterpret_cast<uint32_t*>(D + (size_t)y * dpitch) = out;
  }
}

// bits 32..47 of the product of two 24-bit operands
__device__ __forceinline__ uint32_t mulhi_u24(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t mulhi_u24_s(uint32_t a_uniform, uint32_t b) {   // first operand from a scalar register
  uint32_t r;
  asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(r) : "s"(a_uniform), "v"(b));
  return r;
}

// Same tile, staging and arithmetic as pyr_resize_lds16_kernel, restated twice over:
// (1) per-pixel work for the vector ALU:
//   * a thread's four destination pixels read source columns s0 .. s0+7 of a row (scale factors <= 2): three aligned LDS
//     dwords, two v_alignbyte to start the window at s0, and per pixel one v_perm (bytes s0_i, s0_i+1 into 16-bit fields)
//     + one v_dot2_u32_u16 against (c0, c1) -- instead of two single-byte LDS gathers and two multiplies per row;
//   * the horizontal result of a source row is computed once and reused by the next destination row when that row's upper
//     tap is this row's lower one (a wave = one destination row, so the test is wave-uniform);
//   * (b * (t >> 4)) >> 16 == mul_hi_u24(b << 12, t & ~15): one full-rate instruction per tap.
//   At the right border the table gives s1 = s0 with c1 = 0 (build_taps): byte s0+1 is then whatever follows in LDS, times 0.
// (2) persistent workgroups: with one 4 KB tile per workgroup the seven launches of a pyramid ran at the rate workgroups can
//   be dispatched (~630 per microsecond, measured with the body removed), not at the memory rate.  Here a workgroup walks
//   tiles L, L + gridDim.x, ... and the source window of the NEXT tile is already in flight (held in registers) while the
//   current one is interpolated out of LDS.
struct ResizeGeom {
  int x0, y0, bz, sxa, ncols16, sy_first, nrows;
};
template <int TROWS, int SROWS, int COLS>   // COLS: bytes of a staged source row (RS_COLS for scale factors up to 2; 336 when every window fits 21 chunks)
__global__ __launch_bounds__(256) void pyr_resize_dot_kernel(const uint8_t* __restrict__ src, int spitch,
                                                              unsigned long long simg, uint8_t* __restrict__ dst,
                                                              int dpitch, unsigned long long dimg, int dw, int dh,
                                                              const ResizeTap* __restrict__ xt,
                                                              const ResizeTap* __restrict__ yt, int tiles_x, int tiles_y,
                                                              int n_tiles) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[SROWS * COLS + 16];
  constexpr int NLD = (SROWS + 256 / (COLS / 16) - 1) / (256 / (COLS / 16));   // staging passes: at least 256 / (COLS / 16) rows per pass
  const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int tid = wv * 64 + lane;
  auto geom = [&](int t) {
    ResizeGeom g;
    const int bx = t % tiles_x, r = t / tiles_x;
    const int by = r % tiles_y;
    g.bz = r / tiles_y;
    g.x0 = bx * 256;
    g.y0 = by * TROWS;
    const int xl = min(g.x0 + 255, dw - 1), yl = min(g.y0 + TROWS - 1, dh - 1);
    g.sxa = xt[g.x0].s0 & ~15;
    g.ncols16 = ((xt[xl].s1 - g.sxa) >> 4) + 1;   // <= 35
    g.sy_first = yt[g.y0].s0;
    g.nrows = yt[yl].s1 - g.sy_first + 1;         // <= SROWS
    return g;
  };
  // thread -> (row r0 + k * rpp, 16-byte column c) of the window: one division per tile, all loads issued back to back
  auto fetch = [&](const ResizeGeom& g, uint4 (&v)[NLD], int& r0, int& c, int& rpp) {
    rpp = 256 / g.ncols16;
    r0 = (int)((tid + 0.5f) * (1.0f / (float)g.ncols16));
    c = tid - r0 * g.ncols16;
    if (r0 < rpp) {
      const uint8_t* p = src + (size_t)g.bz * simg + (size_t)g.sy_first * spitch + g.sxa + 16 * c;
#pragma unroll
      for (int k = 0; k < NLD; k++) {
        const int r = r0 + k * rpp;
        v[k] = r < g.nrows ? *reinterpret_cast<const uint4*>(p + (size_t)r * spitch) : make_uint4(0, 0, 0, 0);
      }
    }
  };
  typedef __attribute__((ext_vector_type(2))) unsigned short us2;

  int t = (int)blockIdx.x;
  if (t >= n_tiles) return;
  ResizeGeom g = geom(t);
  uint4 v[NLD];
  int r0, c, rpp;
  fetch(g, v, r0, c, rpp);
  for (;;) {
    // horizontal taps of this tile (L2 hits; overlap the wait for the window)
    const int x4 = g.x0 + lane * 4;
    uint2 txr[4];
#pragma unroll
    for (int i = 0; i < 4; i++) txr[i] = reinterpret_cast<const uint2*>(xt)[min(x4 + i, dw - 1)];
    // and its vertical taps: loads return in order, so everything the interpolation needs is requested BEFORE the next
    // tile's window -- a load issued after the prefetch would have to wait for it
    uint2 tyr[TROWS / 4];
#pragma unroll
    for (int k = 0; k < TROWS / 4; k++) tyr[k] = reinterpret_cast<const uint2*>(yt)[min(g.y0 + wv * (TROWS / 4) + k, dh - 1)];
    if (r0 < rpp) {
#pragma unroll
      for (int k = 0; k < NLD; k++) {
        const int r = r0 + k * rpp;
        if (r < g.nrows) *reinterpret_cast<uint4*>(tile + r * COLS + 16 * c) = v[k];
      }
    }
    __syncthreads();
    const ResizeGeom cur = g;
    const int tn = t + (int)gridDim.x;
    if (tn < n_tiles) {
      g = geom(tn);
      fetch(g, v, r0, c, rpp);
    }
    if (x4 < dw) {
      const int s00 = (int)(int16_t)(txr[0].x & 0xffff);
      const int base = s00 - cur.sxa;
      const uint32_t sh = (uint32_t)base & 3u;
      uint32_t sel[4], cp[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t o = (uint32_t)((int)(int16_t)(txr[i].x & 0xffff) - s00);   // 0 .. 6
        sel[i] = o | 0x0c000c00u | ((o + 1) << 16);
        cp[i] = txr[i].y;                                                         // c0 | c1 << 16
      }
      const uint32_t* trow = reinterpret_cast<const uint32_t*>(tile + (base & ~3));
      auto hrow = [&](int r, uint32_t (&hh)[4]) {
        const uint32_t* p = trow + r * (COLS / 4);
        const uint32_t* p2 = p + 2;
        asm("" : "+v"(p2));   // keep the third dword a separate ds_read_b32 (a 4-byte aligned ds_read_b96 is slow)
        const uint32_t w0 = p[0], w1 = p[1], w2 = *p2;
        const uint32_t W0 = __builtin_amdgcn_alignbyte(w1, w0, sh), W1 = __builtin_amdgcn_alignbyte(w2, w1, sh);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const uint32_t u = __builtin_amdgcn_perm(W1, W0, sel[i]);
          hh[i] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, u), __builtin_bit_cast(us2, cp[i]), 0u, false) & ~15u;
        }
      };
      uint8_t* D = dst + (size_t)cur.bz * dimg + x4;
      uint32_t hp[4] = {0, 0, 0, 0};
      int prev = -1;
#pragma unroll
      for (int k = 0; k < TROWS / 4; k++) {
        const int y = cur.y0 + wv * (TROWS / 4) + k;
        if (y >= dh) break;
        const uint32_t tys = (uint32_t)__builtin_amdgcn_readfirstlane((int)tyr[k].x);
        const uint32_t tyc = (uint32_t)__builtin_amdgcn_readfirstlane((int)tyr[k].y);
        const int ra = (int)(int16_t)(tys & 0xffff) - cur.sy_first, rb = (int)(int16_t)(tys >> 16) - cur.sy_first;
        uint32_t h0[4], h1[4];
        if (ra == prev) {
#pragma unroll
          for (int i = 0; i < 4; i++) h0[i] = hp[i];
        } else {
          hrow(ra, h0);
        }
        if (rb == ra) {
#pragma unroll
          for (int i = 0; i < 4; i++) h1[i] = h0[i];
        } else {
          hrow(rb, h1);
        }
        const uint32_t B0 = (tyc & 0xffffu) << 12, B1 = (tyc >> 16) << 12;
        uint32_t sm[4];
#pragma unroll
        for (int i = 0; i < 4; i++) sm[i] = mulhi_u24(B0, h0[i]) + mulhi_u24(B1, h1[i]) + 2u;
        const uint32_t P01 = (sm[0] | (sm[1] << 16)) >> 2, P23 = (sm[2] | (sm[3] << 16)) >> 2;   // values <= 255 in bytes 0 and 2
        *reinterpret_cast<uint32_t*>(D + (size_t)y * dpitch) = __builtin_amdgcn_perm(P23, P01, 0x06040200u);
#pragma unroll
        for (int i = 0; i < 4; i++) hp[i] = h1[i];
        prev = rb;
      }
    }
    if (tn >= n_tiles) break;
    t = tn;
    __syncthreads();   // every wave is done reading this tile before the next window is written over it
  }
}

// ------------------------------------------------------------------------------------------------ blur
// The blurred planes are read by nobody but the descriptor gather, which fetches a 37-row x 64-byte window per keypoint: one
// memory request per window row in a row-major plane (~55 per keypoint).  They are therefore stored TILED: 16 pixels x 8 rows
// = one 128-byte line, tiles in raster order (pitch / 16 tiles per tile row).  A window then touches ~4 x 6 tiles.
// Byte offset of pixel (x, y); x, y >= 0:
__device__ __forceinline__ uint32_t blur_tiled_offset(int x, int y, int pitch) { return orbfe_tiled_offset(x, y, pitch); }   // orbfe_internal.h
// 7x7 sigma-2 Gaussian, OpenCV's 8.8 fixed-point taps [18,34,48,56,48,34,18], exact 16.16 accumulation,
// round half up.  One 64 x BT_H (56) output tile per workgroup.  Interior tiles of a row-major level stage the
// (64+8) x (56+6) input window with aligned dword loads; tiles touching a level edge take the byte path with
// REFLECT_101 indexing; a tiled level arrives as whole tile rows.
// ---- the tile kernel's blur runs on the matrix cores: the arithmetic of gauss_blur7_mfma_kernel below -- a 7-tap
// pass is Out = In x Band, pixels as i8 (x ^ 0x80), exact in v_mfma_i32_16x16x64_i8 -- fed from the tile's staged window instead of
// a strip walk.  Wave w of the four owns output columns 16w .. 16w + 15 of the 64 x 56 tile and all of its rows:
//   horizontal: per 16-row block of the window ONE product: A = lane (q, r): window row 16 blk + r, bytes 16w + 16q .. + 15 (one
//     aligned ds_read_b128: the operand layout IS the staged rows), B = the band matrix (output column 4 + 16w + n of the window
//     <- input columns 16w + k: the same matrix for every column group), C = 128.  D: lane (q, c) holds H - 32768 + 128 of rows
//     4q .. 4q + 3 at column c, packed (blur_pack) into the i8 digits (a, b) of H - 32768 = 256 a + b;
//   vertical: those dwords of the four blocks ARE the second product's A operand of the same lane (K order: byte 4 ww + i <->
//     window row 16 ww + 4q + i; the band matrices T_b are written in that order), B = T_b for output rows 16b .. 16b + 15:
//     V = 256 (T a) + (T b) + 256 * 32768, pixel = byte 2 of V + 32768; lane (q, n) holds columns 4q .. 4q + 3 of output row
//     16b + n: one dword of the 16 x 8-tiled plane.
// REFLECT_101 needs no matrix of its own here: the staging has put the reflected pixels into the window.  Against the two
// passes on the vector ALUs (v_dot4 / v_dot2 through a second LDS buffer, rounds 1-4): no second LDS buffer, no second barrier, 154
// instead of 243 vector instructions per wave.  Rows 62, 63 of the last block meet zero coefficients only.
typedef int v4i __attribute__((ext_vector_type(4)));
__device__ __attribute__((aligned(16))) int8_t g_blur_tile_tab[5 * 1024];   // [0]: the horizontal band matrix; [1..4]: T_b (1 KB each: 64 lanes x 16 bytes)
__device__ __forceinline__ void blur_pack(const v4i d, int& hi, int& lo) {
  const uint32_t t01 = __builtin_amdgcn_perm((uint32_t)d.y, (uint32_t)d.x, 0x05010400u);   // [d0.b0, d1.b0, d0.b1, d1.b1]
  const uint32_t t23 = __builtin_amdgcn_perm((uint32_t)d.w, (uint32_t)d.z, 0x05010400u);
  lo = (int)(__builtin_amdgcn_perm(t23, t01, 0x05040100u) ^ 0x80808080u);
  hi = (int)__builtin_amdgcn_perm(t23, t01, 0x07060302u);
}
#define BT_W 64
#define BT_H ORBFE_BLUR_TILE_H   // 56: 7 blocks of 8 output rows = 7 storage tiles (58 measured 2-3 % slower: 56 rows end on storage-tile boundaries)
#define BT_INP 96   // LDS pitch (bytes) of the input window: six 16-byte pieces, column j <-> level x = ox - 16 + j (a tiled level arrives
#define BT_COL0 12  // as whole tile rows); BT_COL0: the column of x = ox - 4, where the window the two passes need begins
// RESIZE: the tile also produces its part of level + 1 (cv::resize INTER_LINEAR, the arithmetic of pyr_resize_dot_kernel) from
// the window it has staged for the blur: the pyramid chain and the blur then read every level ONCE, and the seven resize
// launches of a pyramid disappear (launch l = blur of level l + resize l -> l + 1; the last level's launch only blurs).  A
// destination dword (four pixels) belongs to the tile that holds the first source column of its first pixel, a destination row
// to the tile that holds its upper source row (BlurTile::j0 .. r1, from the plan): every tap of an owned dword-row then lies
// inside the window -- staged one dword wider (19 instead of 18) than the blur alone needs --, nothing is computed twice and no
// halo is added.  Thread = (dword column, every (BT_THREADS / 16)-th destination row); its horizontal taps are requested before the
// window's pixels, so they have arrived when the barrier behind the staging opens; the rows' vertical taps go through LDS.
#ifndef BT_MIN_WAVES
#define BT_MIN_WAVES 2   // with one argument hipcc puts the MFMA results into AGPRs and copies every one back (lesson 31)
#endif
#ifndef BT_THREADS
#define BT_THREADS 128   // threads per tile: with the matrix-core blur a tile needs 5 KB of LDS and 56 registers, so sixteen two-wave tiles
#endif                   // are resident per CU (256 threads: eight; 64: the fused resize needs 69 registers): 0.506 / 0.474 / 0.492 ms per level chain
template <bool RESIZE, int THREADS>   // THREADS per tile: THREADS for batches (tiles in flight), 256 for a handful of images (latency of a tile)
__global__ __launch_bounds__(THREADS, BT_MIN_WAVES) void blur_level_kernel(PyrView src, PyrView dst, const BlurTile* __restrict__ tiles, int n_tiles,
                                                         LevelResize rz) {
  __shared__ __attribute__((aligned(16))) uint8_t in[65 * BT_INP];   // 62 staged rows; the last 16-row block reads two more, the last column
                                                                     // group 32 bytes past its row (zero coefficients)
  const int tid = threadIdx.x;
  // this wave's band matrix and the four vertical ones: 5 x 16 bytes per lane, requested before anything else
  const int mlane = tid & 63, mwave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const v4i* mtab = reinterpret_cast<const v4i*>(g_blur_tile_tab);
  const v4i HB = mtab[mlane];
  // whole images per XCD (workgroups go to the XCDs round-robin in linear order): XCD k walks images k, k + 8, ... tile by tile in
  // raster order, so the halo rows and the 128-byte lines neighbouring tiles share are fetched into ONE L2 once (against runs of
  // eight raster-consecutive tiles per XCD: 88.1 k -> 90.2 k frames/s, level chain 0.466 -> 0.441 ms)
  int tile_id = (int)blockIdx.x, img = (int)blockIdx.y;
  {
    const unsigned gx = gridDim.x;
    const unsigned lin = blockIdx.y * gx + blockIdx.x;
    const unsigned grp = lin / (8u * gx);
    if (8u * grp + 8u <= gridDim.y) {
      const unsigned within = lin - grp * 8u * gx;
      img = (int)(8u * grp + (within & 7u));
      tile_id = (int)(within >> 3);
    }
  }
  // the tile's record through the scalar cache (four dwords at a wave-uniform address): the compiler's own choice is a vector
  // dwordx3 + ushort load -- an L2 round trip in front of the window's first load address, on the critical path of every tile
  static_assert(sizeof(BlurTile) == 16, "four dwords");
  BlurTile t;
  {
    const __attribute__((address_space(4))) uint32_t* q =
        (const __attribute__((address_space(4))) uint32_t*)(uintptr_t)(tiles + __builtin_amdgcn_readfirstlane(tile_id));
    uint32_t w4[4];
#pragma unroll
    for (int j = 0; j < 4; j++) w4[j] = q[j];
    __builtin_memcpy(&t, w4, sizeof(t));
  }
  const int lvl = t.level;
  const int w = src.w[lvl], h = src.h[lvl], pitch = src.pitch[lvl];
  const uint8_t* S = src.base[lvl] + (size_t)img * src.img_stride[lvl];
  uint8_t* D = const_cast<uint8_t*>(dst.base[lvl]) + (size_t)img * dst.img_stride[lvl];
  const int ox = t.tx * BT_W, oy = t.ty * BT_H;
  const bool stiled = (src.tiled >> lvl) & 1u;   // the level this launch reads lies in 16 x 8 tiles (written by the launch before it)
  // the resize taps: this thread's dword column J (pixels 4J .. 4J + 3) in registers; the vertical taps of the tile's (at most 48)
  // destination rows go through LDS -- a thread's rows are THREADS / 16 apart, held in registers they cost a wave of occupancy
  const int J = t.j0 + (tid & (ORBFE_FUSE_DWORDS - 1));
  __shared__ uint4 ytap[16 * ORBFE_FUSE_ROWS];   // per destination row: byte offsets of its two source rows in the window, the two weights << 12
  __shared__ uint32_t ydst[16 * ORBFE_FUSE_ROWS];   // ... and the byte offset of the row (of its tile row and row inside it) in level + 1
  uint2 txr[4], tyl = make_uint2(0u, 0u);
  if constexpr (RESIZE) {
#pragma unroll
    for (int i = 0; i < 4; i++) txr[i] = reinterpret_cast<const uint2*>(rz.xt)[min(4 * J + i, rz.dw - 1)];
    tyl = reinterpret_cast<const uint2*>(rz.yt)[min(t.r0 + min(tid, 16 * ORBFE_FUSE_ROWS - 1), rz.dh - 1)];
  }
  {
    // (BT_H+6) rows x NC dwords (x = ox-4 .. ox+67, or .. ox+71 with the resize).  Thread -> dword column c = tid % NC and rows
    // r0 + RPP k (one division; 252 / 247 of 256 threads), all loads issued before the first LDS store.  Interior tiles (the
    // common case, wave-uniform) load plain aligned dwords; on edge tiles a dword that straddles the image border (left edge, the
    // partial dword at the right edge, columns beyond it) is assembled from bytes with REFLECT_101 indexing, and rows reflect as a
    // whole.
    uint32_t* in32 = reinterpret_cast<uint32_t*>(in);
    constexpr int NC = RESIZE ? 19 : 18;
    constexpr int RPP = THREADS / NC, NLD = (BT_H + 6 + RPP - 1) / RPP;
    const int r0 = tid / NC, c = tid - r0 * NC;
    const int x = ox - 4 + 4 * c;
    uint32_t v[NLD];
    const bool interior = oy >= 3 && oy + BT_H + 3 <= h && ox >= 4 && ox - 4 + 4 * NC <= w;
    const bool tilepath = stiled;   // a tiled level arrives as whole tile rows (below), also at the level's edges
    // (round 6: interior windows staged by LDS-DMA -- piece i = 6 * row + column IS byte 16 i of the window for row-major and, with tile
    //  addresses, for tiled sources -- bit-exact, level chain 0.416-0.421 against 0.422-0.425 on packed input, +-0 in the bench: removed,
    //  profiles/r06_level_chain.md)
    if (r0 < RPP && !tilepath) {   // a row-major level
      if (interior) {
        // plain loads: non-temporal ones measured 0.46 -> 0.53 ms per level chain (neighbouring tiles share lines through L2)
        const uint8_t* p0 = S + (size_t)(oy - 3 + r0) * pitch + x;
#pragma unroll
        for (int k = 0; k < NLD; k++)
          v[k] = r0 + RPP * k < BT_H + 6 ? *reinterpret_cast<const uint32_t*>(p0 + (size_t)(RPP * k) * pitch) : 0u;
      } else {
        const bool whole = x >= 0 && x + 3 < w;
        int gx[4];
#pragma unroll
        for (int j = 0; j < 4; j++) gx[j] = reflect101(x + j, w);
#pragma unroll
        for (int k = 0; k < NLD; k++) {
          const int r = r0 + RPP * k;
          v[k] = 0u;
          if (r < BT_H + 6) {
            const int yy = reflect101(oy + r - 3, h);
            auto px = [&](int xx) { return (uint32_t)S[orbfe_level_offset(xx, yy, pitch, stiled)]; };
            if (whole) v[k] = *reinterpret_cast<const uint32_t*>(S + orbfe_level_offset(x, yy, pitch, stiled));
            else v[k] = px(gx[0]) | (px(gx[1]) << 8) | (px(gx[2]) << 16) | (px(gx[3]) << 24);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < NLD; k++) {
        const int r = r0 + RPP * k;
        if (r < BT_H + 6) in32[r * (BT_INP / 4) + BT_COL0 / 4 + c] = v[k];
      }
    }
    if (tilepath) {
      // A tiled level arrives as whole tile rows: the window's 6 x 9 tiles, eight lanes per tile (one 16-byte tile row each), so a
      // load instruction covers eight complete 128-byte lines -- 54 lines per window where the row-major form touches 124.
      // Rows of the first and last tile row outside the window are dropped at the store; tiles outside the plane are not read.
      // Only the window's 62 rows are requested: rows 5 .. 7 of the first tile row, the seven tile rows in between whole, rows 0 .. 2
      // of the last one (oy is a multiple of 56 = 7 x 8, so the window always starts at row 5 of a tile row) -- 372 pieces of 16 bytes.
      constexpr int N_TOP = 3 * 6, N_MID = 7 * 8 * 6, N_ALL = N_TOP + N_MID + 3 * 6;
      constexpr int NP = (N_ALL + THREADS - 1) / THREADS;
      const int ty0 = (oy - 3) >> 3, tx0 = (ox - 16) >> 4;   // (arithmetic shifts: -1 in the first tile row / column)
      const int tiles_y = (h + 7) >> 3, tiles_x = pitch >> 4;
      const uint32_t tstep = (uint32_t)tiles_x << 7;
      // piece -> (tile row, tile column, row inside the tile): eight (three) consecutive lanes share a tile
      // (integer forms of / 3 and / 6 for the small arguments here: (x * 43) >> 7 and >> 8; the mapping is computed once and kept --
      //  recomputing it for the stores was a tenth of the kernel's vector instructions)
      auto piece = [&](int pid, int& tyi, int& txi, int& rr) {
        if (pid < N_TOP) { txi = (pid * 43) >> 7; rr = 5 + pid - 3 * txi; tyi = 0; }
        else if (pid < N_TOP + N_MID) { const int q = pid - N_TOP, tl = q >> 3; rr = q & 7; tyi = (tl * 43) >> 8; txi = tl - 6 * tyi; tyi += 1; }
        else { const int q = pid - N_TOP - N_MID; txi = (q * 43) >> 7; rr = q - 3 * txi; tyi = 8; }
      };
      uint4 pv[NP];
      uint32_t lds_at[NP];
#pragma unroll
      for (int k = 0; k < NP; k++) {
        int tyi, txi, rr;
        piece(min(tid + k * THREADS, N_ALL - 1), tyi, txi, rr);
        const int tr = min(max(ty0 + tyi, 0), tiles_y - 1), tc = min(max(tx0 + txi, 0), tiles_x - 1);   // clamped: a valid address in any case
        pv[k] = *reinterpret_cast<const uint4*>(S + (uint32_t)tr * tstep + ((uint32_t)tc << 7) + (uint32_t)(rr * 16));
        lds_at[k] = (uint32_t)((tyi * 8 + rr - 5) * BT_INP + 16 * txi);   // window row (ty0 + tyi) * 8 + rr - (oy - 3)
      }
#pragma unroll
      for (int k = 0; k < NP; k++)
        if (tid + k * THREADS < N_ALL) *reinterpret_cast<uint4*>(in + lds_at[k]) = pv[k];
      if (!interior) {
        // REFLECT_101 at the level's edges, inside LDS: what the passes read outside the level is within three pixels of it, and
        // the pixels those reflect to lie inside the window.  Columns first (rows inside the level), then whole rows.
        __syncthreads();
        {
          const int nl = ox == 0 ? 3 : 0, nr = w < ox - 4 + 4 * NC ? 3 : 0;   // x = -3 .. -1; x = w .. w + 2
          for (int i = tid; i < (BT_H + 6) * (nl + nr); i += THREADS) {
            const int wr = (int)((i + 0.5f) * (1.0f / (float)(nl + nr))), j = i - wr * (nl + nr);
            const int xx = j < nl ? j - 3 : w + (j - nl);
            const int y = oy - 3 + wr;
            if (y >= 0 && y < h && xx - (ox - 16) < BT_INP)
              in[wr * BT_INP + (xx - (ox - 16))] = in[wr * BT_INP + (reflect101(xx, w) - (ox - 16))];
          }
        }
        __syncthreads();
        {
          const int nt = oy == 0 ? 3 : 0, nb = h < oy + BT_H + 3 ? 3 : 0;     // y = -3 .. -1; y = h .. h + 2
          for (int i = tid; i < (nt + nb) * (BT_INP / 4); i += THREADS) {
            const int j = (int)((i + 0.5f) * (1.0f / (float)(BT_INP / 4))), cdw = i - j * (BT_INP / 4);
            const int y = j < nt ? j - 3 : h + (j - nt);
            const int wr = y - (oy - 3), ws = reflect101(y, h) - (oy - 3);
            if (wr >= 0 && wr < BT_H + 6) in32[wr * (BT_INP / 4) + cdw] = in32[ws * (BT_INP / 4) + cdw];
          }
        }
      }
    }
  }
  if constexpr (RESIZE)
    if (tid < 16 * ORBFE_FUSE_ROWS) {
      const int ra = (int)(int16_t)(tyl.x & 0xffff) - (oy - 3), rb = (int)(int16_t)(tyl.x >> 16) - (oy - 3);
      ytap[tid] = make_uint4((uint32_t)(ra * BT_INP), (uint32_t)(rb * BT_INP), (tyl.y & 0xffffu) << 12, (tyl.y >> 16) << 12);
      const int yd = t.r0 + tid;
      ydst[tid] = rz.dst_tiled ? (uint32_t)(yd >> 3) * ((uint32_t)(rz.dpitch >> 4) << 7) + (uint32_t)((yd & 7) * 16) : (uint32_t)yd * (uint32_t)rz.dpitch;
    }
  __syncthreads();
  if constexpr (RESIZE) {
    // level + 1: the destination dword J of rows Y0 .. Y0 + 2.  Per source row three aligned LDS dwords, two v_alignbyte to start
    // the 8-byte window at the first pixel's source column, per pixel one v_perm (bytes s0, s0 + 1 into 16-bit fields) + one
    // v_dot2_u32_u16 against (c0, c1); (b * (t >> 4)) >> 16 == mul_hi_u24(b << 12, t & ~15).  Rows differ between the lanes of a
    // wave here, so the horizontal result of a source row is not carried over to the next destination row (a divergent test).
    typedef __attribute__((ext_vector_type(2))) unsigned short us2;
    if (J < t.j1) {
      const int s00 = (int)(int16_t)(txr[0].x & 0xffff);
      const int base = s00 - (ox - 4) + BT_COL0;   // >= 4 + BT_COL0: the dword's first source column lies in this tile column
      const uint32_t sh = (uint32_t)base & 3u;
      uint32_t sel[4], cp[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t o = (uint32_t)((int)(int16_t)(txr[i].x & 0xffff) - s00);   // 0 .. 6
        sel[i] = o | 0x0c000c00u | ((o + 1) << 16);
        cp[i] = txr[i].y;                                                         // c0 | c1 << 16
      }
      const uint32_t trow = (uint32_t)(uintptr_t)(in + (base & ~3));   // LDS byte address of the window column the taps start in
      // the three dwords of BOTH source rows in one block of LDS reads (ds_read2_b32 + ds_read_b32 off one address register per row:
      // a 4-byte aligned ds_read_b96 is slow, and every way of keeping the compiler from forming one -- an asm barrier on the pointer, a
      // volatile access -- turned the third dword into a flat_load_dword with a wait of its own)
      auto hrow2 = [&](uint32_t off_a, uint32_t off_b, uint32_t (&ha)[4], uint32_t (&hb)[4]) {
        unsigned long long a01, b01;
        uint32_t a2, b2;
        asm volatile("ds_read2_b32 %0, %4 offset1:1\n\t"
                     "ds_read_b32 %1, %4 offset:8\n\t"
                     "ds_read2_b32 %2, %5 offset1:1\n\t"
                     "ds_read_b32 %3, %5 offset:8\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(a01), "=&v"(a2), "=&v"(b01), "=&v"(b2)
                     : "v"(trow + off_a), "v"(trow + off_b)
                     : "memory");
        const uint32_t A0 = __builtin_amdgcn_alignbyte((uint32_t)(a01 >> 32), (uint32_t)a01, sh), A1 = __builtin_amdgcn_alignbyte(a2, (uint32_t)(a01 >> 32), sh);
        const uint32_t B0w = __builtin_amdgcn_alignbyte((uint32_t)(b01 >> 32), (uint32_t)b01, sh), B1w = __builtin_amdgcn_alignbyte(b2, (uint32_t)(b01 >> 32), sh);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const uint32_t ua = __builtin_amdgcn_perm(A1, A0, sel[i]), ub = __builtin_amdgcn_perm(B1w, B0w, sel[i]);
          ha[i] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, ua), __builtin_bit_cast(us2, cp[i]), 0u, false) & ~15u;
          hb[i] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, ub), __builtin_bit_cast(us2, cp[i]), 0u, false) & ~15u;
        }
      };
      // rows t.r0 + (tid >> 4), + THREADS / 16, ...: the row groups of a wave take consecutive rows
      // level + 1 is written in 16 x 8 tiles (orbfe_internal.h; row-major where a stand-alone kernel reads it next): the dword's
      // place inside its row / tile row is the thread's, the row's is the loop's
      uint8_t* Nimg = rz.dst + (size_t)img * rz.dimg;   // wave-uniform base; the offsets below are 32-bit (a plane is < 2^25 bytes)
      const uint32_t ncol = rz.dst_tiled ? (((uint32_t)((4 * J) >> 4) << 7) + (uint32_t)((4 * J) & 15)) : (uint32_t)(4 * J);
      for (int yi = tid >> 4; yi < t.r1 - t.r0; yi += THREADS / 16) {
        uint8_t* N = Nimg + (ncol + ydst[yi]);
        {
          const uint4 ty = ytap[yi];
          uint32_t h0[4], h1[4];
          hrow2(ty.x, ty.y, h0, h1);
          const uint32_t B0 = ty.z, B1 = ty.w;
          uint32_t sm[4];
#pragma unroll
          for (int i = 0; i < 4; i++) sm[i] = mulhi_u24(B0, h0[i]) + mulhi_u24(B1, h1[i]) + 2u;
          const uint32_t P01 = (sm[0] | (sm[1] << 16)) >> 2, P23 = (sm[2] | (sm[3] << 16)) >> 2;   // values <= 255 in bytes 0 and 2
          *reinterpret_cast<uint32_t*>(N) = __builtin_amdgcn_perm(P23, P01, 0x06040200u);
        }
      }
    }
  }
  {
    const int q = mlane >> 4, r = mlane & 15;
    const v4i c128 = {128, 128, 128, 128}, zero = {0, 0, 0, 0};
    const v4i cfin = {8388608 + 32768, 8388608 + 32768, 8388608 + 32768, 8388608 + 32768};
    v4i TB[4];   // requested here, used behind the first product: not live through the resize part above
#pragma unroll
    for (int b = 0; b < 4; b++) TB[b] = mtab[(1 + b) * 64 + mlane];
    const uint32_t bstep = (uint32_t)(dst.pitch[lvl] >> 4) << 8;      // 16 rows further: 2 tile rows x (pitch / 16) tiles x 128 bytes
#pragma unroll
    for (int g = mwave; g < BT_W / 16; g += THREADS / 64) {   // column group g: output columns 16g .. 16g + 15 of the tile
      v4i Xh, Xl;
      {
        const v4i* arow = reinterpret_cast<const v4i*>(in + r * BT_INP + 16 * g + 16 * q);   // window columns 16g + 16q ..: every tap of the group inside
        v4i A[4];
#pragma unroll
        for (int blk = 0; blk < 4; blk++) A[blk] = arow[blk * BT_INP];   // window rows 16 blk + r
        int ph[4], pl[4];
#pragma unroll
        for (int blk = 0; blk < 4; blk++) {
          const v4i d = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[blk] ^ (int)0x80808080, HB, c128, 0, 0, 0);
          blur_pack(d, ph[blk], pl[blk]);
        }
        Xh = v4i{ph[0], ph[1], ph[2], ph[3]};
        Xl = v4i{pl[0], pl[1], pl[2], pl[3]};
      }
      const int gx = ox + 16 * g + 4 * q;   // a multiple of 4: the four pixels lie in one storage-tile row
      uint8_t* o = D + blur_tiled_offset(gx, oy + r, dst.pitch[lvl]);   // output row oy + 16 b + r: two storage-tile rows further per block
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const v4i vh = __builtin_amdgcn_mfma_i32_16x16x64_i8(Xh, TB[b], zero, 0, 0, 0);
        const v4i vl = __builtin_amdgcn_mfma_i32_16x16x64_i8(Xl, TB[b], cfin, 0, 0, 0);
        const uint32_t r0 = ((uint32_t)vh.x << 8) + (uint32_t)vl.x, r1 = ((uint32_t)vh.y << 8) + (uint32_t)vl.y;
        const uint32_t r2 = ((uint32_t)vh.z << 8) + (uint32_t)vl.z, r3 = ((uint32_t)vh.w << 8) + (uint32_t)vl.w;
        const uint32_t out = __builtin_amdgcn_perm(r1, r0, 0x0c0c0602u) | __builtin_amdgcn_perm(r3, r2, 0x06020c0cu);
        const int row = 16 * b + r;
        // non-temporal: the blurred planes are next read by the descriptor gather, 0.5 GB of other traffic later, and so leave more
        // of the raw levels in the Infinity Cache for FAST (+0.5 % on the step)
        if (gx < w && row < BT_H && oy + row < h) __builtin_nontemporal_store(out, reinterpret_cast<uint32_t*>(o + b * bstep));
      }
    }
  }
}

// ---- the same blur on the matrix cores.  A 7-tap pass over a row is Out = In x Band, a band (Toeplitz) matrix of the taps; with
// pixels as i8 (x ^ 0x80 = x - 128) and taps <= 56 (folded REFLECT_101 taps <= 96) v_mfma_i32_16x16x64_i8 computes it exactly.
// One wave owns a strip of 48 output columns and walks down the level:
//   horizontal: A = 16 rows x 64 pixels, ONE aligned 16-byte load per lane straight into the operand layout (lane (q, r): row r,
//     pixels 16q .. 16q + 15 of the segment [48c - 16, 48c + 48)); the columns that have all seven taps inside the segment, on
//     4-pixel boundaries, are the strip: [48c - 12, 48c + 36).  B = the strip's three band matrices (64 x 16, from
//     the plan's table, in registers for the whole walk); C = 128.  D: lane (q, c) holds H - 32768 + 128 of rows 4q .. 4q + 3 of
//     column c -- a signed 16-bit number whose bytes (high, low ^ 0x80) are the i8 digits of H - 32768 = 256 a + b;
//   vertical: those bytes, packed four rows to a dword, ARE the operand of the second product: a lane's 16 bytes are the rows
//     16 ww + 4q + i (ww = 0..3 <-> dword, i <-> byte) of a 64-row window -- the K order of a matrix product is free as long as
//     both operands agree, and the other operand (the vertical band matrix, one pair for every window: rows outside the level are
//     loaded from their REFLECT_101 source) is written in that order.  With the
//     data as A and the band matrix as B the result comes out transposed: lane (q, r) holds columns 4q .. 4q + 3 of output row r,
//     one dword of the 16 x 8-tiled blurred plane.  V = 256 (T a) + (T b) + 256 * 32768, pixel = (V + 32768) >> 16 = byte 2.
// A window of four 16-row blocks yields the two middle ones; the walk advances by two blocks.  No LDS, no barrier.
#define BLUR_STAGES 2       // passes of source rows in flight per wave (LDS-DMA ring: 2 KB per pass and wave); BLUR_WAIT_ROWS counts on it
#ifndef BLUR_MIN_BLOCKS
#define BLUR_MIN_BLOCKS 4   // workgroups per CU the register allocation must leave room for
#endif
// One 1 KB piece (16 rows x 64 bytes) global -> LDS without passing registers: lane l's 16 bytes land at lds_dst + 16 l.  M0
// (the destination) is the compiler's register: saved and restored inside the statement.  The compiler does not count this
// load: every wait for it is the explicit BLUR_WAIT_ROWS below.
#define BLUR_DMA(gsrc, lds_dst) do { \
    unsigned keep_m0; \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" \
                 : "=&s"(keep_m0) : "v"(gsrc), "s"(lds_dst) : "memory"); \
  } while (0)
// vector-memory operations a wave issues AFTER the two pieces of pass p and before it reads them (at the end of pass p - 1):
// per pass in between two pieces and six stores (every lane stores in every pass): (BLUR_STAGES - 1) * 6 + (BLUR_STAGES - 2) * 2 = 6
static_assert(BLUR_STAGES == 2, "BLUR_WAIT_ROWS waits for vmcnt(6)");
#define BLUR_WAIT_ROWS() asm volatile("s_waitcnt vmcnt(6)" ::: "memory")
__global__ __launch_bounds__(256, BLUR_MIN_BLOCKS) void gauss_blur7_mfma_kernel(PyrView src, PyrView dst, BlurMfmaParams P) {
  const int lane = threadIdx.x & 63;
  const int sid = blockIdx.x * 4 + (threadIdx.x >> 6);
  __shared__ v4i ring[4][BLUR_STAGES][2][64];
  if (sid >= P.n_strips) return;
  const BlurStrip st = P.strips[sid];
  const int lvl = __builtin_amdgcn_readfirstlane((int)st.level), ch = __builtin_amdgcn_readfirstlane((int)st.chunk);
  const int w = src.w[lvl], h = src.h[lvl], sp = src.pitch[lvl], dp = dst.pitch[lvl];
  const uint8_t* S = src.base[lvl] + (size_t)blockIdx.y * src.img_stride[lvl];
  uint8_t* D = const_cast<uint8_t*>(dst.base[lvl]) + (size_t)blockIdx.y * dst.img_stride[lvl];
  const int q = lane >> 4, r = lane & 15;
  const v4i* bt = reinterpret_cast<const v4i*>(P.tab + P.b_off[lvl]) + (size_t)(ch * 3) * 64 + lane;
  const v4i B0 = bt[0], B1 = bt[64], B2 = bt[128];
  const v4i* tt = reinterpret_cast<const v4i*>(P.tab + P.t_off) + lane;
  const v4i T1 = tt[0], T2 = tt[64];
  // Load role: lane l fetches row l >> 2, 16-byte piece lc of the 64-byte segment -- four lanes read 64 contiguous bytes; a lane
  // loading its own operand bytes (16 rows per 16 consecutive lanes) costs four times the cache-line requests -- into LDS slot l.
  // The operand of lane (q, r), row r piece q, is then slot 4r + (q ^ (r >> 2 & 3)): the xor on the SOURCE piece spreads the
  // sixteen rows one b128 read serves over all banks.  A segment that would start left of the image or end right of the pitch
  // is moved inside: the band matrices hold zeros for every pixel outside [0, w).
  const int lrow = lane >> 2, lc = (lane & 3) ^ ((lane >> 4) & 3);
  const int xo = min(max(ORBFE_BLUR_CHUNK * ch - 16 + 16 * lc, 0), sp - 16);
  const int rslot = 4 * r + (q ^ ((r >> 2) & 3));
  const uint8_t* scol = S + xo;
  v4i* const wring = &ring[threadIdx.x >> 6][0][0][0];
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((int)(uint32_t)(size_t)(__attribute__((address_space(3))) v4i*)wring);
  const v4i c128 = {128, 128, 128, 128}, zero = {0, 0, 0, 0};
  const v4i cfin = {8388608 + 32768, 8388608 + 32768, 8388608 + 32768, 8388608 + 32768};
  // The two pieces of pass p: rows [32 p + 16, 32 p + 32) and [32 p + 32, 32 p + 48), into ring stage `stage`.  Rows outside
  // the level are fetched from their REFLECT_101 source row (one reflection, then clamped: only rows within three of the level
  // matter, and h >= 8), so the vertical band matrix is the plain Toeplitz one in every window.
#define BLUR_ROW(y) min(max((y) < 0 ? -(y) : ((y) >= h ? 2 * (h - 1) - (y) : (y)), 0), h - 1)
#define BLUR_REQUEST(p, stage) do { \
    const uint8_t* g0 = scol + (size_t)BLUR_ROW(32 * (p) + 16 + lrow) * sp; \
    const uint8_t* g1 = scol + (size_t)BLUR_ROW(32 * (p) + 32 + lrow) * sp; \
    BLUR_DMA(g0, lds0 + (uint32_t)(stage) * 2048u); \
    BLUR_DMA(g1, lds0 + (uint32_t)(stage) * 2048u + 1024u); \
  } while (0)
#define BLUR_HBLOCK(a, slot) do { \
    const v4i ax = (a) ^ (int)0x80808080; \
    const v4i d0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ax, B0, c128, 0, 0, 0); \
    const v4i d1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ax, B1, c128, 0, 0, 0); \
    const v4i d2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ax, B2, c128, 0, 0, 0); \
    int ph, pl; \
    blur_pack(d0, ph, pl); Xh[0].slot = ph; Xl[0].slot = pl; \
    blur_pack(d1, ph, pl); Xh[1].slot = ph; Xl[1].slot = pl; \
    blur_pack(d2, ph, pl); Xh[2].slot = ph; Xl[2].slot = pl; \
  } while (0)
  v4i Xh[3] = {zero, zero, zero}, Xl[3] = {zero, zero, zero};   // window blocks 0..3 <-> .x .y .z .w, per column group
  const int n_win = (h + ORBFE_BLUR_WINDOW - 1) / ORBFE_BLUR_WINDOW;
  // Pass s of the walk: first product for rows [32 s + 16, 32 s + 48) -- blocks 2 and 3 of window s --, second product for the
  // two middle blocks of the window, then the window moves down by two blocks.  Pass -1 only fills blocks 0 and 1 (rows -16 .. 15).  The rows of pass p are requested BLUR_STAGES passes ahead into stage
  // (p + 1) mod BLUR_STAGES.  Memory operations retire in issue order; inside a pass the order is: products; the next pass's rows
  // LDS -> operands (behind a counted wait: its pieces are older than exactly BLUR_YOUNGER operations); the request for the
  // pass whose stage this pass just vacated; this pass's stores.
  int st_cur = 0;   // stage of pass s
#pragma unroll
  for (int p = -1; p < BLUR_STAGES - 1; p++) BLUR_REQUEST(p, p + 1);
  const int dtile = dp >> 4;
  uint32_t xoff[3], rowoff[2];
  bool okx[3];
  const uint32_t trash = (uint32_t)dst.img_stride[lvl] - 256u + 4u * (uint32_t)lane;   // extractor.cpp: every plane ends in 256 spare bytes
#pragma unroll
  for (int g = 0; g < 3; g++) {
    const int x = ORBFE_BLUR_CHUNK * ch - 12 + 16 * g + 4 * q;   // a multiple of 4: the dword lies in one tile row
    okx[g] = x >= 0 && x < w;
    xoff[g] = ((uint32_t)(x >> 4) << 7) + (uint32_t)(x & 15);
  }
#pragma unroll
  for (int b = 0; b < 2; b++) {   // output row of pass -1: 16 b + r - 32 (never stored); the offset is taken modulo 2^32
    const int o = 16 * b + r;
    rowoff[b] = (((uint32_t)(o >> 3) * (uint32_t)dtile) << 7) + (uint32_t)((o & 7) * 16) - ((uint32_t)dtile << 9);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the first pieces (and this wave's tables) have landed
  v4i A2 = wring[rslot], A3 = wring[64 + rslot];
  for (int s = -1; s < n_win; s++) {
    BLUR_HBLOCK(A2, z);
    BLUR_HBLOCK(A3, w);
    uint32_t out[3][2] = {{0u, 0u}, {0u, 0u}, {0u, 0u}};
    if (s >= 0) {
#pragma unroll
      for (int g = 0; g < 3; g++) {
#pragma unroll
        for (int b = 0; b < 2; b++) {
          const v4i T = b ? T2 : T1;
          const v4i vh = __builtin_amdgcn_mfma_i32_16x16x64_i8(Xh[g], T, zero, 0, 0, 0);
          const v4i vl = __builtin_amdgcn_mfma_i32_16x16x64_i8(Xl[g], T, cfin, 0, 0, 0);
          const uint32_t r0 = ((uint32_t)vh.x << 8) + (uint32_t)vl.x, r1 = ((uint32_t)vh.y << 8) + (uint32_t)vl.y;
          const uint32_t r2 = ((uint32_t)vh.z << 8) + (uint32_t)vl.z, r3 = ((uint32_t)vh.w << 8) + (uint32_t)vl.w;
          out[g][b] = __builtin_amdgcn_perm(r1, r0, 0x0c0c0602u) | __builtin_amdgcn_perm(r3, r2, 0x06020c0cu);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < 3; g++) {
      Xh[g].x = Xh[g].z; Xh[g].y = Xh[g].w;
      Xl[g].x = Xl[g].z; Xl[g].y = Xl[g].w;
    }
    // rows of pass s + 1: LDS -> operands
    const int st_next = st_cur + 1 == BLUR_STAGES ? 0 : st_cur + 1;
    BLUR_WAIT_ROWS();
    A2 = wring[st_next * 128 + rslot];
    A3 = wring[st_next * 128 + 64 + rslot];
    BLUR_REQUEST(s + BLUR_STAGES, st_cur);   // the stage of pass s was read a pass ago
    st_cur = st_next;
    // this pass's stores: the tiled offset of (x, o) splits into a column part (fixed for the strip) and a row part that
    // advances by four tile rows per pass.  Every lane stores in every pass -- a store under a condition is a branch to the
    // compiler, and BLUR_WAIT_ROWS counts on six stores per pass: a dword outside the level goes to the lane's own slot
    // in the 256 spare bytes behind the plane
    {
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const bool oky = s >= 0 && ORBFE_BLUR_WINDOW * s + 16 * b + r < h;
#pragma unroll
        for (int g = 0; g < 3; g++)
          *reinterpret_cast<uint32_t*>(D + ((oky && okx[g]) ? rowoff[b] + xoff[g] : trash)) = out[g][b];
        rowoff[b] += (uint32_t)dtile << 9;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // pieces requested past the last pass must not land in LDS after the wave has gone
#undef BLUR_REQUEST
#undef BLUR_ROW
#undef BLUR_HBLOCK
}

// ------------------------------------------------------------------------------------------------ launchers
void orbfe_launch_copy0(const uint8_t* src, int sstride, size_t simg, uint8_t* dst, int dpitch, size_t dimg, int w,
                        int h, int n_images, int tiled, hipStream_t s) {
  dim3 block(256), grid((((w + 15) / 16) * h + 255) / 256, 1, n_images);
  hipLaunchKernelGGL(copy_level0_kernel, grid, block, 0, s, src, sstride, (unsigned long long)simg, dst, dpitch,
                     (unsigned long long)dimg, w, h, tiled);
}

void orbfe_launch_resize(const uint8_t* src, int spitch, size_t simg, uint8_t* dst, int dpitch, size_t dimg, int dw,
                         int dh, const ResizeTap* xt, const ResizeTap* yt, int n_images, int mode, hipStream_t s) {
  dim3 block(64, 4), grid((dw + 255) / 256, (dh + 3) / 4, n_images);
  if (mode >= 2) {   // scale <= 2 and taps within 8 source bytes: persistent workgroups, perm + dot2 interpolation
#ifndef RS_WGS_NARROW
#define RS_WGS_NARROW 7   // 6: 0.262, 7: 0.254, 8: 0.268 ms per pyramid of 256 images
#endif
    const int wgs = mode == 3 ? RS_WGS_NARROW : 6;   // workgroups per CU (mode 3: every window fits 21 chunks, 14 KB of LDS)
    const int tiles_x = (dw + 255) / 256, tiles_y = (dh + 31) / 32;
    const int n_tiles = tiles_x * tiles_y * n_images;
    const int nb = n_tiles < 256 * wgs ? n_tiles : 256 * wgs;
    if (mode == 3)
      hipLaunchKernelGGL((pyr_resize_dot_kernel<32, 42, 336>), dim3(nb), block, 0, s, src, spitch, (unsigned long long)simg, dst,
                         dpitch, (unsigned long long)dimg, dw, dh, xt, yt, tiles_x, tiles_y, n_tiles);
    else
      hipLaunchKernelGGL((pyr_resize_dot_kernel<32, 42, RS_COLS>), dim3(nb), block, 0, s, src, spitch, (unsigned long long)simg, dst,
                         dpitch, (unsigned long long)dimg, dw, dh, xt, yt, tiles_x, tiles_y, n_tiles);
  }
  else if (mode >= 1)
    hipLaunchKernelGGL(pyr_resize_lds16_kernel, dim3((dw + 255) / 256, (dh + 15) / 16, n_images), block, 0, s, src, spitch,
                       (unsigned long long)simg, dst, dpitch, (unsigned long long)dimg, dw, dh, xt, yt);
  else  // source window of a tile exceeds the staged size (scale factor > 2): direct byte gathers
    hipLaunchKernelGGL(pyr_resize_kernel, grid, block, 0, s, src, spitch, (unsigned long long)simg, dst, dpitch,
                       (unsigned long long)dimg, dw, dh, xt, yt);
}

// Which blur runs: measured on 256 KITTI images (profiles/r04_blur_mfma.md, DESIGN lesson 31) the matrix-core kernel does the
// arithmetic of the LDS kernel in a third of the vector instructions and is bit-exact, but the stage moves 0.74 GB per launch
// and both kernels take 0.29-0.32 ms for it; the LDS kernel is a few per cent ahead and is what a handle uses unless
// orbfe_debug_blur_kernel() selects the other one (the parity test of the matrix-core kernel does).
void orbfe_launch_blur(const PyrView& src, const PyrView& dst, const BlurTile* tiles, int n_tiles, const BlurMfmaParams& mf,
                       int n_images, hipStream_t s) {
  if (mf.use && mf.n_strips > 0) {
    hipLaunchKernelGGL(gauss_blur7_mfma_kernel, dim3((mf.n_strips + 3) / 4, n_images), dim3(256), 0, s, src, dst, mf);
    return;
  }
  orbfe_launch_blur_level(src, dst, tiles, n_tiles, nullptr, n_images, s);
}

void orbfe_launch_blur_level(const PyrView& src, const PyrView& dst, const BlurTile* tiles, int n_tiles, const LevelResize* rz,
                             int n_images, hipStream_t s) {
  if (n_tiles <= 0) return;
  dim3 grid(n_tiles, n_images);
  // a batch wants many tiles in flight per CU (two waves per tile); a one- or two-image call has fewer tiles than the chip has CUs
  // and wants each tile done quickly (four waves per tile: 0.292 -> 0.27 ms for a stereo pair's two extractions)
  const bool few = n_images <= 8;
  if (rz) {
    if (few) hipLaunchKernelGGL((blur_level_kernel<true, 256>), grid, dim3(256), 0, s, src, dst, tiles, n_tiles, *rz);
    else hipLaunchKernelGGL((blur_level_kernel<true, BT_THREADS>), grid, dim3(BT_THREADS), 0, s, src, dst, tiles, n_tiles, *rz);
  } else {
    if (few) hipLaunchKernelGGL((blur_level_kernel<false, 256>), grid, dim3(256), 0, s, src, dst, tiles, n_tiles, LevelResize{});
    else hipLaunchKernelGGL((blur_level_kernel<false, BT_THREADS>), grid, dim3(BT_THREADS), 0, s, src, dst, tiles, n_tiles, LevelResize{});
  }
}

int orbfe_upload_blur_bands() {
  // band matrices of the tile kernel's matrix-core blur (blur_level_kernel): lane (q, n) of a matrix holds 16 bytes.
  //   horizontal (one for every column group g): byte j <-> LDS column 16g + 16q + j, output = LDS column BT_COL0 + 4 + 16g + n
  //   vertical, block b:  byte j = 4 ww + i <-> window row 16 ww + 4q + i, output = window row 3 + 16b + n
  static const int taps[7] = {18, 34, 48, 56, 48, 34, 18};
  static int8_t bt[5 * 1024];
  for (int m = 0; m < 5; m++)
    for (int lane = 0; lane < 64; lane++)
      for (int j = 0; j < 16; j++) {
        const int q = lane >> 4, n = lane & 15;
        const int d = m == 0 ? (16 * q + j) - (4 + BT_COL0 + n) : (16 * (j >> 2) + 4 * q + (j & 3)) - (3 + 16 * (m - 1) + n);
        bt[(m * 64 + lane) * 16 + j] = (int8_t)(d >= -3 && d <= 3 ? taps[d + 3] : 0);
      }
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_blur_tile_tab), bt, sizeof(bt));
}
