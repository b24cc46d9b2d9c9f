// rectify_kernels.hip -- cv::remap(..., INTER_LINEAR) of a batch of 8-bit images through one camera's fixed-point map
// (Source/Examples/Stereo/stereo_euroc.cc:159-160 of the reference; the arithmetic is rectify_internal.h's, shared with the host).
//
// The map is the same for every image of a batch and as large as an image pair (6 bytes per pixel against 1 read + 1 written), so
// a workgroup owns a tile of 128 x 8 destination pixels, loads the tile's map entries ONCE into registers and walks the images
// of the batch with them: gridDim.y groups of images, image f = blockIdx.y, + gridDim.y, ...  A lane produces 4 adjacent
// destination pixels (one uint4 + one uint2 of map, one dword store); 32 lanes write a whole 128-byte line, a wave two rows.
// The source is gathered straight through L1 / L2: neighbouring destination pixels read neighbouring source pixels (the EuRoC
// maps move by 37 source rows over 752 columns), the two taps of a row come from one 16-bit load.  Staging each tile's source
// window in LDS instead (RECT_LDS_WINDOW=1: aligned dword loads, two barriers per image) measured 0.656 ms against 0.35 ms for 512
// EuRoC images and is off; the kernel waits on the vector-memory path's handling of the per-lane gathers, not on bytes (profiles/rectify.md).  Whether a pixel needs the
// border checks is in its map entry; a wave none of whose 256 pixels does -- every wave of a calibration without edge / outside
// pixels -- takes the path without them, decided once per tile, outside the image loop.
#include "rectify_internal.h"

#define RECT_THREADS 256
#ifndef RECT_LDS_WINDOW
#define RECT_LDS_WINDOW 0   // 1: tiles with a source window stage it in LDS (the A/B of profiles/rectify.md: slower)
#endif

__device__ __forceinline__ uint32_t load_pair(const uint8_t* p) {   // bytes p[0] | p[1] << 8, any alignment
  uint16_t v;
  __builtin_memcpy(&v, p, 2);
  return v;
}

__global__ __launch_bounds__(RECT_THREADS) void rectify_batch_kernel(RectMap m, const uint8_t* __restrict__ src, int n_images,
                                                                     size_t src_pitch, size_t src_image_bytes,
                                                                     uint8_t* __restrict__ dst, size_t dst_pitch,
                                                                     size_t dst_image_bytes, int dword_stores, int use_windows) {
#if RECT_LDS_WINDOW
  __shared__ uint32_t win[RECT_WIN_DWORDS];
#endif
  const int tid = threadIdx.x;
  const int x = blockIdx.x * RECT_TILE_W + (tid & 31) * 4;
  const int y = blockIdx.z * RECT_TILE_H + (tid >> 5);
  const bool live = x < m.dst_w && y < m.dst_h;
  uint32_t xy[4] = {ORBFE_RECT_OUTSIDE << ORBFE_RECT_CLASS_SHIFT, ORBFE_RECT_OUTSIDE << ORBFE_RECT_CLASS_SHIFT,
                    ORBFE_RECT_OUTSIDE << ORBFE_RECT_CLASS_SHIFT, ORBFE_RECT_OUTSIDE << ORBFE_RECT_CLASS_SHIFT};
  uint32_t fr[4] = {0, 0, 0, 0};
  if (live) {   // x is a multiple of 4 and below wq: the row's entries are 16- / 8-byte aligned
    const size_t e = (size_t)y * m.wq + x;
    const uint4 a = *reinterpret_cast<const uint4*>(m.xy + e);
    const uint2 b = *reinterpret_cast<const uint2*>(m.frac + e);
    xy[0] = a.x; xy[1] = a.y; xy[2] = a.z; xy[3] = a.w;
    fr[0] = b.x & 0xffffu; fr[1] = b.x >> 16; fr[2] = b.y & 0xffffu; fr[3] = b.y >> 16;
  }
  const int n_px = live ? min(4, m.dst_w - x) : 0;
  const bool border = __any((int)(live && (((xy[0] | xy[1] | xy[2] | xy[3]) & ORBFE_RECT_BORDER_MASK) != 0u)));
  const size_t out_off = (size_t)y * dst_pitch + x;
  const bool wide = dword_stores && n_px == 4;

#if RECT_LDS_WINDOW
  // ---- a tile with a source window: the workgroup stages the window of each image in LDS with aligned dword loads (the next
  // image's loads are issued before this image's taps are read) and every tap comes from LDS
  RectWin wv = {0, 0, 0, 0};
  if (use_windows) wv = m.win[blockIdx.z * gridDim.x + blockIdx.x];   // uniform
  if (wv.w != 0) {
    const int wq = wv.w >> 2, nd = wq * wv.h;
    size_t goff[4];
    bool gv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int i = tid + k * RECT_THREADS;
      gv[k] = i < nd;
      const int rr = i / wq, cc = i - rr * wq;
      goff[k] = gv[k] ? (size_t)(wv.y0 + rr) * src_pitch + (size_t)(wv.x0 + 4 * cc) : 0;
    }
    uint32_t lo[4], ax[4], ay[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {   // the tile has no border pixel: every live lane holds four inner pixels
      const int X = (int)(xy[k] & 8191u) - 1, Y = (int)((xy[k] >> 13) & 8191u) - 1;
      lo[k] = live ? (uint32_t)((Y - wv.y0) * wv.w + (X - wv.x0)) : 0u;
      ax[k] = fr[k] & 31u;
      ay[k] = (fr[k] >> 5) & 31u;
    }
    const uint8_t* wb = reinterpret_cast<const uint8_t*>(win);
    uint32_t v[4] = {0, 0, 0, 0};
    int f = blockIdx.y;
    if (f < n_images) {
      const uint8_t* s = src + (size_t)f * src_image_bytes;
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (gv[k]) v[k] = *reinterpret_cast<const uint32_t*>(s + goff[k]);
    }
    for (; f < n_images; f += gridDim.y) {
      __syncthreads();   // the taps of the image before have been read
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (gv[k]) win[tid + k * RECT_THREADS] = v[k];
      __syncthreads();
      if (f + (int)gridDim.y < n_images) {
        const uint8_t* s = src + (size_t)(f + gridDim.y) * src_image_bytes;
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (gv[k]) v[k] = *reinterpret_cast<const uint32_t*>(s + goff[k]);
      }
      if (live) {
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t r0 = load_pair(wb + lo[k]), r1 = load_pair(wb + lo[k] + wv.w);
          o[k] = orbfe_rect_blend(r0 & 255u, r0 >> 8, r1 & 255u, r1 >> 8, ax[k], ay[k]);
        }
        uint8_t* d = dst + (size_t)f * dst_image_bytes + out_off;
        if (dword_stores) {
          *reinterpret_cast<uint32_t*>(d) = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
        } else {
#pragma unroll
          for (int k = 0; k < 4; k++) d[k] = (uint8_t)o[k];
        }
      }
    }
    return;
  }
#endif

  if (!border) {   // wave-uniform: every live lane holds four inner pixels (a padding entry behind dst_w would have set `border`)
    if (!live) return;
    size_t off[4];
    uint32_t ax[4], ay[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      off[k] = (size_t)(((xy[k] >> 13) & 8191u) - 1u) * src_pitch + ((xy[k] & 8191u) - 1u);
      ax[k] = fr[k] & 31u;
      ay[k] = (fr[k] >> 5) & 31u;
    }
    for (int f = blockIdx.y; f < n_images; f += gridDim.y) {
      const uint8_t* s = src + (size_t)f * src_image_bytes;
      uint32_t r0[4], r1[4], o[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {   // inner: X + 1 < src_w and Y + 1 < src_h, so neither pair leaves its row or the image
        r0[k] = load_pair(s + off[k]);
        r1[k] = load_pair(s + off[k] + src_pitch);
      }
#pragma unroll
      for (int k = 0; k < 4; k++) o[k] = orbfe_rect_blend(r0[k] & 255u, r0[k] >> 8, r1[k] & 255u, r1[k] >> 8, ax[k], ay[k]);
      uint8_t* d = dst + (size_t)f * dst_image_bytes + out_off;
      if (dword_stores) {
        *reinterpret_cast<uint32_t*>(d) = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = (uint8_t)o[k];
      }
    }
    return;
  }
  for (int f = blockIdx.y; f < n_images; f += gridDim.y) {
    const uint8_t* s = src + (size_t)f * src_image_bytes;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = orbfe_rect_pixel(s, src_pitch, m.src_w, m.src_h, xy[k], fr[k]);
    uint8_t* d = dst + (size_t)f * dst_image_bytes + out_off;
    if (wide) {
      *reinterpret_cast<uint32_t*>(d) = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
    } else {
      for (int k = 0; k < n_px; k++) d[k] = (uint8_t)o[k];
    }
  }
}

void orbfe_launch_rectify(const RectMap& m, const uint8_t* src, int n_images, int src_pitch, size_t src_image_bytes, uint8_t* dst,
                          int dst_pitch, size_t dst_image_bytes, hipStream_t s) {
  if (n_images < 1) return;
  const int tx = (m.dst_w + RECT_TILE_W - 1) / RECT_TILE_W, ty = (m.dst_h + RECT_TILE_H - 1) / RECT_TILE_H;
  // image groups: enough workgroups to fill the chip several times over (256 CUs x 8 workgroups of 256 threads), each walking
  // n_images / groups images with its map entries in registers
  const long tiles = (long)tx * ty;
  long groups = (4096 + tiles - 1) / tiles;
  if (groups > n_images) groups = n_images;
  if (groups > 65535) groups = 65535;
  if (groups < 1) groups = 1;
  const int dword_stores = (((uintptr_t)dst | (uintptr_t)dst_pitch | (uintptr_t)dst_image_bytes) & 3) == 0;
  // the windows are staged with dword loads: the source rows must be 4-byte aligned
  const int use_windows = RECT_LDS_WINDOW && (((uintptr_t)src | (uintptr_t)src_pitch | (uintptr_t)src_image_bytes) & 3) == 0;
  const dim3 grid((unsigned)tx, (unsigned)groups, (unsigned)ty), block(RECT_THREADS);
  hipLaunchKernelGGL(rectify_batch_kernel, grid, block, 0, s, m, src, n_images, (size_t)src_pitch, src_image_bytes, dst,
                     (size_t)dst_pitch, dst_image_bytes, dword_stores, use_windows);
}
