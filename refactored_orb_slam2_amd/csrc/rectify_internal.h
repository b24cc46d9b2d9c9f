// rectify_internal.h -- the per-pixel arithmetic of stereo rectification that the batch kernel (rectify_kernels.hip) and the host
// routines (rectify.cpp: orbfe_rectifier_create, orbfe_rectify_image) share.  One definition, compiled for both sides with
// -ffp-contract=off; the per-pixel part is integer arithmetic, so host and device produce the same bytes.
//
// Reference: Source/Examples/Stereo/stereo_euroc.cc:108-111 (cv::initUndistortRectifyMap(K, D, R, P(0:3, 0:3), size, CV_32F) once
// per eye) and :159-160 (cv::remap(..., cv::INTER_LINEAR) of both images of every frame).  No OpenCV exists where this library is
// built and tested: what follows is this project's reading of OpenCV 4.5's scalar paths, as unpinned as the other OpenCV
// primitives.
//
// remap with CV_32F maps and 8-bit pixels works in fixed point: INTER_BITS = 5 (coordinates in 1/32 pixel) and 15-bit weights.
//   sx = rint(map_x * 32.0f) (a float product, round half to even), X = sx >> 5, ax = sx & 31; sy, Y, ay likewise
//   taps (Y, X) (Y, X + 1) (Y + 1, X) (Y + 1, X + 1), weights 32 (32 - ax)(32 - ay), 32 ax (32 - ay), 32 (32 - ax) ay, 32 ax ay:
//   OpenCV's bilinear table; every entry is an exact integer and every four sum to 32 768, so its rounding / correction step never
//   acts.  A tap outside the source reads 0 (BORDER_CONSTANT, value 0).  out = (sum + 16384) >> 15 = (sum / 32 + 512) >> 10.
// The fixed-point map depends on the camera only: it is computed once (orbfe_rect_entry) and kept as two planes,
//   xy    uint32  (X + 1) | (Y + 1) << 13 | class << 26   X + 1, Y + 1 in 0 .. 4095 for every pixel that reads the source
//   frac  uint16  ax | ay << 5
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/orbfe.h"

#define ORBFE_RECT_INNER 0u     // all four taps inside the source
#define ORBFE_RECT_EDGE 1u      // some taps inside
#define ORBFE_RECT_OUTSIDE 2u   // no tap inside (or a coordinate that is not finite / not an int32): the pixel is 0
#define ORBFE_RECT_CLASS_SHIFT 26
#define ORBFE_RECT_BORDER_MASK (3u << ORBFE_RECT_CLASS_SHIFT)   // any bit set: the pixel needs the per-tap checks

// the fixed-point step of one map entry for a sw x sh source (1 .. 4095 per side)
__host__ __device__ inline void orbfe_rect_entry(float map_x, float map_y, int sw, int sh, uint32_t* xy, uint16_t* frac) {
  const float fx = map_x * 32.0f, fy = map_y * 32.0f;
  *xy = ORBFE_RECT_OUTSIDE << ORBFE_RECT_CLASS_SHIFT;
  *frac = 0;
  // finite and inside int32 (2147483648.0f is exact; NaN fails the comparisons)
  if (!(fx >= -2147483648.0f && fx < 2147483648.0f && fy >= -2147483648.0f && fy < 2147483648.0f)) return;
  const int32_t sx = (int32_t)rintf(fx), sy = (int32_t)rintf(fy);
  const int32_t X = sx >> 5, Y = sy >> 5;
  if (X < -1 || X >= sw || Y < -1 || Y >= sh) return;
  const bool inner = X >= 0 && X + 1 < sw && Y >= 0 && Y + 1 < sh;
  *xy = (uint32_t)(X + 1) | (uint32_t)(Y + 1) << 13 | (inner ? ORBFE_RECT_INNER : ORBFE_RECT_EDGE) << ORBFE_RECT_CLASS_SHIFT;
  *frac = (uint16_t)((sx & 31) | (sy & 31) << 5);
}

// (sum of tap x a x b + 512) >> 10 with a in {32 - ax, ax}, b in {32 - ay, ay}: rows first, exact in 32-bit integers
__host__ __device__ inline uint32_t orbfe_rect_blend(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11, uint32_t ax, uint32_t ay) {
  const uint32_t h0 = t00 * (32u - ax) + t01 * ax;
  const uint32_t h1 = t10 * (32u - ax) + t11 * ax;
  return (h0 * (32u - ay) + h1 * ay + 512u) >> 10;
}

// one destination pixel of any class from a pitched sw x sh source; reads nothing outside it
__host__ __device__ inline uint8_t orbfe_rect_pixel(const uint8_t* src, size_t pitch, int sw, int sh, uint32_t xy, uint32_t frac) {
  if ((xy >> ORBFE_RECT_CLASS_SHIFT) & ORBFE_RECT_OUTSIDE) return 0;
  const int X = (int)(xy & 8191u) - 1, Y = (int)((xy >> 13) & 8191u) - 1;
  const bool x0 = X >= 0, x1 = X + 1 < sw, y0 = Y >= 0, y1 = Y + 1 < sh;
  const uint8_t* r0 = src + (size_t)(y0 ? Y : 0) * pitch;
  const uint8_t* r1 = src + (size_t)(y1 ? Y + 1 : sh - 1) * pitch;
  const int c0 = x0 ? X : 0, c1 = x1 ? X + 1 : sw - 1;
  const uint32_t t00 = (x0 && y0) ? r0[c0] : 0u, t01 = (x1 && y0) ? r0[c1] : 0u;
  const uint32_t t10 = (x0 && y1) ? r1[c0] : 0u, t11 = (x1 && y1) ? r1[c1] : 0u;
  return (uint8_t)orbfe_rect_blend(t00, t01, t10, t11, frac & 31u, (frac >> 5) & 31u);
}

// The destination is cut into tiles of RECT_TILE_W x RECT_TILE_H pixels, one workgroup each.  A tile all of whose pixels are inner
// has a source window: the bounding box of its taps, x0 rounded down and w rounded up to 4, computed once per camera.  w = 0: no
// window (border pixels in the tile, a window above RECT_WIN_DWORDS dwords, or one whose rounded width leaves the source row);
// such a tile gathers straight from memory.
#define RECT_TILE_W 128   // 32 lanes x 4 pixels
#define RECT_TILE_H 8     // 4 waves x 2 rows
#define RECT_WIN_DWORDS 1024
struct RectWin {
  int16_t x0, y0, w, h;
};

// the device side of a rectifier: the fixed-point map planes in HBM, rows of `wq` entries (dst_width rounded up to 4; the
// padding entries are class OUTSIDE and never stored)
struct RectMap {
  const uint32_t* xy;
  const uint16_t* frac;
  const RectWin* win;   // [tile row][tile column]
  int wq;
  int dst_w, dst_h, src_w, src_h;
};

void orbfe_launch_rectify(const RectMap& m, const uint8_t* src, int n_images, int src_pitch, size_t src_image_bytes, uint8_t* dst,
                          int dst_pitch, size_t dst_image_bytes, hipStream_t s);
