/*
 * orbfe.h -- C ABI of liborbfe.so: the MI355X (gfx950) ORB front end.
 *
 * This is the drop-in boundary for ORB-SLAM2's per-frame feature front end.  The reference
 * (sjulier/Refactored_ORB_SLAM2) has no FFI for this path: the boundary there is two C++ classes,
 *   ORB_SLAM2::ORBextractor  (Source/Libraries/ORB_SLAM2/include/ORBextractor.h:43-104)
 *   ORB_SLAM2::ORBmatcher    (Source/Libraries/ORB_SLAM2/include/ORBmatcher.h:34-114)
 * and Frame's window query / stereo association (Source/Libraries/ORB_SLAM2/src/Frame.cc:250-263,
 * 341-410, 477-646).  The C++ classes shipped in refactored_orb_slam2_amd/csrc/host/ keep those exact
 * signatures and forward to the entry points below, so Tracking.cc / Frame.cc link unchanged
 * (INTEGRATION.md).  Everything here is plain C: opaque handles, POD structs, pointers and sizes; every
 * function returns ORBFE_OK (0) or a negative error code and never throws.  There is NO CPU fallback:
 * without a HIP device every compute entry point returns ORBFE_ERR_NO_DEVICE.
 *
 * L/ = Source/Libraries/ORB_SLAM2/ of the reference checkout.
 */
#ifndef ORBFE_H
#define ORBFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBFE_VERSION 100

enum {
  ORBFE_OK = 0,
  ORBFE_ERR_INVALID = -1,    /* bad argument (null pointer, unsupported size, bad parameter) */
  ORBFE_ERR_CAPACITY = -2,   /* an output buffer or an internal fixed-size table is too small */
  ORBFE_ERR_NO_DEVICE = -3,  /* no usable HIP device / HIP runtime failure at start-up */
  ORBFE_ERR_HIP = -4,        /* a HIP call failed; orbfe_last_error() has the text */
  ORBFE_ERR_EMPTY = -5,      /* empty input image: outputs untouched (L/src/ORBextractor.cc:981-982) */
  ORBFE_ERR_ALLOC = -6       /* a host memory allocation failed */
};

#define ORBFE_MAX_LEVELS 16
#define ORBFE_GRID_COLS 64   /* FRAME_GRID_COLS, L/include/Frame.h:37 */
#define ORBFE_GRID_ROWS 48   /* FRAME_GRID_ROWS, L/include/Frame.h:36 */
#define ORBFE_TH_HIGH 100    /* ORBmatcher::TH_HIGH, L/src/ORBmatcher.cc:38 */
#define ORBFE_TH_LOW 50      /* ORBmatcher::TH_LOW,  L/src/ORBmatcher.cc:39 */
#define ORBFE_HISTO_LENGTH 30

/* Constructor arguments of ORBextractor (L/src/ORBextractor.cc:407-410) */
typedef struct orbfe_params {
  int32_t n_features;
  float scale_factor;
  int32_t n_levels;
  int32_t ini_th_fast;
  int32_t min_th_fast;
} orbfe_params;

/* Layout-identical to cv::KeyPoint (pt.x, pt.y, size, angle, response, octave, class_id; 28 bytes) */
typedef struct orbfe_keypoint {
  float x, y;
  float size;
  float angle;
  float response;
  int32_t octave;
  int32_t class_id;
} orbfe_keypoint;

typedef struct orbfe_extractor orbfe_extractor;

const char* orbfe_last_error(void);   /* thread-local text of the last failure on this thread */
int orbfe_device_count(int* count);   /* number of visible HIP devices */
/* For hosts that do not link the HIP runtime themselves: the calling thread's current device (handles created with device = -1,
 * the per-thread matcher handle and the C++ drop-in classes use it), and plain device memory with synchronous copies (a C / C++
 * caller of the batched mode keeps its per-frame records in HBM for orbfe_gather_records). */
int orbfe_set_device(int device);
int orbfe_device_malloc(size_t bytes, void** out);
int orbfe_device_free(void* p);
int orbfe_device_upload(void* d_dst, const void* h_src, size_t bytes);
int orbfe_device_download(void* h_dst, const void* d_src, size_t bytes);

/* Hard limits (checked, ORBFE_ERR_INVALID beyond them):
 *   images              at most 4095 x 4095 pixels (keypoint coordinates travel between kernels as 12-bit fields) and at least
 *                       one FAST cell per level the caller wants keypoints from (a level narrower or lower than 2 x 16 + 30
 *                       pixels yields none, where the reference divides by zero, L/src/ORBextractor.cc:753-754)
 *   pyramid             n_levels <= ORBFE_MAX_LEVELS (16); FAST cells <= 66 x 66 pixels
 *   descriptor sets     fewer than 65 536 descriptors per frame / per set (orbfe_hamming_bf_device, orbfe_stereo_match*:
 *                       indices travel as 16-bit fields next to the distance)
 *   projection searches at most 9 500 keypoints per frame (orbfe_search_by_projection_*, orbfe_search_local_points*,
 *                       orbfe_proj_match_batch_device, orbfe_kf_search in its LOOP / RELOC modes: the ordered resolver keeps
 *                       nine bytes per keypoint in LDS); orbfe_proj_candidates / orbfe_proj_best alone take 65 535
 *   stereo matching     (image rows / 8, rounded up) x n_levels <= 8 192 row-bucket keys, rows <= 4 095, and pyramid scale
 *                       factors mvScaleFactor[level] <= 13 (2 x scale + 2 <= 28 rows: a keypoint's row band spans at most
 *                       8 buckets), e.g. 16 levels at a scale factor of 1.18648 or less
 *   inv_level_sigma2    orbfe_proj_best / orbfe_kf_search read n_levels floats (the caller states n_levels)
 *   octree node table   max(N + 3, 4 x nIni) + 1, rounded up to 64, for every level's feature quota N: at most 2 752 nodes,
 *                       56 bytes each in the 160 KiB of LDS of the octree kernel (the table itself is sized for 8 192), so
 *                       nFeatures <= 12 655 at 8 levels and scale factor 1.2
 *   aspect ratio        nIni = round(width / height) of every level with FAST cells (width, height: the level less its
 *                       16-pixel borders) in 1..256: images much taller than wide are refused (a 4095-row image at 16 levels
 *                       and scale factor 1.18648 needs about 2 100 columns)
 *   SearchByBoW         at most 60 000 frame features under one vocabulary node (orbfe_search_by_bow, orbfe_search_by_bow_kf)
 *   RGB-D depth maps    at most 4095 x 4095 samples (orbfe_undistort_frames_device); a keypoint whose truncated coordinates fall
 *                       outside its frame's depth map gets no depth (mvDepth = mvuRight = -1) and nothing outside the map is read
 *                       -- the reference would read out of bounds there; the extractor never produces such a keypoint
 *   rectification       source and destination images of 1 .. 4095 pixels per side (orbfe_rectifier_create: the fixed-point map keeps
 *                       X + 1 and Y + 1 in 13 bits each); pitches at least the widths, image strides at least (height - 1) x pitch
 *                       + width, source and destination must not overlap (orbfe_rectify_batch_device)
 *   pose optimisation   at most 9 500 keypoint rows per frame (the frame limit of the projection searches whose output it reads),
 *                       n_levels 1 .. ORBFE_MAX_LEVELS, point records of at least 12 bytes and a multiple of 4 bytes apart
 *                       (orbfe_pose_optimization, orbfe_pose_optimization_batch_device)
 *   new map points      at most 65 535 keypoints per keyframe (orbfe_triangulate_matches*, orbfe_create_new_map_points: the descriptor
 *                       limit of SearchForTriangulation), at most 65 535 pairs per batch launch, n_levels 1 .. ORBFE_MAX_LEVELS
 *                       (pinned by tests/test_mapping_cpu.py)
 *   Sim3 optimisation   at most 9 500 correspondences per problem (orbfe_optimize_sim3, orbfe_optimize_sim3_batch_device: the frame
 *                       limit of the Sim3 search whose matches it reads), at most 65 535 problems per batch launch, th2 > 0
 *                       (pinned by tests/test_optsim3_cpu.py)
 *   PnP solver          at most 1 024 correspondences and 4 096 hypotheses per problem (ORBFE_PNP_MAX_POINTS / _HYPOTHESES, each with
 *                       its reason), minimal sets of four, min_inliers >= 4, at most 65 535 problems per batch launch (orbfe_pnp_solve,
 *                       orbfe_pnp_solve_batch_device; pinned by tests/test_pnp_cpu.py)
 *   local bundle adj.   at most 64 free and 256 keyframes in all, 65 535 points and 262 140 edges per problem, 65 535 problems per
 *                       launch (the ORBFE_LBA_MAX_* constants, each with its reason; pinned by tests/test_lba_cpu.py and
 *                       tests/test_lba_gpu.py)
 *   bundle adjustment   the limits of the local bundle adjustment, and 1 .. 20 iterations (ORBFE_BA_MAX_ITERATIONS, with its reason;
 *                       orbfe_bundle_adjustment, orbfe_bundle_adjustment_batch_device; pinned by tests/test_ba_cpu.py and
 *                       tests/test_ba_gpu.py)
 *   global bundle       ONE map of at most 2 048 keyframes (any number free), 1 048 575 points and 8 388 600 edges, 1 .. 20
 *   adjustment          iterations (the ORBFE_GBA_MAX_* constants, each with its reason; orbfe_global_bundle_adjustment,
 *                       orbfe_global_bundle_adjustment_device; pinned by tests/test_gba_cpu.py and tests/test_gba_gpu.py)
 *   map update behind   at most 65 536 keyframes and as many rows of adjusted poses, 16 777 216 points and as many rows of adjusted
 *   that adjustment     points (the ORBFE_GBA_MAP_MAX_* constants, each with its reason; orbfe_gba_update_map,
 *                       orbfe_gba_update_map_device; pinned by tests/test_gba_map_cpu.py and tests/test_gba_map_gpu.py)
 *   initial map         at most 4 096 keypoints a frame (ORBFE_INIT_MAX_MATCHES) and 65 535 problems per launch, 1 .. 20 iterations,
 *                       q >= 1, min_points >= 0 (orbfe_create_initial_map, orbfe_create_initial_map_batch_device; pinned by
 *                       tests/test_ba_cpu.py and tests/test_ba_gpu.py)
 *   keyframe database   at most 4 096 words per vector, 65 535 queries per call, 4 194 304 adds between two clears, Q x slots and
 *                       Q x cand_cap <= 67 108 864 (the ORBFE_KFDB_* constants, each with its reason; pinned by
 *                       tests/test_kfdb_cpu.py)
 *   map-point refresh   at most 1 024 observations per point, 1 048 576 points, 16 777 216 observations and 1 048 576 keyframes per
 *                       call, n_levels 1 .. ORBFE_MAX_LEVELS (the ORBFE_MP_MAX_* constants, each with its reason; pinned by
 *                       tests/test_mappoint_cpu.py)
 *   covisibility graph  at most 32 768 keyframe rows, 2 048 entries per subject (conn_cap), 65 535 subjects or problems per launch,
 *                       16 777 216 slots and 1 048 576 local keyframes per call, the point and observation limits of the map-point
 *                       refresh (the ORBFE_COV_MAX_* constants, each with its reason; pinned by tests/test_covis_cpu.py)
 *   local map           at most 65 535 frames per launch, kf_cap <= 2 051, p_cap <= 1 048 576, 16 777 216 also-seen indices, the table
 *                       limits of the covisibility graph (the ORBFE_LM_MAX_* constants, each with its reason; pinned by
 *                       tests/test_localmap_cpu.py)
 *   essential graph     at most 32 768 vertices, 262 144 edges and 131 072 envelope blocks per problem, 65 535 problems per launch,
 *                       16 777 216 points per map correction (the ORBFE_EG_MAX_* constants, each with its reason; pinned by
 *                       tests/test_egraph_cpu.py and tests/test_egraph_gpu.py)
 *   essential graph     ONE graph of at most 32 768 vertices, 262 144 edges and 4 194 304 envelope blocks (the ORBFE_EGRID_MAX_*
 *   across the device   constants, each with its reason; orbfe_essential_graph_grid, orbfe_essential_graph_grid_device; pinned by
 *                       tests/test_egraph_grid_cpu.py and tests/test_egraph_grid_gpu.py)
 * Each limit up to the covisibility graph's is pinned at its largest accepted and its first refused value by tests/test_limits_gpu.py (levels: also
 * tests/test_cabi_cpu.py; depth maps: tests/test_frames_cpu.py and tests/test_frames_gpu.py; rectification:
 * tests/test_rectify_cpu.py and tests/test_rectify_gpu.py; pose optimisation: tests/test_pose_cpu.py).
 * Threads: a handle serialises its own calls (internal mutex); different handles may be used from different threads at the same
 * time (Frame.cc:91-94 runs the two extractors on two threads).  The library holds no other mutable global state and reads no
 * environment variables.  The matcher entry points that take no handle (orbfe_search_*, orbfe_stereo_match, orbfe_kf_search,
 * ...) work on a handle the library creates per calling thread -- one HIP stream, scratch HBM and pinned staging that grow to
 * the largest call -- and keeps until the process ends: three for ORB-SLAM2's Tracking / LocalMapping / LoopClosing threads.
 * A thread that is about to end gives its handle back with orbfe_thread_release(). */
int orbfe_thread_release(void);   /* destroys the calling thread's implicit matcher handle, if it has one */

/* ------------------------------------------------------------------------------------- ORBextractor */
/* ORBextractor::ORBextractor (L/src/ORBextractor.cc:407-464).  device < 0 selects the current device. */
int orbfe_extractor_create(const orbfe_params* params, int device, orbfe_extractor** out);
int orbfe_extractor_destroy(orbfe_extractor* e);

/* Getters of L/include/ORBextractor.h:60-74; each writes n_levels floats. */
int orbfe_extractor_levels(const orbfe_extractor* e, int* n_levels);
int orbfe_extractor_scale_factors(const orbfe_extractor* e, float* out);
int orbfe_extractor_inv_scale_factors(const orbfe_extractor* e, float* out);
int orbfe_extractor_sigma2(const orbfe_extractor* e, float* out);
int orbfe_extractor_inv_sigma2(const orbfe_extractor* e, float* out);
int orbfe_extractor_features_per_level(const orbfe_extractor* e, int32_t* out);
/* Upper bound on keypoints per image: sum over levels of max(N_level + 3, 4 * nIni). */
int orbfe_extractor_max_keypoints(const orbfe_extractor* e, int w, int h, int* cap);

/* ORBextractor::operator() (L/src/ORBextractor.cc:978-1039) on ONE host image, synchronous.
 * img: CV_8UC1, h rows of w bytes, `stride` bytes between rows.  kps/desc: caller-owned host buffers of
 * `cap` entries (desc: cap x 32 bytes).  *n_out = number of keypoints.  Keypoints are in level order,
 * inside a level in DistributeOctTree list order, coordinates in level-0 pixels. */
int orbfe_extract(orbfe_extractor* e, const uint8_t* img, int w, int h, int stride, orbfe_keypoint* kps,
                  uint8_t* desc, int cap, int* n_out);

/* mvImagePyramid[level] of the last orbfe_extract call (L/include/ORBextractor.h:76; read by
 * Frame::ComputeStereoMatches, L/src/Frame.cc:483,567-589).  Copies the level (no border) to host. */
int orbfe_pyramid_level(orbfe_extractor* e, int level, uint8_t* dst, int dst_stride, int* w, int* h);
int orbfe_pyramid_level_size(const orbfe_extractor* e, int w0, int h0, int level, int* w, int* h);
/* All levels at once (one device synchronisation): dst[level] receives level `level` with row stride dst_stride[level]. */
int orbfe_pyramid_levels(orbfe_extractor* e, uint8_t* const* dst, const int* dst_stride);

/* Batched operator(): n_images host images of identical geometry, synchronous.  imgs[i] points to image i.
 * kps: n_images x cap, desc: n_images x cap x 32, n_out: n_images. */
int orbfe_extract_batch(orbfe_extractor* e, const uint8_t* const* imgs, int n_images, int w, int h, int stride,
                        orbfe_keypoint* kps, uint8_t* desc, int cap, int32_t* n_out);

/* Device-resident batch: all pointers are DEVICE pointers; asynchronous on `stream` (a hipStream_t, or
 * NULL for the handle's own stream).  d_imgs: image i at d_imgs + i*image_pitch, rows `stride` bytes
 * apart.  d_kps: n_images x cap, d_desc: n_images x cap x 32, d_n_out: n_images int32.  Work space is
 * (re)allocated when the geometry or batch size grows -- call once untimed before timing.
 * Level 0 in place: when d_imgs, stride and image_pitch are multiples of 16 and stride >= w rounded up to 16 (what
 * hipMemcpy2D into a pitched allocation or an image decoder delivers) the images ARE pyramid level 0 -- no copy.  They must
 * then stay unchanged until the results of this batch and every later read of its pyramid (orbfe_stereo_match_device,
 * orbfe_device_pyramid, orbfe_pyramid_level*) are complete.  Other layouts (tightly packed odd-width rows) are copied into
 * pitched planes first. */
int orbfe_extract_batch_device(orbfe_extractor* e, const uint8_t* d_imgs, int n_images, int w, int h, int stride,
                               size_t image_pitch, orbfe_keypoint* d_kps, uint8_t* d_desc, int cap,
                               int32_t* d_n_out, void* stream);
/* Device pointer + geometry of pyramid level `level` of image `image` of the last device batch.  Level 0 is row-major (rows
 * `pitch` bytes apart).  Levels >= 1 are row-major too when a stand-alone resize kernel wrote them, but the fused level chain (the
 * default) stores the levels it writes in TILES of 16 pixels x 8 rows = 128 bytes, tiles in raster order, pitch / 16 tiles per tile
 * row: pixel (x, y) at ((y >> 3) * (pitch >> 4) + (x >> 4)) * 128 + (y & 7) * 16 + (x & 15); orbfe_device_pyramid_layout says which.
 * orbfe_pyramid_level / orbfe_pyramid_levels always deliver row-major host copies. */
int orbfe_device_pyramid(const orbfe_extractor* e, int image, int level, const uint8_t** d_ptr, int* pitch,
                         int* w, int* h);
int orbfe_device_pyramid_layout(const orbfe_extractor* e, int level, int* tiled);   /* *tiled = 1: the 16 x 8 tiles described above */
int orbfe_sync(orbfe_extractor* e);   /* wait for the handle's stream(s) */
/* Waits for the handle's stream and returns ORBFE_ERR_CAPACITY if a kernel of an earlier (asynchronous)
 * batch flagged an internal table overflow; ORBFE_OK otherwise. */
int orbfe_device_status(orbfe_extractor* e);

/* Stage-level outputs of the last batch, for parity tests (host copies; synchronous).
 * candidates: FAST keypoints handed to DistributeOctTree (x, y relative to (16,16), score) in
 * vToDistributeKeys order; blurred: workingMat after GaussianBlur; level_keypoints: octree selection
 * before scaling (x, y in level coords, response). */
int orbfe_debug_candidates(orbfe_extractor* e, int image, int level, int32_t* x, int32_t* y, int32_t* score,
                           int cap, int* n);
int orbfe_debug_blurred(orbfe_extractor* e, int image, int level, uint8_t* dst, int dst_stride);
/* How pyramid and blur run from the next call on: 0 = the fused level chain (default: launch l blurs level l and writes level
 * l + 1 from the same staged windows), 1 = resize chain + the matrix-core blur (v_mfma_i32_16x16x64_i8 band products; DESIGN.md
 * lesson 31), 2 = resize chain + one LDS blur launch over all levels (rounds 1-4).  Same bytes; for parity tests and A/B timing. */
int orbfe_debug_blur_kernel(orbfe_extractor* e, int kind);
int orbfe_debug_pyramid(orbfe_extractor* e, int image, int level, uint8_t* dst, int dst_stride);
int orbfe_debug_level_keypoints(orbfe_extractor* e, int image, int level, int32_t* x, int32_t* y,
                                int32_t* score, int cap, int* n);

/* Per-stage HIP-event timing of the handle's stream.  enable != 0 records events around every kernel
 * stage of subsequent batches; orbfe_stage_times returns the accumulated milliseconds and launch counts
 * since the last reset.  Stage ids: */
enum {
  ORBFE_STAGE_PYRAMID = 0,
  ORBFE_STAGE_FAST = 1,
  ORBFE_STAGE_OCTREE = 2,
  ORBFE_STAGE_BLUR = 3,
  ORBFE_STAGE_DESCRIBE = 4,
  ORBFE_STAGE_COUNT = 5
};
int orbfe_profile_enable(orbfe_extractor* e, int enable);  /* 0 = off, 1 = every stage, otherwise a bit mask: bit (1 + stage) */
int orbfe_stage_times(orbfe_extractor* e, float* ms /*[ORBFE_STAGE_COUNT]*/, int32_t* launches, int reset);
/* The same events as intervals: for every stage launch timed since the last orbfe_stage_times / orbfe_stage_intervals call, its
 * stage index and the milliseconds from ref_event (a hipEvent_t the caller recorded earlier on the same device, timing enabled) to
 * the launch's first and last event.  Two handles that run side by side on two streams (left and right extractor) stretch each
 * other's launches; the union of their intervals is the time the chip spent on that kernel (bench.py's roofline).  The launches
 * also enter the totals of orbfe_stage_times.  At most cap intervals are written, *n receives their number. */
int orbfe_stage_intervals(orbfe_extractor* e, void* ref_event, int32_t* stage, float* start_ms, float* end_ms, int cap, int32_t* n);

/* --------------------------------------------------------------------------------------- ORBmatcher */
/* Work-space handle of the matcher kernels (scratch HBM + a HIP stream).  One handle serves one thread at
 * a time; the host-pointer entry points below that take no handle use a thread-local one, so they may be
 * called concurrently from Tracking / LocalMapping / LoopClosing threads (ORBmatcher objects are
 * stack-constructed per call site in the reference, L/src/Tracking.cc:781,1070). */
typedef struct orbfe_matcher orbfe_matcher;
int orbfe_matcher_create(int device, orbfe_matcher** out);
int orbfe_matcher_destroy(orbfe_matcher* m);
int orbfe_matcher_sync(orbfe_matcher* m);

/* ORBmatcher::DescriptorDistance (L/src/ORBmatcher.cc:1542-1556) for all pairs: dist[i*nB + j] =
 * Hamming(A[i], B[j]) as uint16.  DEVICE pointers (32-byte rows, 16-byte aligned), asynchronous on stream. */
int orbfe_hamming_matrix_device(const uint8_t* d_A, int nA, const uint8_t* d_B, int nB, uint16_t* d_dist,
                                void* stream);

/* Brute-force best / second-best (the inner loops of SearchByBoW, L/src/ORBmatcher.cc:201-222): for
 * every row i of A the first-minimum over j of B (strict <, index order) and the second-smallest
 * distance.  groupA/groupB (nullable, both or neither): compare only where groupA[i] == groupB[j]
 * (vocabulary node id); maskB (nullable): skip j with maskB[j] != 0 (already matched).  n_sets independent
 * problems: set s uses rows [s*strideA, s*strideA + nA[s]) of A and of out, [s*strideB, ..+nB[s]) of B;
 * max_nA >= every nA[s]; nB[s] < 65536.  All pointers DEVICE pointers; asynchronous on stream. */
typedef struct orbfe_bf_match {
  int32_t best_idx;    /* -1 when no candidate */
  int32_t best_dist;   /* 256 when none */
  int32_t second_dist; /* 256 when none */
} orbfe_bf_match;
int orbfe_hamming_bf_device(const uint8_t* d_A, const int32_t* d_nA, int strideA, int max_nA, const uint8_t* d_B,
                            const int32_t* d_nB, int strideB, const int32_t* d_groupA, const int32_t* d_groupB,
                            const uint8_t* d_maskB, int n_sets, orbfe_bf_match* d_out, void* stream);

/* View of the Frame members the projection searches read (L/include/Frame.h): mvKeysUn, mDescriptors,
 * mvuRight and the image bounds; the 64x48 grid (mGrid) is rebuilt on the device from them exactly as
 * Frame::AssignFeaturesToGrid / PosInGrid do (L/src/Frame.cc:250-263,399-410). */
typedef struct orbfe_frame_view {
  int32_t n;                        /* Frame::N */
  const orbfe_keypoint* keys_un;    /* mvKeysUn */
  const uint8_t* desc;              /* mDescriptors (n x 32) */
  const float* u_right;             /* mvuRight, nullable */
  float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY */
} orbfe_frame_view;

/* One projected map point (A11: L/src/ORBmatcher.cc:52-71; A12: :1270-1308); 68 bytes */
typedef struct orbfe_query {
  float u, v;       /* projection */
  float u_r;        /* right-image coordinate of the projection */
  float radius;     /* window half-size, already multiplied by the level scale */
  int32_t min_level, max_level; /* GetFeaturesInArea level filter */
  int32_t valid;    /* 0 = the reference skips this point before the window query */
  int32_t blocks;   /* map point has Observations() > 0 */
  float angle;      /* keypoint angle (rotation histogram of A12) */
  uint8_t desc[32];
} orbfe_query;

typedef struct orbfe_cand {
  int32_t idx;   /* frame keypoint index */
  int32_t dist;  /* Hamming distance to the query descriptor */
} orbfe_cand;

/* Window query + distances, the data-parallel part of every SearchByProjection
 * (Frame::GetFeaturesInArea L/src/Frame.cc:341-397 + DescriptorDistance).  HOST pointers in, HOST
 * results out; synchronous.  For query q writes up to max_cand candidates in the reference's
 * enumeration order to cand[q*max_cand ..] and their total number to n_cand[q] (a count > max_cand
 * signals truncation).  The stereo gate |u_r - mvuRight| <= radius is applied on the device. */
int orbfe_proj_candidates(const orbfe_frame_view* frame, const orbfe_query* q, int nq, orbfe_cand* cand,
                          int32_t* n_cand, int max_cand);

/* SearchByProjection(Frame&, const vector<MapPoint*>&, th) (L/src/ORBmatcher.cc:45-128) on the device:
 * window query + distances in parallel, then the order-dependent assignment by one wave per frame.
 * blocked[idx] != 0 <=> F.mvpMapPoints[idx] has Observations() > 0 on entry (updated in place).
 * assigned[idx] = query index written to F.mvpMapPoints[idx]; entries not written keep their value.
 * *n_matches = return value of the reference.  HOST pointers, synchronous. */
int orbfe_search_by_projection_points(const orbfe_frame_view* frame, const orbfe_query* q, int nq, float nnratio,
                                      uint8_t* blocked, int32_t* assigned, int* n_matches);
/* SearchByProjection(Frame& cur, const Frame& last, th, bMono) (L/src/ORBmatcher.cc:1247-1383).  A slot the rotation check clears
 * (:1372 mvpMapPoints[...] = NULL) leaves with assigned = -1 and blocked = 0, as in the reference's frame. */
int orbfe_search_by_projection_frame(const orbfe_frame_view* cur, const orbfe_query* q, int nq,
                                     int check_orientation, uint8_t* blocked, int32_t* assigned, int* n_matches);

/* SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist)
 * (L/src/ORBmatcher.cc:1385-1504), used by Tracking::Relocalization.  One query per keyframe map point that is not
 * bad and not in sAlreadyFound and that passes the projection / distance checks (:1408-1434): u, v, radius,
 * min_level = nPredictedLevel-1, max_level = nPredictedLevel+1, angle = pKF->mvKeysUn[i].angle, desc, valid = 1,
 * blocks = 1.  blocked[i2] on entry = CurrentFrame.mvpMapPoints[i2] != NULL (:1453).  No stereo gate (u_right of the
 * view is ignored); a match needs bestDist <= max_dist (:1466).  Outputs as orbfe_search_by_projection_frame. */
int orbfe_search_by_projection_keyframe(const orbfe_frame_view* cur, const orbfe_query* q, int nq, int check_orientation,
                                        int max_dist, uint8_t* blocked, int32_t* assigned, int* n_matches);

/* ---- Frame::isInFrustum + Tracking::SearchLocalPoints -------------------------------------------
 * The Frame members Frame::isInFrustum reads (L/src/Frame.cc:284-339). */
typedef struct orbfe_frustum {
  float Rcw[9], tcw[3], Ow[3];        /* mRcw (row-major), mtcw, mOw */
  float fx, fy, cx, cy, mbf;
  float min_x, max_x, min_y, max_y;   /* mnMinX, mnMaxX, mnMinY, mnMaxY */
  float log_scale_factor;             /* mfLogScaleFactor */
  int32_t n_levels;                   /* mnScaleLevels, 1..ORBFE_MAX_LEVELS (ORBFE_ERR_INVALID otherwise) */
  float scale_factors[ORBFE_MAX_LEVELS]; /* mvScaleFactors */
} orbfe_frustum;                      /* 168 bytes */

/* The MapPoint members the path reads (L/include/MapPoint.h); 72 bytes */
typedef struct orbfe_map_point {
  float pos[3], normal[3];            /* GetWorldPos(), GetNormal() */
  float min_distance, max_distance;   /* mfMinDistance, mfMaxDistance (un-scaled; 0.8 / 1.2 are applied as in MapPoint.cc:383-391) */
  int32_t skip;                       /* mnLastFrameSeen == mCurrentFrame.mnId || isBad()  (L/src/Tracking.cc:1057-1060) */
  int32_t observed;                   /* Observations() > 0 */
  uint8_t desc[32];                   /* GetDescriptor() */
} orbfe_map_point;

/* What isInFrustum leaves in the MapPoint (L/src/Frame.cc:329-335); 24 bytes.  in_view != 0 also means
 * pMP->IncreaseVisible() (L/src/Tracking.cc:1063). */
typedef struct orbfe_track {
  int32_t in_view;                    /* mbTrackInView */
  float proj_x, proj_y, proj_xr;      /* mTrackProjX, mTrackProjY, mTrackProjXR */
  int32_t level;                      /* mnTrackScaleLevel */
  float view_cos;                     /* mTrackViewCos */
} orbfe_track;

/* Second half of Tracking::SearchLocalPoints (L/src/Tracking.cc:1050-1078): isInFrustum(pMP, 0.5) for every local map
 * point, then ORBmatcher(nnratio).SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th) (L/src/ORBmatcher.cc:45-128).
 * HOST pointers, synchronous.  track[i] is written for every point; blocked / assigned as in
 * orbfe_search_by_projection_points (assigned[idx] = index into mp[]); *n_to_match = nToMatch. */
int orbfe_search_local_points(const orbfe_frame_view* frame, const orbfe_frustum* frustum, const orbfe_map_point* mp,
                              int n_points, float th, float nnratio, orbfe_track* track, uint8_t* blocked,
                              int32_t* assigned, int* n_to_match, int* n_matches);

/* Batched, device-resident form: frame f owns keypoint rows [f*cap, f*cap + d_n[f]) and map points
 * d_points[f*p_cap .. f*p_cap + d_n_points[f]) with its own d_frustum[f].  The queries never leave HBM.  d_track
 * [n_frames][p_cap], d_blocked [n_frames][cap] (in/out), d_assigned [n_frames][cap] (in/out), d_n_to_match and
 * d_n_matches [n_frames].  Asynchronous on `stream` (NULL = the handle's stream). */
int orbfe_search_local_points_batch_device(orbfe_matcher* m, int n_frames, const orbfe_keypoint* d_kps,
                                           const uint8_t* d_desc, const int32_t* d_n, const float* d_u_right, int cap,
                                           float min_x, float max_x, float min_y, float max_y,
                                           const orbfe_frustum* d_frustum, const orbfe_map_point* d_points,
                                           const int32_t* d_n_points, int p_cap, float th, float nnratio,
                                           orbfe_track* d_track, uint8_t* d_blocked, int32_t* d_assigned,
                                           int32_t* d_n_to_match, int32_t* d_n_matches, void* stream);

/* ---- motion-model tracking on the device: Frame::UnprojectStereo (L/src/Frame.cc:668-679) and the projection part of
 * SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (L/src/ORBmatcher.cc:1257-1308) ------------- */
typedef struct orbfe_unproject_cam {   /* the Frame members UnprojectStereo reads */
  float Rwc[9], Ow[3];                 /* mRwc (row-major), mOw */
  float cx, cy, invfx, invfy;
} orbfe_unproject_cam;                 /* 64 bytes */

typedef struct orbfe_last_point {      /* LastFrame keypoint i with its map point; 60 bytes */
  float pos[3];                        /* pMP->GetWorldPos() */
  int32_t valid;                       /* LastFrame.mvpMapPoints[i] != NULL && !LastFrame.mvbOutlier[i] */
  int32_t observed;                    /* pMP->Observations() > 0 */
  int32_t octave;                      /* LastFrame.mvKeys[i].octave */
  float angle;                         /* LastFrame.mvKeysUn[i].angle */
  uint8_t desc[32];                    /* pMP->GetDescriptor() */
} orbfe_last_point;

typedef struct orbfe_track_pose {      /* CurrentFrame members read by :1257-1308; 160 bytes */
  float Rcw[9], tcw[3];                /* CurrentFrame.mTcw */
  float fx, fy, cx, cy, mbf;
  float min_x, max_x, min_y, max_y;
  int32_t forward, backward;           /* bForward, bBackward (:1267-1268; tlc = Rlw*twc + tlw stays with the caller) */
  float th;
  float scale_factors[ORBFE_MAX_LEVELS]; /* CurrentFrame.mvScaleFactors */
} orbfe_track_pose;

/* One record per keypoint of every frame: map point = UnprojectStereo(i) when d_depth > 0 (valid = 0 otherwise), descriptor /
 * octave / angle of the keypoint itself (a map point created from this frame, L/src/MapPoint.cc:57-86).  DEVICE pointers,
 * asynchronous on `stream`.  d_points [n_frames][cap]. */
int orbfe_unproject_stereo_device(int n_frames, const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
                                  const float* d_depth, int cap, const orbfe_unproject_cam* d_cam, int observed,
                                  orbfe_last_point* d_points, void* stream);
/* Queries of frame f from the points of frame (f - frame_shift) mod n_frames (frame_shift = 1: the previous frame of a
 * sequence batch; 0: the caller arranged the points per frame): projection, invzc / bounds rejects, radius =
 * th * mvScaleFactors[octave], level range by bForward / bBackward, u_r = u - mbf * invzc.  d_nq[f] receives the point
 * count of the source frame.  Feed the result to orbfe_proj_match_batch_device(mode 1). */
int orbfe_track_queries_device(int n_frames, const orbfe_track_pose* d_pose, const orbfe_last_point* d_points,
                               const int32_t* d_n_points, int p_cap, int frame_shift, orbfe_query* d_queries,
                               int32_t* d_nq, void* stream);

/* The two calls above in one pass, for callers that need the stereo points only as the next frame's search queries (a tracking
 * loop that creates its temporal points from the stereo depth, L/src/Tracking.cc:877-936 UpdateLastFrame, then runs
 * SearchByProjection(cur, last)): queries of frame f from the KEYPOINTS of frame f - frame_shift -- UnprojectStereo with that frame's
 * camera (L/src/Frame.cc:668-679), then the projection with frame f's pose (L/src/ORBmatcher.cc:1270-1308) -- without the 60-byte
 * point record per keypoint going through memory.  Byte-equal to orbfe_unproject_stereo_device + orbfe_track_queries_device.
 * Frames in front of the batch (f < frame_shift): the carry frame when the five d_carry_* arrays are given (one frame: [cap]
 * keypoints / descriptors / depth, one count, one camera -- the last frame of the batch before), otherwise the batch's own tail
 * (index mod n_frames, as orbfe_track_queries_device).  The carry holds one frame, so it takes frame_shift 0 or 1 only: a carry
 * with frame_shift > 1 is ORBFE_ERR_INVALID.  d_nq[f] = keypoint count of the source frame. */
int orbfe_track_queries_stereo_device(int n_frames, const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
                                      const float* d_depth, int cap, const orbfe_unproject_cam* d_cam, int observed,
                                      const orbfe_keypoint* d_carry_kps, const uint8_t* d_carry_desc, const int32_t* d_carry_n,
                                      const float* d_carry_depth, const orbfe_unproject_cam* d_carry_cam,
                                      const orbfe_track_pose* d_pose, int frame_shift, orbfe_query* d_queries, int32_t* d_nq,
                                      void* stream);

/* ---- lens distortion, image bounds and RGB-D depth: the per-keypoint tail of Frame::Frame ------------------------------------
 * Monocular (L/src/Frame.cc:216) and RGB-D (:157-159) frames: UndistortKeyPoints (:419-445, cv::undistortPoints with the default five
 * iterations, R = I, P = K, in double), ComputeImageBounds (:447-476) and ComputeStereoFromRGBD (:648-666) on the depth map as
 * Tracking::GrabImageRGBD scales it (L/src/Tracking.cc:210-211).  k1 == 0 means no undistortion at all (mvKeysUn = mvKeys, bounds
 * (0, cols, 0, rows)), whatever k2 .. k3 hold (:420-423, :469-474).
 * Bounds: the four floats of orbfe_image_bounds are mnMinX .. mnMaxY -- they go into EVERY min_x ... max_y the library takes
 * (orbfe_frame_view, orbfe_proj_match_batch_device, orbfe_search_local_points_batch_device, orbfe_track_pose, orbfe_frustum,
 * orbfe_kf_camera) for frames of that camera; with distortion they are not (0, w, 0, h), and undistorted keypoints may lie outside
 * them (the grid then leaves them out, Frame::PosInGrid :399-410).
 * The RGB-D motion-model step reuses two entry points unchanged: orbfe_track_queries_stereo_device fed keys_un and the depth out of
 * orbfe_undistort_frames_device (UnprojectStereo reads mvKeysUn, :668-679; octave and angle are those of mvKeys), its
 * orbfe_track_pose records with the undistorted bounds and th = 15 (L/src/Tracking.cc:793-798); then orbfe_proj_match_batch_device
 * (mode 1) fed keys_un, u_right and the undistorted bounds. */
typedef struct orbfe_calibration {
  float fx, fy, cx, cy;          /* mK */
  float k1, k2, p1, p2, k3;      /* mDistCoef; k3 = 0 when the settings file has none (L/src/Tracking.cc:67-77) */
  float mbf;                     /* Camera.bf */
  float depth_factor;            /* mDepthMapFactor: 1.0f / DepthMapFactor, or 1 when |DepthMapFactor| < 1e-5 (L/src/Tracking.cc:141-147) */
  int32_t reserved;              /* 0 */
} orbfe_calibration;             /* 48 bytes */

/* ComputeImageBounds (L/src/Frame.cc:447-476) of a width x height image: undistorts the float corners (0,0), (cols,0), (0,rows),
 * (cols,rows); min_x = min(c0.x, c2.x), max_x = max(c1.x, c3.x), min_y = min(c0.y, c1.y), max_y = max(c2.y, c3.y).  HOST,
 * synchronous, needs no device.  width / height 1 .. 4095, fx and fy != 0. */
int orbfe_image_bounds(const orbfe_calibration* cal, int width, int height, float* min_x, float* max_x, float* min_y, float* max_y);
/* cv::undistortPoints as Frame calls it, for n host points (x, y interleaved); xy_un may equal xy.  HOST, synchronous: a
 * calibration-time utility (bounds, a handful of points), not a fallback of the device entry below.  The same arithmetic, bit for bit. */
int orbfe_undistort_points(const orbfe_calibration* cal, const float* xy, int n, float* xy_un);

#define ORBFE_DEPTH_NONE 0   /* monocular Frame: keys_un only (d_u_right / d_depth_out / d_n_depth optional: -1, -1, 0, :219-220) */
#define ORBFE_DEPTH_U16 1    /* raw sensor map, e.g. TUM depth PNGs: mvDepth = (float)raw * depth_factor */
#define ORBFE_DEPTH_F32 2    /* float map: scaled by depth_factor only when fabsf(depth_factor - 1.0f) > 1e-5 */
/* The per-keypoint tail of Frame::Frame for n_frames frames in one launch.  DEVICE pointers, asynchronous on `stream` (NULL: the
 * NULL stream).  Frame f: keypoint rows [f*cap, f*cap + d_n[f]) of d_kps (mvKeys) -> the same rows of d_kps_un (mvKeysUn: pt
 * undistorted, size / angle / response / octave / class_id copied), d_u_right (mvuRight) and d_depth_out (mvDepth);
 * d_n_depth[f] = keypoints with depth (d > 0).  Frame f's depth map is at d_depth + f*depth_image_bytes, width x height samples
 * (uint16 or float), rows depth_pitch bytes apart; ComputeStereoFromRGBD reads the sample at the TRUNCATED coordinates of the
 * distorted keypoint, imDepth.at<float>((int)y, (int)x).  A keypoint whose truncated coordinates fall outside the map gets no depth
 * (-1, -1) and nothing outside the map is read; the extractor never produces one.  d_kps_un may equal d_kps (in place).  Rows at and
 * behind d_n[f] are not written; d_n[f] is clamped to [0, cap].
 * Limits (ORBFE_ERR_INVALID): n_frames >= 0 (0: nothing is launched), cap >= 1, fx and fy != 0, a known depth_format; with depth:
 * width / height 1 .. 4095, depth_pitch >= width samples, depth_image_bytes >= (height - 1) * depth_pitch + width samples, the map
 * pointer, pitch and image stride multiples of the sample size.  Without a device: ORBFE_ERR_NO_DEVICE (there is no CPU path). */
int orbfe_undistort_frames_device(int n_frames, const orbfe_keypoint* d_kps, const int32_t* d_n, int cap,
                                  const orbfe_calibration* cal, int depth_format, const void* d_depth, int width, int height,
                                  int depth_pitch, size_t depth_image_bytes, orbfe_keypoint* d_kps_un, float* d_u_right,
                                  float* d_depth_out, int32_t* d_n_depth, void* stream);

/* ---- stereo rectification: cv::initUndistortRectifyMap + cv::remap of the EuRoC stereo driver ---------------------------------
 * Source/Examples/Stereo/stereo_euroc.cc reads LEFT. / RIGHT. K, D, R, P from the settings file, builds two float maps per eye with
 * cv::initUndistortRectifyMap(K, D, R, P(0:3, 0:3), size, CV_32F) (:108-111) and runs cv::remap(..., cv::INTER_LINEAR) on both images
 * of every frame (:159-160) before TrackStereo; Frame::ComputeStereoMatches is only valid on such pairs.  A rectifier is that pair of
 * maps for one camera, built once; orbfe_rectify_batch_device is the remap of a batch of images in HBM (csrc/rectify_kernels.hip).
 * No OpenCV exists where this library is built and tested: the arithmetic below is this project's reading of OpenCV 4.5's scalar
 * paths, as unpinned as the other OpenCV primitives.
 * Maps (host, double, once per camera): A = P(0:3, 0:3) x R, each element summed over k = 0, 1, 2; ir = adjugate(A) x (1.0 / det),
 * det expanded along the first row (det == 0: ORBFE_ERR_INVALID).  Row i starts with _x = i*ir[1] + ir[2], _y = i*ir[4] + ir[5],
 * _w = i*ir[7] + ir[8]; column j: w = 1./_w, x = _x*w, y = _y*w, x2 = x*x, y2 = y*y, r2 = x2 + y2, _2xy = 2*x*y,
 * kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2, xd = x*kr + p1*_2xy + p2*(r2 + 2*x2), yd = y*kr + p1*(r2 + 2*y2) + p2*_2xy,
 * map_x = (float)(fx*xd + u0), map_y = (float)(fy*yd + v0), then _x += ir[0], _y += ir[3], _w += ir[6] (running sums).
 * D holds k1 k2 p1 p2 k3; more coefficients cannot be expressed and a skew K[0][1] != 0 is refused.
 * Pixels (8-bit, one channel, INTER_LINEAR, BORDER_CONSTANT 0): sx = rint(map_x * 32.0f) (float product, half to even), X = sx >> 5,
 * ax = sx & 31, likewise sy, Y, ay; a product that is not finite or not an int32 puts the pixel outside.  Taps (Y, X) (Y, X+1)
 * (Y+1, X) (Y+1, X+1) with the weights (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax ay; a tap outside the source reads 0;
 * out = (sum + 512) >> 10 -- OpenCV's 15-bit weight table is exactly 32 x these products, so this equals its (sum + 16384) >> 15. */
typedef struct orbfe_rectify_camera {
  double K[9], D[5], R[9], P[12];          /* row-major, as the settings file holds them */
  int32_t src_width, src_height;           /* the raw image */
  int32_t dst_width, dst_height;           /* the map / the rectified image (the reference uses the same size) */
} orbfe_rectify_camera;
typedef struct orbfe_rectifier orbfe_rectifier;
/* device >= 0: the fixed-point map is uploaded to that device (orbfe_rectify_batch_device); device = -1: a host-only handle for
 * orbfe_rectifier_maps / _coverage / orbfe_rectify_image, which needs no GPU.  Sizes 1 .. 4095 per side. */
int orbfe_rectifier_create(const orbfe_rectify_camera* cam, int device, orbfe_rectifier** out);
int orbfe_rectifier_destroy(orbfe_rectifier* r);
int orbfe_rectifier_info(const orbfe_rectifier* r, orbfe_rectify_camera* cam, int* device);   /* either output may be NULL */
/* The float maps, dst_height x dst_width each, to HOST buffers */
int orbfe_rectifier_maps(const orbfe_rectifier* r, float* map_x, float* map_y);
/* Destination pixels by class: inner = all four taps inside the source; outside = no tap inside (the pixel is 0); edge = the rest */
int orbfe_rectifier_coverage(const orbfe_rectifier* r, int32_t* inner, int32_t* edge, int32_t* outside);
/* cv::remap of ONE host image (src_height rows of src_width bytes, src_stride apart -> dst_height x dst_width, dst_stride apart).
 * HOST, synchronous: a calibration-time and test utility, not a fallback of the device entry below.  The same arithmetic, byte for
 * byte.  Strides at least the widths. */
int orbfe_rectify_image(const orbfe_rectifier* r, const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride);
/* cv::remap of n_images images in one launch.  DEVICE pointers on the rectifier's device (the caller's current device),
 * asynchronous on `stream` (NULL: the NULL stream).  Image f is read at d_src + f*src_image_bytes (rows src_pitch apart) and written
 * at d_dst + f*dst_image_bytes (rows dst_pitch apart).  Nothing outside src_width x src_height of an image is read; only dst_width
 * bytes of each destination row are written (padding stays untouched).  Any alignment; a destination whose pointer, pitch and image
 * stride are multiples of 4 is written in dwords.
 * Limits (ORBFE_ERR_INVALID): n_images >= 0 (0: nothing is launched), each pitch >= its width, each image stride >=
 * (height - 1) * pitch + width, source and destination must not overlap.  A host-only rectifier: ORBFE_ERR_NO_DEVICE. */
int orbfe_rectify_batch_device(orbfe_rectifier* r, const uint8_t* d_src, int n_images, int src_pitch, size_t src_image_bytes,
                               uint8_t* d_dst, int dst_pitch, size_t dst_image_bytes, void* stream);

/* ---- Optimizer::PoseOptimization (L/src/Optimizer.cc:233-435) on the device ----------------------------------------------------
 * What every tracked frame runs after its projection search (Tracking::TrackWithMotionModel L/src/Tracking.cc:798-830,
 * TrackLocalMap :845-866, TrackReferenceKeyFrame, Relocalization): one 6-DoF vertex, one unary edge per keypoint with a map point --
 * monocular when mvuRight[i] < 0 (2-D error, Huber delta (float)sqrt(5.991), chi2 bound (float)5.991), stereo otherwise (3-D error,
 * (float)sqrt(7.815), (float)7.815), information mvInvLevelSigma2[octave] x I -- four rounds of g2o's Levenberg optimize(10), each
 * from the input pose, edges re-classified after every round, the robust kernels removed after the third, one round only with fewer
 * than 10 edges, nothing at all with fewer than 3.  csrc/pose_internal.h states the arithmetic (all double) line by line; neither
 * Eigen nor g2o exists where this library is built and tested, so it is this project's reading of their source, unpinned (DESIGN
 * section 2), checked against an independent numpy reading (tests/np_pose.py) to one float ulp of the pose and equal flags.
 * One deliberate deviation: after a round every edge is classified by its chi2 at that round's final pose; the reference reads, for
 * an edge that was active, the error of the last Levenberg trial even when that trial was rejected (a difference near 1e-10).
 * Deterministic: a frame's result does not depend on the run, on its position in the batch or on the batch size. */
typedef struct orbfe_pose_camera {       /* what the edges read of the Frame */
  float fx, fy, cx, cy, mbf;
  int32_t n_levels;                      /* 1 .. ORBFE_MAX_LEVELS */
  float inv_level_sigma2[ORBFE_MAX_LEVELS]; /* mvInvLevelSigma2 */
} orbfe_pose_camera;                     /* 88 bytes */
typedef struct orbfe_pose_result {
  float Tcw[12];                         /* rows of [R | t] after SetPose; the input pose when n_initial < 3 */
  int32_t n_initial, n_bad, n_inliers;   /* nInitialCorrespondences, nBad, the return value */
  int32_t rounds, iterations;            /* rounds run (1 or 4; 0 when n_initial < 3), Levenberg iterations over all rounds */
} orbfe_pose_result;                     /* 68 bytes */
#define ORBFE_POSE_DISCARD 1   /* also Tracking.cc:815-826: assigned[idx] = -1 and outlier[idx] = 0 for every outlier */
/* One frame, the per-frame call of Tracking.  HOST pointers, synchronous, on the calling thread's current device; runs the kernel
 * of the batch form (no CPU fallback: ORBFE_ERR_NO_DEVICE without a device).  frame: n, keys_un and u_right (NULL: every edge is
 * monocular) are read, desc is not.  assigned[idx] >= 0 <=> mvpMapPoints[idx] != NULL, its value an index into the n_points records
 * at `points`, point_stride bytes apart, whose first three floats are GetWorldPos() (orbfe_map_point: 72, orbfe_last_point: 60, or
 * bare positions: 12).  Tcw_in: 12 floats, the rows of [R | t] of mTcw.  outlier[idx] (mvbOutlier) is written for every idx < n:
 * 0 where there is no point (the reference leaves those entries untouched).
 * A row whose assigned value is >= n_points or whose octave is outside [0, n_levels) is no edge: nothing is read for it and it is
 * counted nowhere.  z == 0 of a point in the camera frame is not specified.
 * Limits (ORBFE_ERR_INVALID): 0 <= n <= 9 500 (the frame limit of the projection searches), n_points >= 0, n_levels 1 ..
 * ORBFE_MAX_LEVELS, point_stride >= 12 and a multiple of 4, no null pointer except u_right (and keys_un / assigned / points /
 * outlier when their count is 0). */
int orbfe_pose_optimization(const orbfe_frame_view* frame, const int32_t* assigned, const void* points, int point_stride,
                            int n_points, const orbfe_pose_camera* camera, const float* Tcw_in, orbfe_pose_result* result,
                            uint8_t* outlier);
/* n_frames frames in one launch, one workgroup per frame.  DEVICE pointers, asynchronous on `stream` (NULL: the NULL stream).
 * Frame f owns keypoint rows [f*cap, f*cap + d_n[f]) of d_keys_un / d_u_right (nullable: all monocular) / d_assigned / d_outlier;
 * assigned values index the point records of frame (f - frame_shift) mod n_frames, d_points + that frame * p_cap * point_stride,
 * of which d_n_points[that frame] exist -- the convention of orbfe_track_queries_device, so the d_assigned of
 * orbfe_proj_match_batch_device (mode 0 and 1) and of orbfe_search_local_points_batch_device feeds this call unchanged.  d_camera:
 * ONE record for the batch; d_Tcw_in [n_frames][12]; d_result [n_frames]; d_outlier [n_frames][cap].  d_n[f] is clamped to
 * [0, cap], d_n_points to [0, p_cap]; rows at and behind d_n[f] are neither read nor written.
 * flags: 0 or ORBFE_POSE_DISCARD (d_assigned is written only then; the counts in d_result are those before the discard).
 * Limits (ORBFE_ERR_INVALID): n_frames >= 0 (0: nothing is launched), 1 <= cap <= 9 500, p_cap >= 1, frame_shift >= 0,
 * point_stride >= 12 and a multiple of 4, unknown flag bits, null pointers other than d_u_right, records not 4-byte aligned.
 * n_levels lives in device memory and is not validated here: the kernel clamps nothing but treats an octave outside
 * [0, min(n_levels, ORBFE_MAX_LEVELS)) as no edge. */
int orbfe_pose_optimization_batch_device(int n_frames, const orbfe_keypoint* d_keys_un, const float* d_u_right, const int32_t* d_n,
                                         int cap, int32_t* d_assigned, const void* d_points, int point_stride,
                                         const int32_t* d_n_points, int p_cap, int frame_shift, const orbfe_pose_camera* d_camera,
                                         const float* d_Tcw_in, orbfe_pose_result* d_result, uint8_t* d_outlier, int flags,
                                         void* stream);

/* SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (L/src/ORBmatcher.cc:161-273), entirely on the device.
 * A DBoW2::FeatureVector is passed as its nodes sorted by id, each {node_id, start, count} into an index array
 * (nodesA/idxA = pKF->mFeatVec, nodesB/idxB = F.mFeatVec).  validA[i] != 0 <=> keyframe feature i has a map point
 * that is not bad.  matchB[j] = keyframe feature matched to frame feature j (the caller stores
 * vpMapPointsKF[matchB[j]] in vpMapPointMatches[j]) or -1; *n_matches = the reference's return value.
 * HOST pointers, synchronous. */
typedef struct orbfe_featvec_node { int32_t node_id, start, count; } orbfe_featvec_node;
int orbfe_search_by_bow(const uint8_t* descA, const float* angleA, const uint8_t* validA, int nA,
                        const orbfe_featvec_node* nodesA, int n_nodesA, const int32_t* idxA, const uint8_t* descB,
                        const float* angleB, int nB, const orbfe_featvec_node* nodesB, int n_nodesB,
                        const int32_t* idxB, float nnratio, int check_orientation, int32_t* matchB, int* n_matches);

/* SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (L/src/ORBmatcher.cc:494-612): both sides carry a validity mask
 * (map point present and not bad), the acceptance is bestDist < TH_LOW (strict), and the result is per feature of the
 * first keyframe: matchA[i] = index in the second keyframe (the caller stores vpMapPoints2[matchA[i]]) or -1. */
int orbfe_search_by_bow_kf(const uint8_t* descA, const float* angleA, const uint8_t* validA, int nA,
                           const orbfe_featvec_node* nodesA, int n_nodesA, const int32_t* idxA, const uint8_t* descB,
                           const float* angleB, const uint8_t* validB, int nB, const orbfe_featvec_node* nodesB,
                           int n_nodesB, const int32_t* idxB, float nnratio, int check_orientation, int32_t* matchA,
                           int* n_matches);

/* The candidate loop of the searches in which no query blocks another -- Fuse (L/src/ORBmatcher.cc:818-868), Fuse with Sim3
 * (:983-1009), SearchBySim3 (both directions, :1118-1147, 1194-1223): for every query the FIRST minimum-distance keypoint
 * of KeyFrame::GetFeaturesInArea(u, v, radius) (L/src/KeyFrame.cc:526-567) whose octave lies in [min_level, max_level]
 * (nPredictedLevel-1 .. nPredictedLevel).  gate: ORBFE_GATE_NONE, or ORBFE_GATE_FUSE_CHI2 = Fuse's reprojection test with
 * u_r = the projected right coordinate and inv_level_sigma2 = mvInvLevelSigma2, n_levels (<= ORBFE_MAX_LEVELS) floats
 * (e2 * invSigma2 > 7.8 stereo / 5.99 mono).
 * best_idx[q] = keypoint index or -1, best_dist[q] = its distance (256 if none): the caller applies TH_LOW / TH_HIGH and
 * the map bookkeeping (Replace / AddObservation / the mutual check) in query order.  HOST pointers, synchronous. */
enum { ORBFE_GATE_NONE = 1, ORBFE_GATE_FUSE_CHI2 = 2 };
int orbfe_proj_best(const orbfe_frame_view* keyframe, const orbfe_query* q, int nq, int gate, const float* inv_level_sigma2,
                    int n_levels, int32_t* best_idx, int32_t* best_dist);

/* ---- whole-function projection searches of the keyframe-rate callers ---------------------------------
 * Fuse (L/src/ORBmatcher.cc:766-907), Fuse with Sim3 (:909-1027), SearchBySim3 (:1029-1245, one direction per call),
 * SearchByProjection(KeyFrame*, Scw, ...) (:275-386) and SearchByProjection(Frame&, KeyFrame*, set, th, ORBdist)
 * (:1385-1504) share one shape: project every candidate map point into a camera, gate it (depth, image bounds, distance
 * range, viewing angle), predict its pyramid level, query the window and take the best descriptor.  orbfe_kf_search runs
 * all of that on the device; what stays with the caller is the pose algebra in front (decomposing Scw, composing
 * sR21 / t21: a handful of 3x3 products) and the map bookkeeping behind (Replace / AddObservation / AddMapPoint,
 * vpReplacePoint, the mutual check), which must replay in point order on the SLAM objects. */
enum {
  ORBFE_KF_FUSE = 1,       /* :766-907   float 1/z, KeyFrame::IsInImage, normal gate, chi-square gate, <= TH_LOW is the caller's */
  ORBFE_KF_FUSE_SIM3 = 2,  /* :909-1027  double 1.0/z, IsInImage, normal gate, no chi-square gate */
  ORBFE_KF_SIM3 = 3,       /* :1029-1245 second transform (sR21, t21), dist3D = |p3Dc2|, no normal gate */
  ORBFE_KF_LOOP = 4,       /* :275-386   float 1/z, IsInImage, normal gate; vpMatched blocks (sequential), accept <= max_dist */
  ORBFE_KF_RELOC = 5       /* :1385-1504 no depth gate, double 1.0/z, (fx*xc)*invzc, Frame bounds (< min || > max), levels
                              [l-1, l+1], occupied keypoints block, accept <= max_dist, rotation histogram */
};
typedef struct orbfe_kf_camera {
  float R[9], t[3];         /* p1 = R * p3Dw + t   (Rcw, tcw; SearchBySim3: R1w, t1w) */
  float R2[9], t2[3];       /* ORBFE_KF_SIM3 only: p2 = R2 * p1 + t2   (sR21, t21) */
  float Ow[3];              /* camera centre: dist3D = |p3Dw - Ow| (unused by ORBFE_KF_SIM3) */
  float fx, fy, cx, cy, mbf;
  float min_x, max_x, min_y, max_y;   /* mnMinX .. mnMaxY of the keyframe / frame searched in */
  float log_scale_factor;             /* mfLogScaleFactor */
  int32_t n_levels;                   /* mnScaleLevels, 1..ORBFE_MAX_LEVELS */
  float th;                           /* radius = th * mvScaleFactors[nPredictedLevel] */
  float scale_factors[ORBFE_MAX_LEVELS];
} orbfe_kf_camera;                    /* 220 bytes */
typedef struct orbfe_kf_point {       /* one candidate map point; 72 bytes */
  float pos[3], normal[3];            /* GetWorldPos(), GetNormal() */
  float min_distance, max_distance;   /* mfMinDistance, mfMaxDistance (un-scaled, see orbfe_map_point) */
  int32_t skip;                       /* the reference `continue`s before projecting (NULL, isBad(), already found ...) */
  float angle;                        /* ORBFE_KF_RELOC: pKF->mvKeysUn[i].angle for the rotation histogram */
  uint8_t desc[32];                   /* GetDescriptor() */
} orbfe_kf_point;
typedef struct orbfe_kf_result {      /* 24 bytes */
  int32_t best_idx;                   /* keypoint of the first minimum distance among the gated candidates, -1 = none.
                                         ORBFE_KF_LOOP / RELOC: the keypoint this point was ASSIGNED to (-1 = none / removed) */
  int32_t best_dist;                  /* its distance (256 = none); LOOP / RELOC: unspecified */
  int32_t level;                      /* nPredictedLevel, -1 when a gate rejected the point */
  float u, v, u_r;                    /* the projection (u_r = u - mbf * invz) */
} orbfe_kf_result;
/* keyframe = mvKeysUn / mDescriptors / mvuRight / bounds of the KeyFrame (Frame for ORBFE_KF_RELOC) searched in;
 * inv_level_sigma2 = mvInvLevelSigma2 (ORBFE_KF_FUSE, n_levels floats, else NULL).  blocked (LOOP: vpMatched[idx] != NULL;
 * RELOC: CurrentFrame.mvpMapPoints[idx] != NULL) is read and updated, NULL for the other modes.  check_orientation and
 * max_dist (TH_LOW / ORBdist) apply to LOOP / RELOC.  *n_matches: LOOP / RELOC = the reference's return value, otherwise the
 * number of points with a candidate.  HOST pointers, synchronous. */
int orbfe_kf_search(const orbfe_frame_view* keyframe, const float* inv_level_sigma2, const orbfe_kf_camera* cam,
                    const orbfe_kf_point* points, int n_points, int mode, int check_orientation, int max_dist,
                    uint8_t* blocked, orbfe_kf_result* results, int* n_matches);

/* ---- all Fuse calls of LocalMapping::SearchInNeighbors in one batch (L/src/LocalMapping.cc:425-509) --------------------------
 * A fuse batch keeps K target keyframes in HBM with their grids built once, and one table of candidate map points that persists
 * between calls.  Row (k, i) -- point i searched in target k -- is, all 24 bytes, what orbfe_kf_search(targets[k], target k's
 * 1 / sigma2 table, cams[k], point i, mode) returns, whatever K is, wherever the row stands in the batch and whether a full or a
 * partial search computed it; a row skipped by the mask or by the point's own `skip` holds what that call writes for a skipped
 * point (-1, 256, -1, 0, 0, 0).  The K calls of the reference depend on each other only through the map: MapPoint::Replace can
 * change the surviving point's descriptor (ComputeDistinctiveDescriptors), so the caller searches everything once, replays the
 * targets in order on its map and, before it enters target k + 1, searches again the points whose descriptor changed, in the
 * targets from k + 1 on (the partial search below).  mode: ORBFE_KF_FUSE or ORBFE_KF_FUSE_SIM3.
 * Limits (ORBFE_ERR_INVALID, checked before a device is looked for): K >= 0 and n_points >= 0 (0 launches nothing), at most 65 535
 * keypoints per target, K x n_points within
 * int32_t, n_levels 1 .. ORBFE_MAX_LEVELS per target, point_idx strictly ascending and within the table, first_target 0 .. K, no
 * null pointer where a count is positive.  No CPU fallback (ORBFE_ERR_NO_DEVICE).  Pinned by tests/test_neighbors_cpu.py and
 * tests/test_neighbors_gpu.py. */
typedef struct orbfe_fuse_batch orbfe_fuse_batch;
/* targets[k]: mvKeysUn, mDescriptors, mvuRight (or NULL) and the bounds of target k; cams[k] its camera; inv_level_sigma2 + k *
 * ORBFE_MAX_LEVELS: its own mvInvLevelSigma2, cams[k].n_levels floats read (ORBFE_KF_FUSE; may be NULL for ORBFE_KF_FUSE_SIM3).
 * Everything is copied: one packed upload, one grid-build launch for all K (targets whose image bounds differ -- several cameras --
 * get a launch each: the grid geometry is a launch constant).  HOST pointers, synchronous. */
int orbfe_fuse_batch_create(int K, const orbfe_frame_view* targets, const orbfe_kf_camera* cams, const float* inv_level_sigma2,
                            int mode, orbfe_fuse_batch** out);
/* The same with the arrays already in HBM, target k at offset k * cap (keypoints, descriptors x 32, u_right; d_u_right may be NULL,
 * a keypoint without a right coordinate holds a negative value), d_n[k] <= cap keypoints each, 1 <= cap <= 65 535.  The arrays are
 * BORROWED: they stay the caller's and must outlive the handle unchanged.  The grids are built on `stream` (NULL: the handle's own);
 * searches on another stream are the caller's to order behind it. */
int orbfe_fuse_batch_create_device(int K, const orbfe_keypoint* d_keys, const uint8_t* d_desc, const float* d_u_right, const int32_t* d_n,
                                   int cap, float min_x, float max_x, float min_y, float max_y, const orbfe_kf_camera* d_cams,
                                   const float* d_inv_level_sigma2, int mode, void* stream, orbfe_fuse_batch** out);
/* A batch lives for one keyframe: a destroyed handle leaves its stream, device blocks and pinned mirrors to the next handle the
 * calling thread creates (allocating them costs more than the searches); orbfe_thread_release() frees what is left, and a thread
 * that ends without calling it keeps them until the process ends, as it keeps its implicit matcher handle.  Destroy waits for the
 * handle's own stream and for the work it enqueued on the caller's streams (an event behind each), not for the rest of the device, so
 * the blocks change hands idle.  A handle serialises its own calls (internal mutex). */
int orbfe_fuse_batch_destroy(orbfe_fuse_batch* b);
/* point_idx == NULL: `points` (n_points records) REPLACES the resident table and every row (k >= first_target, i) is searched;
 * n_idx is ignored.  point_idx != NULL (n_idx entries, strictly ascending, n_points = the resident table's size): points[j] replaces
 * record point_idx[j] and only the rows (k >= first_target, i in point_idx) are searched.  skip: NULL, or K x n_points bytes, non-zero
 * = the row is known to be skipped (NULL, bad, already in that keyframe); it only saves work.  results: K x n_points, row (k, i) at
 * k * n_points + i; only searched rows are written, every other byte is left as it was.  HOST pointers, synchronous. */
int orbfe_fuse_batch_search(orbfe_fuse_batch* b, const orbfe_kf_point* points, int n_points, const int32_t* point_idx, int n_idx,
                            int first_target, const uint8_t* skip, orbfe_kf_result* results);
/* The same with the records, the index list, the mask and the results in HBM, asynchronous on `stream` (NULL: the handle's own); the
 * host form makes the same launches between its packed upload and download.  An index outside the table, which only the host form
 * can refuse, is dropped. */
int orbfe_fuse_batch_search_device(orbfe_fuse_batch* b, const orbfe_kf_point* d_points, int n_points, const int32_t* d_point_idx,
                                   int n_idx, int first_target, const uint8_t* d_skip, orbfe_kf_result* d_results, void* stream);

/* SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vMatchedPairs, bOnlyStereo) (L/src/ORBmatcher.cc:614-764)
 * with CheckDistEpipolarLine (:137-159).  The epipole (:622-630) is computed by the caller. */
typedef struct orbfe_epipolar {
  float F12[9];               /* row-major */
  float ex, ey;               /* epipole of pKF1's camera centre in pKF2's image */
  float scale_factors[ORBFE_MAX_LEVELS];  /* pKF2->mvScaleFactors */
  float level_sigma2[ORBFE_MAX_LEVELS];   /* pKF2->mvLevelSigma2 */
} orbfe_epipolar;             /* 172 bytes */
/* keys = mvKeysUn, u_right = mvuRight (NULL = monocular: all -1), has_mp[i] = (GetMapPoint(i) != NULL); FeatureVectors as in
 * orbfe_search_by_bow.  matchA[i] = index in pKF2 matched to feature i of pKF1, or -1 (vMatchedPairs = the pairs
 * (i, matchA[i]) in ascending i).  No match blocks another (vbMatched2 is never set in the reference); among the
 * candidates that pass the gates the smallest distance wins, the LAST one on ties (`dist > bestDist` rejects, :691). */
int orbfe_search_for_triangulation(const orbfe_keypoint* keysA, const uint8_t* descA, const float* u_rightA,
                                   const uint8_t* has_mpA, int nA, const orbfe_featvec_node* nodesA, int n_nodesA,
                                   const int32_t* idxA, const orbfe_keypoint* keysB, const uint8_t* descB,
                                   const float* u_rightB, const uint8_t* has_mpB, int nB, const orbfe_featvec_node* nodesB,
                                   int n_nodesB, const int32_t* idxB, const orbfe_epipolar* ep, int only_stereo,
                                   int check_orientation, int32_t* matchA, int* n_matches);

/* ---- LocalMapping::CreateNewMapPoints (L/src/LocalMapping.cc:185-423) -----------------------------------------------------------
 * The loop body behind SearchForTriangulation, per match (idx1, idx2) of a (pKF1, pKF2) pair (:261-402): parallax of the two rays,
 * stereo parallax, the choice between linear triangulation / UnprojectStereo(idx1) / UnprojectStereo(idx2) / reject, and the gates
 * in the reference's order and precision.  For an accepted pair the record also holds what MapPoint::UpdateNormalAndDepth
 * (L/src/MapPoint.cc:340-381) yields for the new point with exactly these two observations and pKF1 as reference keyframe, so it
 * fills an orbfe_map_point / orbfe_kf_point directly.  What stays with the caller is what the reference interleaves: new MapPoint,
 * AddObservation, AddMapPoint, ComputeDistinctiveDescriptors, mlpRecentAddedMapPoints.
 * csrc/mapping_internal.h states the arithmetic once (cv::Mat expressions as frustum_kernels.hip reads them, `cos` / `atan2` the
 * float overloads).  The 4x4 decomposition of the linear path is this project's own one-sided Jacobi in double on the float matrix
 * (cv::SVD is not available where this library is built); UnprojectStereo reads the UNDISTORTED keypoint
 * (the reference reads mvKeys, equal for rectified stereo and for the undistorted input this library produces).
 * Deterministic: no atomics, a row's record depends on that row's inputs only.  No CPU fallback (ORBFE_ERR_NO_DEVICE). */
typedef struct orbfe_tri_view {        /* what the loop reads of one KeyFrame */
  float Rcw[9], tcw[3], Ow[3];         /* GetRotation() row-major, GetTranslation(), GetCameraCenter() */
  float fx, fy, cx, cy, invfx, invfy, mb, mbf;
  int32_t n_levels;                    /* mnScaleLevels, 1 .. ORBFE_MAX_LEVELS */
  float scale_factors[ORBFE_MAX_LEVELS]; /* mvScaleFactors; slot 1 is read as mfScaleFactor (ratioFactor, :210) whatever n_levels is */
  float level_sigma2[ORBFE_MAX_LEVELS];  /* mvLevelSigma2 */
} orbfe_tri_view;                      /* 224 bytes */
enum {                                 /* orbfe_new_point.code: 0 accepted, else the first `continue` the pair takes */
  ORBFE_TRI_OK = 0,
  ORBFE_TRI_NO_MATCH = 1,              /* matchA[i] < 0 or >= nB, or an octave outside [0, n_levels) of its view: nothing more is read */
  ORBFE_TRI_W_ZERO = 2,                /* :311  the homogeneous coordinate of the linear solution is 0 */
  ORBFE_TRI_LOW_PARALLAX = 3,          /* :322  no stereo and very low parallax (also: a stereo keypoint with depth <= 0) */
  ORBFE_TRI_BEHIND1 = 4,               /* :328  z1 <= 0 */
  ORBFE_TRI_BEHIND2 = 5,               /* :332  z2 <= 0 */
  ORBFE_TRI_REPROJ1 = 6,               /* :346 / :355  reprojection error in pKF1 (5.991 mono, 7.8 stereo, compared in double) */
  ORBFE_TRI_REPROJ2 = 7,               /* :370 / :379  in pKF2 (its right-image term uses pKF1's mbf, as :374 does) */
  ORBFE_TRI_DIST_ZERO = 8,             /* :391 */
  ORBFE_TRI_SCALE = 9                  /* :400  scale consistency */
};
enum { ORBFE_TRI_PATH_NONE = 0, ORBFE_TRI_PATH_LINEAR = 1, ORBFE_TRI_PATH_UNPROJECT1 = 2, ORBFE_TRI_PATH_UNPROJECT2 = 3 };
typedef struct orbfe_new_point {
  float pos[3], normal[3];             /* x3D; mNormalVector.  All eight floats are 0 unless code == 0 */
  float min_distance, max_distance;    /* mfMinDistance, mfMaxDistance (un-scaled, see orbfe_map_point) */
  int32_t idx2;                        /* the pKF2 feature, -1 for ORBFE_TRI_NO_MATCH */
  int32_t code;                        /* ORBFE_TRI_* */
  int32_t path;                        /* ORBFE_TRI_PATH_*: how x3D was (or would have been) obtained */
} orbfe_new_point;                     /* 44 bytes */
/* One (pKF1, pKF2) pair, geometry only.  HOST pointers, synchronous, on the calling thread's current device.  keys = mvKeysUn,
 * u_right = mvuRight and depth = mvDepth of both keyframes (u_right and depth NULL together: every keypoint monocular), matchA[i] =
 * the pKF2 feature matched to pKF1 feature i or -1 (the output of orbfe_search_for_triangulation).  out[i] for every i < nA,
 * *n_new = the number of accepted rows.
 * Limits (ORBFE_ERR_INVALID): 0 <= nA, nB <= 65 535 (the descriptor limit of the search), n_levels of both views in 1 ..
 * ORBFE_MAX_LEVELS, u_right without depth, null pointers other than u_right / depth (keys / matchA / out may be NULL when their
 * count is 0).  nA == 0 launches nothing. */
int orbfe_triangulate_matches(const orbfe_tri_view* view1, const orbfe_keypoint* keys1, const float* u_right1, const float* depth1,
                              int nA, const orbfe_tri_view* view2, const orbfe_keypoint* keys2, const float* u_right2,
                              const float* depth2, int nB, const int32_t* matchA, orbfe_new_point* out, int* n_new);
/* The same for K independent pairs (pKF1, neighbour k) in one launch.  DEVICE pointers, asynchronous on `stream` (NULL: the NULL
 * stream).  pKF1: ONE view and one block of capA keypoint rows; pair k reads its first d_nA[k] rows, its matches d_matchA rows
 * [k*capA, k*capA + d_nA[k]) and writes the same rows of d_out; neighbour k is d_view2[k] and rows [k*capB, k*capB + d_nB[k]) of
 * d_keys2 / d_u_right2 / d_depth2.  d_nA[k] is clamped to [0, capA], d_nB[k] to [0, capB]; rows at and behind d_nA[k] are neither
 * read nor written.  d_n_new[k] = accepted rows of pair k.  A pair's records do not depend on K or on its position in the batch.
 * Limits (ORBFE_ERR_INVALID): 0 <= K <= 65 535 (0: nothing is launched), 1 <= capA, capB <= 65 535, u_right without depth, null
 * pointers other than d_u_right* / d_depth*, records not 4-byte aligned.  n_levels lives in device memory and is not validated
 * here: an octave outside [0, min(n_levels, ORBFE_MAX_LEVELS)) makes the row ORBFE_TRI_NO_MATCH. */
int orbfe_triangulate_matches_batch_device(int K, const orbfe_tri_view* d_view1, const orbfe_keypoint* d_keys1, const float* d_u_right1,
                                           const float* d_depth1, const int32_t* d_nA, int capA, const orbfe_tri_view* d_view2,
                                           const orbfe_keypoint* d_keys2, const float* d_u_right2, const float* d_depth2,
                                           const int32_t* d_nB, int capB, const int32_t* d_matchA, orbfe_new_point* d_out,
                                           int32_t* d_n_new, void* stream);
/* The loop of :215-422 for pKF1 and K neighbours in covisibility order: per neighbour the baseline gate (:221-235), the search of
 * orbfe_search_for_triangulation and the triangulation, back to back on one stream.  pKF1 is uploaded once, its candidate mask
 * stays on the device and the triangulation clears it at every accepted feature, so neighbour k+1's search skips what neighbour k
 * gave a map point (ORBmatcher.cc:655-664); nothing synchronises with the host between neighbours and everything comes back in
 * one copy.  A neighbour record is side B of orbfe_search_for_triangulation plus depth, its view, its epipolar record (F12 and the
 * epipole stay the caller's) and, for the monocular gate, ComputeSceneMedianDepth(2). */
typedef struct orbfe_tri_neighbor {
  const orbfe_keypoint* keys;          /* pKF2->mvKeysUn */
  const uint8_t* desc;                 /* mDescriptors */
  const float* u_right;                /* mvuRight, NULL: monocular */
  const float* depth;                  /* mvDepth, NULL with u_right */
  const uint8_t* has_mp;               /* GetMapPoint(i) != NULL */
  const orbfe_featvec_node* nodes;     /* mFeatVec */
  const int32_t* idx;
  int32_t n, n_nodes;
  orbfe_tri_view view;
  orbfe_epipolar ep;
  float median_depth;                  /* read when monocular != 0 */
} orbfe_tri_neighbor;                  /* 464 bytes (LP64) */
/* HOST pointers, synchronous.  has_mpA is in/out: accepted features are set.  monocular = mbMonocular selects the gate: 0 skips a
 * neighbour with baseline < its mb, else one with baseline / median_depth < 0.01 (compared in double).  only_stereo is the search's
 * bOnlyStereo (false in the reference), check_orientation the matcher's.  The sequential replay of the search (a pKF1 feature listed
 * under two vocabulary nodes) keeps its meaning per neighbour.  The reference's early exit on CheckNewKeyFrames(): pass fewer
 * neighbours.  points[k*nA + i] = the record of pKF1 feature i with neighbour k (all ORBFE_TRI_NO_MATCH for a skipped one),
 * n_matches[k] = the search's return value or -1 for a neighbour the gate skipped, n_new[k] = accepted points.
 * Limits (ORBFE_ERR_INVALID): as orbfe_triangulate_matches for nA, every neighbours[k].n and the views; K >= 0 (0: nothing is
 * launched); node counts >= 0; the FeatureVector checks of orbfe_search_for_triangulation. */
int orbfe_create_new_map_points(const orbfe_keypoint* keysA, const uint8_t* descA, const float* u_rightA, const float* depthA,
                                uint8_t* has_mpA, int nA, const orbfe_featvec_node* nodesA, int n_nodesA, const int32_t* idxA,
                                const orbfe_tri_view* viewA, const orbfe_tri_neighbor* neighbors, int K, int monocular,
                                int only_stereo, int check_orientation, orbfe_new_point* points, int32_t* n_matches, int32_t* n_new);

/* ---- Sim3Solver (L/src/Sim3Solver.cc) ---------------------------------------------------------------------------------------------
 * The RANSAC of LoopClosing::ComputeSim3 between orbfe_search_by_bow and the Sim3 search: a hypothesis is Horn's closed-form
 * similarity from three correspondences (ComputeSim3, :216-322), its score the two-sided reprojection test of CheckInliers
 * (:324-344).  All H hypotheses of a problem are independent, so one launch evaluates them all (one wave per hypothesis, the
 * verdicts of 64 correspondences are one ballot) and a second one applies the sequential rule of iterate (:178-193) to the
 * counts: the solver returns the FIRST hypothesis with count > min_inliers -- every earlier one has a smaller count, so the
 * reference's `>=` test on mnBestInliers holds there -- and without one its best is the LAST hypothesis with the maximal count.
 * iterate(n) in chunks is a cursor over the same sequence (refactored_orb_slam2_amd/sim3.py: iterate_replay).
 * The caller draws the triples (Sim3Solver.cc:155-172; sim3.py: draw_triples); the library holds no random state.
 * csrc/sim3_internal.h states the arithmetic once, float where the reference is float (centroids, Pr, M, P3, projections, errors)
 * and double where it is double (the sums of N, ang, nom / den).  cv::eigen and cv::Rodrigues are not available where this library
 * is built: the eigenvector of the largest eigenvalue of the 4x4 comes from this project's own cyclic Jacobi in double on the float
 * matrix, Rodrigues is evaluated in double and rounded to float.  Two properties:
 *   - q and -q give the same rotation through the atan2 form (the axis flips and the angle 2 * ang becomes 2 * pi - 2 * ang), so the
 *     sign convention of the eigenvector does not matter;
 *   - a quaternion with a zero imaginary part (norm(vec) == 0) is 0 / 0 in the reference: every comparison with NaN is false and the
 *     hypothesis has 0 inliers.  Here too: n_inliers == 0 and an all-zero inlier word row, the rest of the record unspecified (it may
 *     hold NaN); nothing traps and no other record is touched.
 * Deterministic: no atomics, a hypothesis' record and words depend on its problem and its triple only.  No CPU fallback. */
#define ORBFE_SIM3_MAX_PAIRS 1024        /* correspondences of a problem: 48 bytes each once prepared, 48 KiB = the LDS a workgroup
                                            stages them in (three workgroups per CU); a loop candidate has tens to hundreds */
#define ORBFE_SIM3_MAX_HYPOTHESES 4096   /* the reference never exceeds its maxIterations (300) */
typedef struct orbfe_sim3_view {         /* what the solver reads of one KeyFrame */
  float Rcw[9], tcw[3];                  /* GetRotation() row-major, GetTranslation() */
  float fx, fy, cx, cy;                  /* mK */
} orbfe_sim3_view;                       /* 64 bytes */
typedef struct orbfe_sim3_pair {         /* one kept match (Sim3Solver.cc:62-100) */
  float Xw1[3], Xw2[3];                  /* pMP1->GetWorldPos(), pMP2->GetWorldPos() */
  float max_err1, max_err2;              /* (float)(size_t)(9.210 * mvLevelSigma2[octave]): the caller truncates, as the
                                            reference's vector<size_t> does (include/Sim3Solver.h:74-75) */
} orbfe_sim3_pair;                       /* 32 bytes */
typedef struct orbfe_sim3_hypothesis {
  float s, R[9], t[3];                   /* ms12i, mR12i row-major, mt12i; all 0 for a triple the device form rejects */
  int32_t n_inliers;                     /* mnInliersi */
  int32_t reserved[2];
} orbfe_sim3_hypothesis;                 /* 64 bytes */
typedef struct orbfe_sim3_result {
  int32_t returned;                      /* the hypothesis iterate returns on (first count > min_inliers), or -1 */
  int32_t n_inliers;                     /* its count, 0 without one */
  int32_t best;                          /* == returned when >= 0, else the last hypothesis with the maximal count; -1: none evaluated */
  int32_t best_inliers;                  /* mnBestInliers */
  float T12[12];                         /* mBestT12, rows 0-2: [s * R | t] */
  float s, R[9], t[3];                   /* GetEstimatedScale / Rotation / Translation */
  int32_t reserved[3];
} orbfe_sim3_result;                     /* 128 bytes */
/* SetRansacParameters (:112-136) for N correspondences: epsilon = (float)min_inliers / N, ceil(log(1 - probability) /
 * log(1 - pow(epsilon, 3))) in double, 1 when min_inliers == N, then max(1, min(that, max_iterations)).  Pure host.
 * ORBFE_ERR_INVALID: N < 1, min_inliers < 0 or > N, max_iterations < 0, probability outside (0, 1). */
int orbfe_sim3_ransac_iterations(int N, double probability, int min_inliers, int max_iterations);
/* One problem.  HOST pointers, synchronous, on the calling thread's current device.  triples[3*h .. 3*h+2] index the pairs.
 * hyps[H] and words[H][ceil(n/64)] are optional (NULL skips their download); bit (i & 63) of word i / 64 is the verdict of pair i,
 * the tail bits of the last word are 0 and n_inliers is the popcount of the row.  result_mask[ceil(n/64)] is the word row of
 * result->best (zeros without one).  n < 3 or n < min_inliers (:144-147): returned = best = -1, no hypothesis is evaluated, hyps
 * and words come back zero and nothing is launched.  One packed upload, one packed download, one synchronisation.
 * Limits (ORBFE_ERR_INVALID): 0 <= n <= ORBFE_SIM3_MAX_PAIRS, 0 <= H <= ORBFE_SIM3_MAX_HYPOTHESES, min_inliers >= 0, a triple
 * index outside [0, n) or repeated within its triple, null views / result / result_mask, null pairs with n > 0 or triples with H > 0. */
int orbfe_sim3_solve(const orbfe_sim3_view* view1, const orbfe_sim3_view* view2, const orbfe_sim3_pair* pairs, int n,
                     const int32_t* triples, int H, int fix_scale, int min_inliers, orbfe_sim3_hypothesis* hyps, uint64_t* words,
                     orbfe_sim3_result* result, uint64_t* result_mask);
/* P problems in one launch pair.  DEVICE pointers, asynchronous on `stream` (NULL: the NULL stream).  Problem p: d_view1[p],
 * d_view2[p], d_fix_scale[p], d_min_inliers[p], pair rows [p*cap, p*cap + d_n[p]), triple rows [p*h_cap, p*h_cap + d_H[p]); it writes
 * the same rows of d_hyps, the first ceil(d_n[p]/64) words of rows [p*h_cap, ..) of d_words (row stride W = ceil(cap/64)), d_result[p]
 * and the first ceil(d_n[p]/64) words of d_result_mask[p*W ..].  Counts are clamped to [0, cap] / [0, h_cap]; rows and words behind
 * them are neither read nor written.  A triple with an index outside [0, d_n[p]) or a repeated one yields an all-zero record and
 * word row and reads nothing outside the problem.  A problem with fewer than 3 or than min_inliers pairs gets returned = best = -1
 * and nothing else.  A problem's bytes do not depend on P, on its position in the batch or on the run.
 * Limits (ORBFE_ERR_INVALID): 0 <= P <= 65 535 (0: nothing is launched), 1 <= cap <= ORBFE_SIM3_MAX_PAIRS, 1 <= h_cap <=
 * ORBFE_SIM3_MAX_HYPOTHESES, null pointers, records not 4-byte (d_words / d_result_mask: 8-byte) aligned. */
int orbfe_sim3_solve_batch_device(int P, const orbfe_sim3_view* d_view1, const orbfe_sim3_view* d_view2, const orbfe_sim3_pair* d_pairs,
                                  const int32_t* d_n, int cap, const int32_t* d_triples, const int32_t* d_H, int h_cap,
                                  const int32_t* d_fix_scale, const int32_t* d_min_inliers, orbfe_sim3_hypothesis* d_hyps,
                                  uint64_t* d_words, orbfe_sim3_result* d_result, uint64_t* d_result_mask, void* stream);

/* ---- PnPsolver (L/src/PnPsolver.cc) -----------------------------------------------------------------------------------------------
 * The RANSAC of Tracking::Relocalization (L/src/Tracking.cc:1258-1283) between orbfe_search_by_bow and orbfe_pose_optimization: a
 * hypothesis is EPnP (compute_pose, :451-500) on four correspondences, its score the reprojection test of CheckInliers (:291-320);
 * a hypothesis that becomes the best so far is refined by EPnP on all its inliers (Refine, :248-289).  All H hypotheses of a problem
 * are independent, so one launch evaluates them all (one wave per hypothesis).  A failed refine is deterministic, so the refines
 * that matter are those of the STRICT PREFIX MAXIMA of the count sequence with count >= min_inliers; a second launch evaluates
 * them side by side, and a third applies the sequential rule of iterate (:205-243) to the counts and refine verdicts: find()
 * returns the refined pose of the first prefix maximum whose refine has count > min_inliers, and without one the best hypothesis
 * (the first with the maximal count) if that count is >= min_inliers.  iterate(n) in chunks is a cursor over the same records
 * (refactored_orb_slam2_amd/pnp.py: iterate_replay).  The caller draws the minimal sets (:184-197; pnp.py: draw_minimal_sets) and
 * sets the parameters (orbfe_pnp_ransac_parameters); the library holds no random state.
 * csrc/pnp_internal.h states the arithmetic once: double where the reference is double (all of compute_pose), and the float
 * roundings of CheckInliers where it rounds.  The legacy CvMat routines are not available where this library is built: symmetric
 * eigenproblems (3x3 PCA, 12x12 MtM) go through this project's cyclic two-sided Jacobi in double, the 3x3 inverse, the 3x3 SVD of
 * Horn's step and the three small least-squares solves through a one-sided Jacobi SVD without any threshold.
 *   - With four points MtM has a four-dimensional null space and the four vectors an SVD returns for it are an arbitrary basis,
 *     which the rest of EPnP depends on.  The basis this library chose is part of the interface: orbfe_pnp_diag exports it, with
 *     the control points (whose PCA axes have a free sign each), so that a reading of the reference can continue from it.
 *   - A coplanar or repeated set makes the third PCA eigenvalue 0 and the inverse 0 / 0: everything behind it is NaN, every
 *     comparison of CheckInliers is false, n_inliers == 0 and the word row is all zero; the rest of the record is unspecified (it
 *     may hold NaN).  Every iteration has a cap, nothing traps and no other record is touched.
 * Deterministic: no atomics, a hypothesis' record depends on its problem and its minimal set only.  No CPU fallback. */
#define ORBFE_PNP_MAX_POINTS 1024        /* correspondences of a problem: 24 bytes each, 24 KiB of the LDS a workgroup stages them
                                            in beside its waves' workspaces; a relocalisation candidate has tens to hundreds */
#define ORBFE_PNP_MAX_HYPOTHESES 4096    /* the reference never exceeds its maxIterations (300) */
typedef struct orbfe_pnp_point {         /* one kept match (PnPsolver.cc:81-100) */
  float Xw[3];                           /* pMP->GetWorldPos() */
  float u, v;                            /* mvKeysUn[i].pt */
  float max_err;                         /* mvLevelSigma2[octave] * th2 in float (:155) */
} orbfe_pnp_point;                       /* 24 bytes */
typedef struct orbfe_pnp_camera {
  float fx, fy, cx, cy;                  /* the frame's floats; the solver widens them to double (:104-107) */
} orbfe_pnp_camera;                      /* 16 bytes */
typedef struct orbfe_pnp_hypothesis {
  double R[9], t[3];                     /* mRi row-major, mti */
  int32_t n_inliers;                     /* mnInliersi */
  int32_t winner;                        /* 0, 1, 2: which of find_betas_approx_1 / _2 / _3 had the smallest reprojection error */
  int32_t refine;                        /* row of its refine record (== its own index) when it is a strict prefix maximum with
                                            count >= min_inliers, else -1 */
  int32_t reserved;
} orbfe_pnp_hypothesis;                  /* 112 bytes; all 0 (refine -1) for a set the device form rejects */
typedef struct orbfe_pnp_refine {
  double R[9], t[3];                     /* the pose of Refine() on the hypothesis' inliers */
  int32_t n_inliers;                     /* mnRefinedInliers */
  int32_t success;                       /* n_inliers > min_inliers (:277) */
  int32_t winner;
  int32_t n_used;                        /* correspondences the refine solved on (the hypothesis' count) */
} orbfe_pnp_refine;                      /* 112 bytes; rows of hypotheses without a refine are not written */
typedef struct orbfe_pnp_result {        /* what find() returns */
  int32_t returned;                      /* the hypothesis at which find() returns: the first whose refine succeeds; at exhaustion the
                                            best one if its count is >= min_inliers; else -1 */
  int32_t refined;                       /* 1: Tcw / n_inliers are the refine record's of `returned`, 0: the hypothesis' own */
  int32_t n_inliers;                     /* nInliers, 0 without a pose */
  int32_t best;                          /* the first hypothesis with the maximal count >= min_inliers when find() ended, or -1 */
  int32_t best_inliers;                  /* mnBestInliers */
  int32_t reserved[3];
  float Tcw[12];                         /* rows 0-2 of the returned matrix: the doubles rounded to float as convertTo does */
} orbfe_pnp_result;                      /* 80 bytes */
typedef struct orbfe_pnp_diag {          /* one compute_pose: the conventions it chose and what it derived from them */
  double cws[12];                        /* the control points: centroid, then centroid + sqrt(d_k / n) * axis_k */
  double V[48];                          /* v[0..3] (:727-730): unit vectors of the four smallest eigenvalues of MtM, smallest first */
  double eig[5];                         /* their eigenvalues, and the fifth smallest */
  double betas[12];                      /* Betas[1..3] after gauss_newton */
  double rep_errors[3];                  /* rep_errors[1..3] */
} orbfe_pnp_diag;                        /* 640 bytes */
/* SetRansacParameters (:119-156) for N correspondences, except the error bounds.  *min_inliers_out = max((int)(N * epsilon),
 * min_inliers, min_set) with the float product truncated, *epsilon_out = max(epsilon, (float)that / N), *iterations_out = 1 when
 * that == N, else ceil(log(1 - probability) / log(1 - pow(epsilon, 3))) in double, then max(1, min(it, max_iterations)).  Pure host.
 * ORBFE_ERR_INVALID: N < 1, min_inliers < 0, max_iterations < 0, min_set != 4, probability outside (0, 1), epsilon outside [0, 1],
 * a null output. */
int orbfe_pnp_ransac_parameters(int N, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                                int32_t* min_inliers_out, int32_t* iterations_out, float* epsilon_out);
/* One problem.  HOST pointers, synchronous, on the calling thread's current device.  sets[4*h .. 4*h+3] index the points; min_set
 * must be 4.  min_inliers is the adjusted value (orbfe_pnp_ransac_parameters).  Optional outputs (NULL skips them): hyps[H],
 * words[H][ceil(n/64)], refines[H], refine_words[H][ceil(n/64)], diag[H], refine_diag[H]; rows of refines / refine_words /
 * refine_diag are meaningful where hyps[h].refine == h and zero elsewhere.  Bit (i & 63) of word i / 64 is the verdict of point i,
 * the tail bits of the last word are 0 and n_inliers is the popcount of the row.  result_mask[ceil(n/64)] is the word row that goes
 * with result->Tcw (zeros without a pose).  n < min_inliers (:171-174): returned = best = -1, nothing is evaluated or launched, the
 * optional outputs come back zero.  One packed upload, one packed download, one synchronisation.
 * Limits (ORBFE_ERR_INVALID): 0 <= n <= ORBFE_PNP_MAX_POINTS, 0 <= H <= ORBFE_PNP_MAX_HYPOTHESES, min_inliers >= 4, min_set == 4, an
 * index outside [0, n) or repeated within its set, null camera / result / result_mask, null points with n > 0 or sets with H > 0. */
int orbfe_pnp_solve(const orbfe_pnp_camera* camera, const orbfe_pnp_point* points, int n, const int32_t* sets, int min_set, int H,
                    int min_inliers, orbfe_pnp_hypothesis* hyps, uint64_t* words, orbfe_pnp_refine* refines, uint64_t* refine_words,
                    orbfe_pnp_diag* diag, orbfe_pnp_diag* refine_diag, orbfe_pnp_result* result, uint64_t* result_mask);
/* P problems in three launches.  DEVICE pointers, asynchronous on `stream` (NULL: the NULL stream).  Problem p: d_camera[p],
 * d_min_inliers[p], point rows [p*cap, p*cap + d_n[p]), set rows [p*h_cap, p*h_cap + d_H[p]); it writes the same rows of d_hyps (and
 * of d_refines / d_diag / d_refine_diag where a refine ran; d_diag and d_refine_diag may be NULL), the first ceil(d_n[p]/64) words of
 * those rows of d_words / d_refine_words (row stride W = ceil(cap/64)), d_result[p] and the first ceil(d_n[p]/64) words of
 * d_result_mask[p*W ..].  Counts are clamped to [0, cap] / [0, h_cap]; rows and words behind them are neither read nor written.  A
 * set with an index outside [0, d_n[p]) or a repeated one yields an all-zero record (refine -1) and word row and reads nothing
 * outside the problem.  A problem with fewer than 4 or than min_inliers points gets returned = best = -1 and nothing else.  A
 * problem's bytes do not depend on P, on its position in the batch or on the run.
 * Limits (ORBFE_ERR_INVALID): 0 <= P <= 65 535 (0: nothing is launched), 1 <= cap <= ORBFE_PNP_MAX_POINTS, 1 <= h_cap <=
 * ORBFE_PNP_MAX_HYPOTHESES, null pointers, records not 8-byte aligned (d_camera / d_points / d_n / d_sets / d_H / d_min_inliers /
 * d_result: 4-byte). */
int orbfe_pnp_solve_batch_device(int P, const orbfe_pnp_camera* d_camera, const orbfe_pnp_point* d_points, const int32_t* d_n, int cap,
                                 const int32_t* d_sets, const int32_t* d_H, int h_cap, const int32_t* d_min_inliers,
                                 orbfe_pnp_hypothesis* d_hyps, uint64_t* d_words, orbfe_pnp_refine* d_refines, uint64_t* d_refine_words,
                                 orbfe_pnp_diag* d_diag, orbfe_pnp_diag* d_refine_diag, orbfe_pnp_result* d_result,
                                 uint64_t* d_result_mask, void* stream);

/* ---- Optimizer::OptimizeSim3 (L/src/Optimizer.cc:1381-1573) ----------------------------------------------------------------------
 * The last step of LoopClosing::ComputeSim3 (L/src/LoopClosing.cc:224-322): the similarity S12 of orbfe_sim3_result and the matches
 * of the Sim3 search are refined by g2o's Levenberg on one 7-DoF vertex with two Huber edges per correspondence -- x1 = S12 X2 in
 * image 1 and x2 = S12^-1 X1 in image 2, points fixed -- and the candidate is accepted when the return value is >= 20.  Schedule:
 * optimize(5); every correspondence with chi2 > th2 on either edge is dropped (nBad); fewer than 10 left: return 0 and the
 * similarity is NOT written, although the dropped matches are already nulled; otherwise optimize(10 when nBad > 0, else 5) on the
 * rest, a second classification, and the estimate is returned with the number of correspondences that survived both.
 * csrc/optsim3_internal.h states the arithmetic once, all in double: g2o::Sim3 (exp with its four branches on 1e-5, map, inverse,
 * operator*), oplus with the fixed-scale rule, the edges' NUMERIC Jacobians (central differences, delta = 1e-9, through oplus: the
 * reference's edges have no linearizeOplus), Huber, the quadratic form and g2o's Levenberg (lambda = 1e-5 * max diag H at iteration
 * 0 of each call, at most 10 trials per iteration).  The camera-frame points are the float gemm R * Xw + t of the reference.  Eigen
 * and g2o cannot be built where this library is built: the 7 x 7 system is solved by this project's unpivoted L D L^T, the
 * quaternion formulas are Eigen's written out (a reading, unpinned).
 * One deliberate deviation, the one of orbfe_pose_optimization: a correspondence is classified by its chi2 at the final estimate of
 * the optimize() call.  The reference reads the error that the last Levenberg trial left in the edge, also when that trial was
 * rejected; such a step is taken at a large lambda and is tiny.
 * Deterministic: no atomics, a problem's result and flags depend on its own rows only.  No CPU fallback. */
typedef struct orbfe_optsim3_pair {      /* one correspondence that passed the filters of Optimizer.cc:1436-1468; 48 bytes */
  float Xw1[3], Xw2[3];                  /* GetWorldPos() of pMP1, pMP2 */
  float obs1[2], obs2[2];                /* mvKeysUn[i].pt of KF1, mvKeysUn[i2].pt of KF2 */
  float inv_sigma2_1, inv_sigma2_2;      /* mvInvLevelSigma2[octave] of each */
} orbfe_optsim3_pair;
typedef struct orbfe_optsim3_result {    /* s, R[9], t[3]: the input's bits when n_inliers == 0 by the < 10 rule */
  float s, R[9], t[3];                   /* g2oS12: scale(), rotation().toRotationMatrix() row-major, translation() */
  int32_t n_pairs, n_bad, n_inliers;     /* nCorrespondences, nBad of the first classification, the return value */
  int32_t iterations[2];                 /* Levenberg iterations of the two optimize() calls (reported, not part of parity) */
  int32_t reserved[2];
} orbfe_optsim3_result;                  /* 80 bytes */
/* One problem.  HOST pointers, synchronous, on the calling thread's current device.  view1 / view2: GetRotation, GetTranslation and
 * mK of pKF1 / pKF2; s_R_t_in: g2oS12 as 13 floats (scale, rotation row-major, translation -- LoopClosing builds it from the float
 * matrices of the solver); th2: the chi-square bound (10 in LoopClosing), its float square root is the Huber delta; bad[n]: 1 where
 * the reference nulls the vpMatches1 entry (in either classification).  n < 10 still runs the first optimize(5) and classification,
 * as the reference does, and returns n_inliers == 0 with the input transform; n == 0 launches nothing.  One packed upload, one
 * launch, one packed download.
 * Limits (ORBFE_ERR_INVALID): 0 <= n <= 9 500, th2 > 0 (a NaN is refused), null views / s_R_t_in / result, null pairs or bad with
 * n > 0. */
int orbfe_optimize_sim3(const orbfe_sim3_view* view1, const orbfe_sim3_view* view2, const orbfe_optsim3_pair* pairs, int n,
                        const float* s_R_t_in, float th2, int fix_scale, orbfe_optsim3_result* result, uint8_t* bad);
/* P problems in one launch, one workgroup each.  DEVICE pointers, asynchronous on `stream` (NULL: the NULL stream).  Problem p:
 * d_view1[p], d_view2[p], d_s_R_t_in[13 * p ..], d_th2[p], d_fix_scale[p], pair rows [p*cap, p*cap + d_n[p]); it writes d_result[p] and
 * the same rows of d_bad.  Counts are clamped to [0, cap]; rows behind them are neither read nor written.  A d_th2[p] that is not
 * > 0 is not checked on the device: every comparison with it decides as IEEE does, nothing traps and no other problem is touched.
 * A problem's bytes do not depend on P, on its position in the batch or on the run.
 * Limits (ORBFE_ERR_INVALID): 0 <= P <= 65 535 (0: nothing is launched), 0 <= cap <= 9 500, null pointers (d_pairs and d_bad may be
 * null when cap == 0), records not 4-byte aligned. */
int orbfe_optimize_sim3_batch_device(int P, const orbfe_sim3_view* d_view1, const orbfe_sim3_view* d_view2,
                                     const orbfe_optsim3_pair* d_pairs, const int32_t* d_n, int cap, const float* d_s_R_t_in,
                                     const float* d_th2, const int32_t* d_fix_scale, orbfe_optsim3_result* d_result, uint8_t* d_bad,
                                     void* stream);

/* ---- Optimizer::LocalBundleAdjustment (L/src/Optimizer.cc:437-760) ------------------------------------------------------------------
 * The call of LocalMapping::Run behind orbfe_create_new_map_points and the fuse searches: the poses of the local keyframes and the
 * positions of the map points they see are refined together by g2o's Levenberg, the keyframes that only see those points held fixed.
 * One vertex of 6 unknowns per free keyframe, one of 3 per point, one edge per observation: EdgeSE3ProjectXYZ (2 rows) where
 * u_right < 0, EdgeStereoSE3ProjectXYZ (3 rows) otherwise, information inv_sigma2 * I, analytic Jacobians.  Schedule: optimize(5) with
 * a Huber kernel on every edge (delta = (float)sqrt(5.991) / (float)sqrt(7.815)); every edge with chi2 > 5.991 / 7.815 or a
 * non-positive depth goes to level 1; all Huber kernels off; optimize(10) over the level-0 edges; a second classification of every
 * edge is the erase list.  A vertex without a level-0 edge is not active in an optimize call: it keeps its estimate.
 * csrc/lba_internal.h states the arithmetic once, all in double: the system of BlockSolver_6_3 with the points marginalised (Hpp,
 * Hll, Hpl, lambda on both diagonals, Hll^-1 per point by Eigen's cofactor formula, Hschur = Hpp - sum Hpl Hll^-1 Hpl^T, back
 * substitution), updates exp(x) * estimate for poses and += for points, and g2o's Levenberg over all active vertices (lambda = 1e-5 *
 * max diag at iteration 0 of each optimize call, computeScale over the whole update, at most 10 trials after a failure, push / pop
 * of every estimate).  An edge is classified by the chi2 its last evaluation left in it -- the last trial of the optimize call, also
 * a rejected one -- and by its depth at the estimates, as the reference does.  Eigen and g2o cannot be built where this library is
 * built: SimplicialLLT is a dense unpivoted L L^T of the reduced system here, a pivot that is not > 0 is its failure, and after such a
 * failure the estimates are left alone (g2o applies the stale solution and pops it).  DESIGN section 2: a reading, unpinned.
 * Edges must be listed point by point, keyframes ascending inside a point, and no (keyframe, point) pair twice: the reference's
 * observations are a map keyed by keyframe.  The host form sorts; the device form checks and refuses (rounds = -1).
 * Not taken over: the stop flag is not read while the launch runs.
 * Deterministic: no floating-point atomics, every block is summed by one lane in list order; a problem's bytes depend on its own
 * rows only.  No CPU fallback.
 * Limits, each refused with ORBFE_ERR_INVALID one step past it (pinned by tests/test_lba_cpu.py and tests/test_lba_gpu.py):
 *   ORBFE_LBA_MAX_FREE       64 free keyframes: the reduced system of 384 unknowns is 1.2 MB of workspace and its factorisation 9.4
 *                            million updates per trial on the ONE workgroup a problem has -- a few milliseconds; both grow with
 *                            the square and the cube, and the local windows of the reference stay below it
 *   ORBFE_LBA_MAX_KEYFRAMES  256 keyframes, free and fixed: their estimates and the saved ones live in LDS (28 KB)
 *   ORBFE_LBA_MAX_POINTS     65 535 points
 *   ORBFE_LBA_MAX_EDGES      65 535 x 4 edges
 *   ORBFE_LBA_MAX_PROBLEMS   65 535 problems per launch */
#define ORBFE_LBA_MAX_FREE 64
#define ORBFE_LBA_MAX_KEYFRAMES 256
#define ORBFE_LBA_MAX_POINTS 65535
#define ORBFE_LBA_MAX_EDGES 262140
#define ORBFE_LBA_MAX_PROBLEMS 65535
#define ORBFE_LBA_FIRST_ROUND_ONLY 1      /* flags: the reference's bDoMore = false -- round 1, its classification as the erase list */
#define ORBFE_LBA_ERASE 1                 /* bits of an erase byte: the observation is on the erase list; */
#define ORBFE_LBA_DROPPED 2               /* the edge was at level 1 in round 2 */
typedef struct orbfe_lba_edge {           /* one observation; 24 bytes */
  int32_t kf, point;                      /* indices into the problem's keyframes and points */
  float u, v, u_right;                    /* mvKeysUn[i].pt, mvuRight[i] (< 0: a monocular edge) */
  float inv_sigma2;                       /* mvInvLevelSigma2[octave] of the keyframe; finite and > 0 */
} orbfe_lba_edge;
typedef struct orbfe_lba_problem {        /* where one problem of a batch lies in the batch's arrays; 24 bytes */
  int32_t kf_offset, n_kf;                /* rows of d_poses / d_fixed / d_poses_out */
  int32_t point_offset, n_points;         /* records of d_points, rows of d_points_out */
  int32_t edge_offset, n_edges;           /* rows of d_edges / d_erase */
} orbfe_lba_problem;
typedef struct orbfe_lba_result {         /* 72 bytes, 8-byte aligned */
  int32_t rounds;                         /* optimize calls run: 0 (no free keyframe or no edge), 1, 2; -1: refused on the device */
  int32_t n_free, n_edges;
  int32_t iterations[2], trials[2];       /* Levenberg iterations and trials of each round (reported, not part of parity) */
  int32_t n_dropped, n_erase;             /* edges at level 1 after round 1, edges on the erase list */
  int32_t reserved;
  double chi2_first[2], chi2_final[2];    /* activeRobustChi2 at the start and at the end of each round */
} orbfe_lba_result;
/* One problem.  HOST pointers, synchronous, on the calling thread's current device.  camera: fx fy cx cy mbf are read; poses: n_kf x
 * 12 floats, rows of [R | t] (GetPose); fixed[n_kf]: != 0 for a keyframe of lFixedCameras or with mnId == 0; points: n_points x 3
 * floats (GetWorldPos); edges in any order (sorted here; the same pair twice is refused).  poses_out: a free keyframe's pose as
 * Converter::toCvMat(SE3Quat) rounds it, a fixed one's bytes as given; points_out: a point without an edge as given; erase[n_edges]:
 * ORBFE_LBA_* bits in the caller's edge order.  A problem without a free keyframe or without an edge returns its inputs, rounds = 0.
 * One upload, one launch, one download; the workspace is allocated for the call.
 * Limits (ORBFE_ERR_INVALID): the ORBFE_LBA_MAX_* above, n_kf, n_points, n_edges >= 0, every edge's kf and point in range, inv_sigma2
 * finite and > 0, null camera / result, null arrays with a count > 0, flags outside ORBFE_LBA_FIRST_ROUND_ONLY. */
int orbfe_local_bundle_adjustment(const orbfe_pose_camera* camera, const float* poses, const uint8_t* fixed, int n_kf, const float* points,
                                  int n_points, const orbfe_lba_edge* edges, int n_edges, int flags, float* poses_out, float* points_out,
                                  uint8_t* erase, orbfe_lba_result* result);
/* The bytes of workspace a batch of P problems needs whose counts stay within kf_cap keyframes, point_cap points and edge_cap edges
 * each.  HOST pointer.  Limits (ORBFE_ERR_INVALID): 0 <= P <= ORBFE_LBA_MAX_PROBLEMS, the caps >= 0 and within the ORBFE_LBA_MAX_*
 * (kf_cap: ORBFE_LBA_MAX_KEYFRAMES), null bytes. */
int orbfe_lba_workspace_bytes(int P, int kf_cap, int point_cap, int edge_cap, size_t* bytes);
/* P problems in one launch, one workgroup each.  DEVICE pointers, asynchronous on `stream` (NULL: the NULL stream).  Problem p lies
 * where d_problems[p] says: n_kf rows of d_poses (12 floats) / d_fixed / d_poses_out from kf_offset on, n_points records of d_points
 * (point_stride bytes apart, the position first: three floats, orbfe_new_point and orbfe_map_point qualify) and rows of d_points_out
 * (3 floats) from point_offset on, n_edges rows of d_edges / d_erase from edge_offset on.  Rows no problem names are neither read nor
 * written; inputs are not modified.  A problem whose counts are negative or exceed the caps, which has more than ORBFE_LBA_MAX_FREE
 * free keyframes, or whose edge list breaks a rule (index out of range, inv_sigma2 not finite or not > 0, not in (point, keyframe)
 * order, a pair twice) is refused by its workgroup: rounds = -1, poses and points copied through, erase bytes 0; no other problem is
 * touched.  d_workspace: workspace_bytes >= what orbfe_lba_workspace_bytes states for (P, kf_cap, point_cap, edge_cap), 256-byte
 * aligned; its contents mean nothing before or after.  A problem's bytes do not depend on P, on its position or on the run.
 * Limits (ORBFE_ERR_INVALID): as orbfe_lba_workspace_bytes (P == 0: nothing is launched), point_stride >= 12 and a multiple of 4,
 * a workspace that is too small or misaligned, null pointers, records not 4-byte (d_result: 8-byte) aligned, unknown flags. */
int orbfe_local_bundle_adjustment_batch_device(int P, const orbfe_pose_camera* d_camera, const orbfe_lba_problem* d_problems,
                                               const float* d_poses, const uint8_t* d_fixed, const uint8_t* d_points, int point_stride,
                                               const orbfe_lba_edge* d_edges, int kf_cap, int point_cap, int edge_cap, int flags,
                                               float* d_poses_out, float* d_points_out, uint8_t* d_erase, orbfe_lba_result* d_result,
                                               void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- Optimizer::BundleAdjustment (L/src/Optimizer.cc:43-231) -----------------------------------------------------------------------
 * The full bundle adjustment behind GlobalBundleAdjustemnt: the call of Tracking::CreateInitialMapMonocular (20 iterations, robust)
 * and of LoopClosing::RunGlobalBundleAdjustment (10 iterations, not robust).  The same graph as the local bundle adjustment above --
 * its vertices, its two edge types, its records (orbfe_lba_edge, orbfe_lba_problem), its edge order, its workspace
 * (orbfe_lba_workspace_bytes), its arithmetic (csrc/lba_internal.h) and its one workgroup per problem (csrc/lba_optimize.h) -- under
 * another schedule: ONE optimize(n_iterations), the Huber kernel on every edge iff ORBFE_BA_ROBUST; no classification of the edges,
 * no second round, no erase list.  The Huber delta of a monocular edge is (float)sqrt(5.99) here (:82), where the local bundle
 * adjustment has (float)sqrt(5.991); the stereo delta is (float)sqrt(7.815) in both.  fixed[k] != 0 for the keyframe with mnId == 0.
 * A point without an edge is left out of the graph and keeps its bytes.  EVERY keyframe comes back as
 * Converter::toCvMat(SE3Quat) rounds its estimate (:189-203) -- a fixed one and a free one without an edge: the pose that went in,
 * through the quaternion and back.
 * Not taken over: the stop flag is not read while the launch runs.
 * Deterministic: no atomics; a problem's bytes depend on its own rows only, not on P or on its place in the batch.  No CPU fallback.
 * Limits, each refused with ORBFE_ERR_INVALID one step past it (pinned by tests/test_ba_cpu.py and tests/test_ba_gpu.py): the
 * ORBFE_LBA_MAX_* of the kernel it shares, and
 *   ORBFE_BA_MAX_ITERATIONS  20 iterations: the most a caller of the reference asks for (Tracking: 20, LoopClosing: 10, the default
 *                            5).  A launch cannot be interrupted and an iteration runs up to ten trials, so the cap is what bounds
 *                            a launch.  Measured: 9 ms per trial at 8 016 edges and 20 free keyframes, 4 ms per trial at the 7 194
 *                            edges of a two-keyframe map at the initialiser's cap (profiles/local_bundle_adjustment.md,
 *                            profiles/initial_map.md), i.e. 0.1 s and at worst 1 s for 20 iterations there.  NOT measured: a trial
 *                            at the largest problem the limits admit (262 140 edges, 64 free keyframes); by operation count it is
 *                            about a hundred times the first figure, so 20 iterations there are tens of seconds and at worst
 *                            minutes.  A larger cap would admit nothing the reference asks for and multiply that */
#define ORBFE_BA_MAX_ITERATIONS 20
#define ORBFE_BA_ROBUST 1                 /* flags: the reference's bRobust -- a Huber kernel on every edge */
typedef struct orbfe_ba_result {          /* 40 bytes, 8-byte aligned */
  int32_t rounds;                         /* 1: optimize() ran; 0: no free keyframe or no edge; -1: refused on the device */
  int32_t n_free, n_edges;
  int32_t iterations, trials;             /* Levenberg iterations and trials (reported, not part of parity) */
  int32_t reserved;
  double chi2_first, chi2_final;          /* activeRobustChi2 at the start and at the end */
} orbfe_ba_result;
/* One problem.  HOST pointers, synchronous, on the calling thread's current device; arguments as orbfe_local_bundle_adjustment's
 * (edges in any order, sorted here; the same pair twice is refused).  A problem without a free keyframe or without an edge returns
 * its inputs, rounds = 0.  One upload, one launch, one download; the workspace is allocated for the call.
 * Limits (ORBFE_ERR_INVALID): as orbfe_local_bundle_adjustment, 1 <= n_iterations <= ORBFE_BA_MAX_ITERATIONS, flags outside
 * ORBFE_BA_ROBUST. */
int orbfe_bundle_adjustment(const orbfe_pose_camera* camera, const float* poses, const uint8_t* fixed, int n_kf, const float* points,
                            int n_points, const orbfe_lba_edge* edges, int n_edges, int n_iterations, int flags, float* poses_out,
                            float* points_out, orbfe_ba_result* result);
/* P problems in one launch, one workgroup each.  DEVICE pointers, asynchronous on `stream` (NULL: the NULL stream).  Layout, refusal
 * of a problem by its workgroup (rounds = -1, poses and points copied through, no other problem touched) and workspace as
 * orbfe_local_bundle_adjustment_batch_device; n_iterations and flags hold for every problem.
 * Limits (ORBFE_ERR_INVALID): as that call, 1 <= n_iterations <= ORBFE_BA_MAX_ITERATIONS, flags outside ORBFE_BA_ROBUST. */
int orbfe_bundle_adjustment_batch_device(int P, const orbfe_pose_camera* d_camera, const orbfe_lba_problem* d_problems,
                                         const float* d_poses, const uint8_t* d_fixed, const uint8_t* d_points, int point_stride,
                                         const orbfe_lba_edge* d_edges, int kf_cap, int point_cap, int edge_cap, int n_iterations,
                                         int flags, float* d_poses_out, float* d_points_out, orbfe_ba_result* d_result,
                                         void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- Global bundle adjustment beyond one workgroup (LoopClosing::RunGlobalBundleAdjustment's call of BundleAdjustment) ----------------
 * The same function, graph, records, edge order, arithmetic (csrc/lba_internal.h) and result record as orbfe_bundle_adjustment, for
 * ONE map too large for one workgroup: every phase of a trial is a launch over the whole device (csrc/gba_kernels.hip), the
 * reduced system is factored by a blocked dense L L^T over tiles of ORBFE_GBA_TILE_KEYFRAMES row blocks, and a one-workgroup
 * control kernel keeps the Levenberg bookkeeping on the device.  Every sum keeps the owner and the order of the one-workgroup form,
 * so a problem within the ORBFE_LBA_MAX_* limits gives the same bytes from both (pinned by tests/test_gba_gpu.py).
 * The host reads one control record per trial (pinned memory, one stream synchronisation) and enqueues the next trial's launches:
 * BOTH forms below are therefore SYNCHRONOUS on their stream -- they return when the outputs are written.
 * Not taken over: the stop flag is not read between iterations; no fill-reducing ordering; one problem per call.
 * Deterministic: no floating-point atomics; no CPU fallback.
 * Limits, each refused with ORBFE_ERR_INVALID one step past it, before a device is looked for (pinned by tests/test_gba_cpu.py):
 *   ORBFE_GBA_MAX_KEYFRAMES   2 048 keyframes, free and fixed: the reduced system of 12 288 unknowns is 1.2 GB of workspace
 *   ORBFE_GBA_MAX_POINTS      1 048 575 points: 277 MB of per-point blocks
 *   ORBFE_GBA_MAX_EDGES       8 388 600 edges (eight per point at the point cap): 4.3 GB of per-edge blocks, and every edge index
 *                             times the widest per-edge record stays an int
 *   ORBFE_BA_MAX_ITERATIONS   as above
 * and a constant that is NOT a limit, stated so that tests can stand on its edges:
 *   ORBFE_GBA_TILE_KEYFRAMES  8 row blocks (48 rows) per tile of the factorisation: three tiles of doubles fit the 64 KB of LDS a
 *                             workgroup gets without asking, and 16 x 16 lanes hold 3 x 3 entries each */
#define ORBFE_GBA_MAX_KEYFRAMES 2048
#define ORBFE_GBA_MAX_POINTS 1048575
#define ORBFE_GBA_MAX_EDGES 8388600
#define ORBFE_GBA_TILE_KEYFRAMES 8
/* One problem.  HOST pointers, synchronous, on the calling thread's current device.  Arguments, result record and validation rules
 * as orbfe_bundle_adjustment's (edges in any order, sorted here as there; the same pair twice is refused), against the limits above:
 * any number of the keyframes may be free.  The workspace is allocated for the call.
 * Limits (ORBFE_ERR_INVALID): 0 <= n_kf <= ORBFE_GBA_MAX_KEYFRAMES, 0 <= n_points <= ORBFE_GBA_MAX_POINTS, 0 <= n_edges <=
 * ORBFE_GBA_MAX_EDGES, 1 <= n_iterations <= ORBFE_BA_MAX_ITERATIONS, flags outside ORBFE_BA_ROBUST, every edge's kf and point in
 * range, inv_sigma2 finite and > 0. */
int orbfe_global_bundle_adjustment(const orbfe_pose_camera* camera, const float* poses, const uint8_t* fixed, int n_kf,
                                   const float* points, int n_points, const orbfe_lba_edge* edges, int n_edges, int n_iterations,
                                   int flags, float* poses_out, float* points_out, orbfe_ba_result* result);
/* The workspace of one problem of at most kf_cap keyframes, point_cap points and edge_cap edges.  HOST pointer.
 * Limits (ORBFE_ERR_INVALID): the caps >= 0 and within the ORBFE_GBA_MAX_*, null bytes. */
int orbfe_gba_workspace_bytes(int kf_cap, int point_cap, int edge_cap, size_t* bytes);
/* One problem from arrays in HBM.  DEVICE pointers; SYNCHRONOUS on `stream` (NULL: the NULL stream), see above.  d_points: records
 * of point_stride bytes that start with the position; d_edges: point by point, keyframes ascending, as the batch forms take them;
 * d_result: one record in HBM.  A problem whose edge list breaks that rule, names an index out of range or carries an inv_sigma2
 * that is not finite and > 0 is refused on the device: rounds = -1, poses and points copied through, nothing else written.
 * d_workspace: workspace_bytes >= what orbfe_gba_workspace_bytes states for (n_kf, n_points, n_edges), 256-byte aligned; its
 * contents do not matter and are not kept.  Inputs are not modified.
 * Limits (ORBFE_ERR_INVALID): as orbfe_global_bundle_adjustment, point_stride >= 12 and a multiple of 4, records 4-byte aligned,
 * d_result 8-byte, null pointers (the arrays of a count of 0 may be null). */
int orbfe_global_bundle_adjustment_device(const orbfe_pose_camera* d_camera, const float* d_poses, const uint8_t* d_fixed, int n_kf,
                                          const uint8_t* d_points, int point_stride, int n_points, const orbfe_lba_edge* d_edges,
                                          int n_edges, int n_iterations, int flags, float* d_poses_out, float* d_points_out,
                                          orbfe_ba_result* d_result, void* d_workspace, size_t workspace_bytes, void* stream);
/* Measurement only (tools/gba_rate.py): copies the calling thread's sums of stream-event times per phase, in milliseconds, to ms
 * (7 floats: plan, build, Dinv / Schur, factorisation, solves, update / chi2, control read-back; NULL: not copied), clears them, and
 * switches the timing of this thread's later calls of the two forms above on (enable != 0) or off.  Timing synchronises the stream
 * after every phase: the sums are the phases' device times, and a timed call is slower than an untimed one. */
int orbfe_debug_gba_phases(int enable, float* ms);

/* ---- The map update behind the global bundle adjustment (LoopClosing::RunGlobalBundleAdjustment, L/src/LoopClosing.cc:648-703) ---------
 * What the reference does with mTcwGBA / mPosGBA once the adjustment has finished.  Keyframes: a breadth-first walk of the spanning
 * tree from the map's origins; a keyframe the adjustment did not optimise (local mapping inserted it meanwhile) gets
 * mTcwGBA = (Tcw * parent.Twc) * parent.mTcwGBA, the bracket from the poses before the walk, and every keyframe reached gets
 * SetPose(mTcwGBA) (L/src/KeyFrame.cc:75-88: Twc and the stereo centre Cw with it).  Points: one the adjustment optimised takes its
 * mPosGBA; any other moves with its reference keyframe, Xw' = Rwc_new * (Rcw_before * Xw + tcw_before) + twc_new; a bad point stays.
 * UpdateNormalAndDepth is not part of this block.  The arithmetic is csrc/gba_map_internal.h's reading of cv::Mat (float dots in index
 * order, zeros and ones of a 4 x 4 operand included, double epilogue), bit for bit the numpy reading of tests/np_gba_map.py.
 * On the device a keyframe's pose is a function of its parent's alone, so the walk becomes a rule per keyframe: an optimised one takes
 * its row of gba_poses; another one follows its parent in the round after the parent is done.  Three launches over the keyframes
 * (csrc/gba_map_kernels.hip: Tchildc per keyframe; ONE workgroup that loops rounds behind a barrier until a round makes no progress;
 * SetPose per keyframe) and one thread per point; no workspace, no host read-back, no floating-point atomics (the counts of the
 * result record are integer atomics).  A round of the chain costs 2 us while few keyframes wait and up to 10 us when 65 535 do
 * (profiles/gba_map_update.md): a chain of 64 under a map of 1 048 575 points is 0.14 ms, the worst chain the limit admits 0.5 - 0.7 s.
 * Rules the data decides, the same in both forms:
 *   a keyframe whose chain of parents does not end in an optimised keyframe -- an origin that is not optimised, a cycle, a parent that
 *   is itself unreached -- is ORBFE_GBA_MAP_KF_UNREACHED: its record carries its old pose with that pose's Twc and Cw.  DEVIATION: the
 *   reference reads an empty mTcwGBA there;
 *   a point whose reference keyframe is unreached stays (the reference's `continue`, :688).
 * Non-finite poses are not refused: they go through the arithmetic as it is.
 * Limits, each refused with ORBFE_ERR_INVALID one step past it, before a device is looked for (pinned by tests/test_gba_map_cpu.py):
 *   ORBFE_GBA_MAP_MAX_KEYFRAMES  65 536 keyframes (32 times ORBFE_GBA_MAX_KEYFRAMES: the map keeps growing while the adjustment runs
 *                                and across loops): a lane of the chain's one workgroup of 1 024 keeps its keyframes in one 64-bit
 *                                mask, and the done-marks of all of them are 8 KB of LDS; also the most rows of gba_poses
 *   ORBFE_GBA_MAP_MAX_POINTS     16 777 216 points, the limit of orbfe_sim3_correct_points: the staging block of the host form
 *                                (32 bytes a point in and out, 12 a row of gba_points) stays under 1 GB; also the most rows of
 *                                gba_points */
#define ORBFE_GBA_MAP_MAX_KEYFRAMES 65536
#define ORBFE_GBA_MAP_MAX_POINTS 16777216
#define ORBFE_GBA_MAP_KF_OPTIMISED 0  /* mnBAGlobalForKF == nLoopKF: the row of gba_poses */
#define ORBFE_GBA_MAP_KF_PROPAGATED 1 /* the correction of its parent */
#define ORBFE_GBA_MAP_KF_UNREACHED 2  /* see above: the old pose */
typedef struct orbfe_gba_map_keyframe { /* 112 bytes, 8-byte aligned */
  float Tcw[12];  /* the pose after the update, rows of [R | t] (mTcwGBA; the old pose of an unreached keyframe) */
  float Twc[12];  /* SetPose's inverse of it, rows of [Rwc | Ow] */
  float Cw[3];    /* SetPose's stereo centre */
  int32_t status; /* ORBFE_GBA_MAP_KF_* */
} orbfe_gba_map_keyframe;
typedef struct orbfe_gba_map_result { /* 32 bytes */
  int32_t n_optimised, n_propagated, n_unreached; /* keyframes per status */
  int32_t n_taken, n_moved, n_left;               /* points that took gba_points, moved with their keyframe, stayed */
  int32_t rounds;                                 /* propagation rounds that made progress: the longest chain of propagated keyframes */
  int32_t reserved;
} orbfe_gba_map_result;
/* HOST pointers, synchronous, on the calling thread's current device: one upload, the launches, one download.
 * poses[n_kf][12]: the current Tcw, rows of [R | t] as orbfe_global_bundle_adjustment takes them; parent[n_kf]: the row of the
 * spanning-tree parent, -1 for an origin; kf_gba_row[n_kf]: >= 0 for an optimised keyframe, its row of gba_poses[n_gba_kf][12], -1
 * for one that is not; half_baseline: mHalfBaseline, one value for the map.  points[n_points][3]; point_gba_row[n_points]: >= 0 takes
 * that row of gba_points[n_gba_points][3]; ref[n_points]: the row of the reference keyframe, -1 for a point that stays (a bad one);
 * point_gba_row wins over ref.  kf_out[n_kf], points_out[n_points][3], one result record.  Inputs are not modified.
 * Limits (ORBFE_ERR_INVALID): 0 <= n_kf, n_gba_kf <= ORBFE_GBA_MAP_MAX_KEYFRAMES; 0 <= n_points, n_gba_points <=
 * ORBFE_GBA_MAP_MAX_POINTS; parent and ref in -1 .. n_kf - 1, kf_gba_row in -1 .. n_gba_kf - 1, point_gba_row in -1 .. n_gba_points - 1;
 * null arrays with a count > 0, null result; kf_out 8-byte, every other array 4-byte aligned; an output that is an input
 * or another output. */
int orbfe_gba_update_map(const float* poses, const int32_t* parent, const int32_t* kf_gba_row, int n_kf, const float* gba_poses,
                         int n_gba_kf, float half_baseline, const float* points, const int32_t* point_gba_row, const int32_t* ref,
                         int n_points, const float* gba_points, int n_gba_points, orbfe_gba_map_keyframe* kf_out, float* points_out,
                         orbfe_gba_map_result* result);
/* The same on DEVICE pointers, asynchronous on `stream` (NULL: the NULL stream): d_gba_poses / d_gba_points may be the d_poses_out /
 * d_points_out of orbfe_global_bundle_adjustment_device, so the chain needs no copy.  d_points: records of point_stride bytes that
 * start with the position.  A parent, ref or row the host cannot check is never read out of bounds: a parent or ref outside
 * 0 .. n_kf - 1 is no parent / no reference keyframe, a kf_gba_row >= n_gba_kf makes the keyframe unreached, a point_gba_row >=
 * n_gba_points makes the point stay; every negative row reads as -1.
 * Limits (ORBFE_ERR_INVALID): the counts, the null pointers, the alignment and the aliasing as above; point_stride >= 12 and a
 * multiple of 4. */
int orbfe_gba_update_map_device(const float* d_poses, const int32_t* d_parent, const int32_t* d_kf_gba_row, int n_kf,
                                const float* d_gba_poses, int n_gba_kf, float half_baseline, const uint8_t* d_points, int point_stride,
                                const int32_t* d_point_gba_row, const int32_t* d_ref, int n_points, const float* d_gba_points,
                                int n_gba_points, orbfe_gba_map_keyframe* d_kf_out, float* d_points_out, orbfe_gba_map_result* d_result,
                                void* stream);

/* ---- KeyFrameDatabase (L/src/KeyFrameDatabase.cc, D/src/ScoringObject.cpp: L1) -----------------------------------------------------
 * The first step of both place-recognition chains: DetectRelocalizationCandidates in front of orbfe_search_by_bow .. the pose
 * optimisation, DetectLoopCandidates in front of orbfe_search_by_bow_kf .. orbfe_optimize_sim3.  The handle keeps the BoW vectors
 * orbfe_compute_bow produced (word ids and double values) in device memory and answers Q queries per call against every entry.
 * Every output is decided bit for bit by a plain reading of the reference; no tolerance applies anywhere:
 *   entries      add appends the keyframe to the list of each of its words, so an entry has an add sequence number: its SLOT.  Slots
 *                are handed out in add order and are not reused before clear; erase frees the entry, adding the id again takes a new,
 *                later slot.
 *   sharing set  S of a query = the live entries with at least one common word (for a loop query: whose id is not in the query's
 *                connected set); an entry's `words` = the number of common words; lKFsSharingWords = S ordered by (smallest common
 *                word id, slot)
 *   thresholds   maxCommonWords = max words over S; minCommonWords = (int)(maxCommonWords * 0.8f); an entry is SCORED when
 *                words > minCommonWords; si = (float)(-sum / 2.0), sum += fabs(vi - wi) - fabs(vi) - fabs(wi) over the common words
 *                in ascending word order, in double (vi the query's value)
 *   relocalisation   every scored entry, in S order, starts acc = best = si and walks its at most 10 covisible neighbours in their
 *                given order: a neighbour IN S adds its mRelocScore in float (being scored is not required) and replaces the best
 *                keyframe when its score is strictly larger; bestAccScore starts at 0; an entry is retained when acc > 0.75f *
 *                bestAccScore; the candidates are the best keyframes of the retained entries, in order, first occurrence only.
 *                mRelocScore of a neighbour that is in S but not scored is what the most recent earlier query that scored it left
 *                there; the reference never initialises the field.  The handle carries it per slot, starts it at 0.0f on add (the
 *                one deviation) and applies the queries of a batch in index order.
 *   loop         scored entries with si >= minScore form lScoreAndMatch; a neighbour counts only when it is in S and scored, so no
 *                state crosses queries; bestAccScore starts at minScore; the rest as above
 *   neighbours   an id that names no live entry at query time is skipped
 * Limits (ORBFE_ERR_INVALID unless stated): */
#define ORBFE_KFDB_MAX_WORDS 4096        /* words of one vector, entry or query: a workgroup stages a query's ids and values in 48 KiB
                                            of LDS.  A frame of 2 000 features has at most 2 000 words. */
#define ORBFE_KFDB_NEIGHBOURS 10         /* GetBestCovisibilityKeyFrames(10), L/src/KeyFrameDatabase.cc:149, :262 */
#define ORBFE_KFDB_MAX_QUERIES 65535     /* queries per call: grid.y */
#define ORBFE_KFDB_MAX_SLOTS 4194304     /* adds between two clears (ORBFE_ERR_CAPACITY): slot indices and strip counts stay far inside
                                            int32 */
#define ORBFE_KFDB_MAX_CELLS 67108864    /* Q x slots and Q x cand_cap of one call (ORBFE_ERR_CAPACITY): the work space is ten 4-byte
                                            arrays of Q x slots, 2.5 GiB at this limit */
#define ORBFE_KFDB_SCORE_UNKNOWN (-1.0f) /* orbfe_kfdb_score of an id that is not in the database; L1 scores lie in [0, 1] */
enum { ORBFE_KFDB_L1_NORM = 0, ORBFE_KFDB_L2_NORM, ORBFE_KFDB_CHI_SQUARE, ORBFE_KFDB_KL, ORBFE_KFDB_BHATTACHARYYA,
       ORBFE_KFDB_DOT_PRODUCT };   /* DBoW2::ScoringType; only L1_NORM, ORBvoc's, is accepted */
typedef struct orbfe_kfdb orbfe_kfdb;
typedef struct orbfe_kfdb_query_info {
  int32_t n_sharing;           /* |S| */
  int32_t max_common_words, min_common_words;
  int32_t n_scored;            /* nscores */
  int32_t n_matches;           /* lScoreAndMatch.size() */
  float best_acc_score;        /* bestAccScore; 0 when the function returned before the accumulation */
  float min_score_to_retain;   /* 0.75f * bestAccScore; 0 likewise */
  int32_t n_candidates;
} orbfe_kfdb_query_info;       /* 32 bytes */
/* device < 0: the current device.  Without a device: ORBFE_ERR_NO_DEVICE (there is no CPU fallback). */
int orbfe_kfdb_create(int n_words, int scoring, int device, orbfe_kfdb** out);
int orbfe_kfdb_destroy(orbfe_kfdb* db);
int orbfe_kfdb_clear(orbfe_kfdb* db);   /* entries, covisibility rows and carried scores; slots start at 0 again */
int orbfe_kfdb_size(const orbfe_kfdb* db, int* n_live, int* n_slots);
/* the keyframe id of every slot, -1 where erased: the first min(n_slots, cap) are written */
int orbfe_kfdb_slots(const orbfe_kfdb* db, int64_t* kf_ids, int cap, int* n_slots);
/* ids ascend strictly and lie in [0, n_words), values are finite and positive, 0 <= n <= ORBFE_KFDB_MAX_WORDS, kf_id >= 0; an id
 * that is live already is ORBFE_ERR_INVALID.  Synchronous. */
int orbfe_kfdb_add(orbfe_kfdb* db, int64_t kf_id, const int32_t* bow_ids, const double* bow_vals, int n);
int orbfe_kfdb_erase(orbfe_kfdb* db, int64_t kf_id);   /* an unknown id is not an error, as in the reference */
/* GetBestCovisibilityKeyFrames(10) of n_rows keyframes, in its order, rows padded with -1.  Rows are kept by keyframe id until clear
 * (a keyframe may get its row before it is added and keeps it across erase and add); they are resolved to live entries at the next
 * query. */
int orbfe_kfdb_set_covisibles(orbfe_kfdb* db, int n_rows, const int64_t* kf_ids, const int64_t* neigh /* [n_rows][10] */);
/* Vocabulary::score of one vector against m listed entries (the minScore loop of LoopClosing::DetectLoop, L/src/LoopClosing.cc:
 * 112-133); out[k] = ORBFE_KFDB_SCORE_UNKNOWN where kf_ids[k] is not live.  HOST pointers, synchronous. */
int orbfe_kfdb_score(orbfe_kfdb* db, const int32_t* q_ids, const double* q_vals, int n, const int64_t* kf_ids, int m, float* out);
/* Q queries as a CSR (q_offsets[0] == 0, each vector as for add).  HOST pointers; one packed upload, one packed download, one
 * synchronisation.  n_cand[q] is the full count; the first min(n_cand[q], cand_cap) ids of row q of cand[Q][cand_cap] are written,
 * nothing behind them.  Optional (NULL): info[Q]; common_words[Q][n_slots] and scores[Q][n_slots], written where the slot was
 * scored and untouched elsewhere (orbfe_kfdb_slots names the slots).  Relocalisation queries update the carried scores in index
 * order; loop queries change nothing.  min_score is finite and not negative; the connected ids of a query ascend strictly. */
int orbfe_kfdb_detect_relocalization(orbfe_kfdb* db, int Q, const int32_t* q_offsets, const int32_t* q_ids, const double* q_vals,
                                     int cand_cap, int64_t* cand, int32_t* n_cand, orbfe_kfdb_query_info* info, int32_t* common_words,
                                     float* scores);
int orbfe_kfdb_detect_loop(orbfe_kfdb* db, int Q, const int32_t* q_offsets, const int32_t* q_ids, const double* q_vals,
                           const float* min_score, const int32_t* conn_offsets, const int64_t* conn_ids, int cand_cap, int64_t* cand,
                           int32_t* n_cand, orbfe_kfdb_query_info* info, int32_t* common_words, float* scores);
/* The same with DEVICE pointers, asynchronous on `stream` (NULL: the NULL stream).  The vectors are not validated: lengths are clamped
 * to [0, ORBFE_KFDB_MAX_WORDS], a list that does not ascend finds fewer common words, nothing outside the stated arrays is read or
 * written.  Rows behind the counts are neither read nor written.  A query's bytes do not depend on Q or on its position in the
 * batch, except through the carried relocalisation scores as defined above.  The handle's work space serves one call at a time:
 * calls on one stream order themselves; synchronise the stream before any other call on the handle.  When entries or rows changed
 * since the last query, the call first uploads the resolved neighbour rows with a blocking copy. */
int orbfe_kfdb_detect_relocalization_device(orbfe_kfdb* db, int Q, const int32_t* d_q_offsets, const int32_t* d_q_ids,
                                            const double* d_q_vals, int cand_cap, int64_t* d_cand, int32_t* d_n_cand,
                                            orbfe_kfdb_query_info* d_info, int32_t* d_common_words, float* d_scores, void* stream);
int orbfe_kfdb_detect_loop_device(orbfe_kfdb* db, int Q, const int32_t* d_q_offsets, const int32_t* d_q_ids, const double* d_q_vals,
                                  const float* d_min_score, const int32_t* d_conn_offsets, const int64_t* d_conn_ids, int cand_cap,
                                  int64_t* d_cand, int32_t* d_n_cand, orbfe_kfdb_query_info* d_info, int32_t* d_common_words,
                                  float* d_scores, void* stream);
/* A/B knob of tools/kfdb_rate.py: how the detection calls that FOLLOW arrange their passes.  0 (default): the common pass counts, a
 * score pass sums the scored pairs alone.  1: the common pass also forms the L1 sum of every pair with a common word, in the same
 * order, and the score pass only copies.  Results do not depend on it (tests/test_kfdb_gpu.py); profiles/keyframe_database.md has
 * the times. */
int orbfe_debug_kfdb_arrangement(int arrangement);

/* ---- MapPoint::ComputeDistinctiveDescriptors (L/src/MapPoint.cc:229-320) and MapPoint::UpdateNormalAndDepth (:340-381) ---------------
 * The two calls that end every step which creates, fuses or moves map points (L/src/LocalMapping.cc:137-138, :413-415, :501-502,
 * L/src/Optimizer.cc:759, L/src/LoopClosing.cc:474, :504, L/src/Tracking.cc:473-474, :599-600, :1010-1011), for P points in one launch
 * sequence.  A point is an ORDERED list of observations (keyframe, keypoint index) plus a position; the order is the iteration order
 * of the reference's std::map<KeyFrame*, size_t>, and the caller states it.  Given the list every output is decided bit for bit by a
 * plain reading (csrc/mappoint_internal.h); no tolerance applies anywhere:
 *   descriptor   live = the observations whose keyframe is not bad, in list order, N = |live|.  N == 0: nothing is chosen (best = -1,
 *                desc zero).  Otherwise row i holds the N Hamming distances (0 .. 256) from live descriptor i to every live descriptor,
 *                its own 0 included; median_i = the element (int)(0.5 * (N - 1)) of the sorted row (the floor); the winner is the first
 *                i with the least median (strict <), so N = 1 and N = 2 always give the first live observation.  best is the winner's
 *                position in the CALLER's list, desc its 32 bytes, n_live = N.
 *   normal, depth   over ALL n_obs observations (the reference does not read isBad() here): d = pos - Ow in float, r = (float)(1.0 /
 *                sqrt(sum of (double)d * (double)d in element order)), sum = sum + d * r in float in LIST ORDER from 0.0f, normal =
 *                sum * (float)(1.0 / (double)n_obs); with PC = pos - Ow[ref]: dist = (float)sqrt(sum (double)PC^2), max_distance =
 *                dist * scale_factors[ref_octave], min_distance = max_distance / scale_factors[n_levels - 1].  For two observations
 *                these are the bytes orbfe_triangulate_matches writes for the pair.
 * Taken over: both functions' arithmetic and skips.  Not taken over: the locks (the caller marshals under them), and the pointer
 * order of the std::map, which is an input here.  An observation at zero distance from the point follows IEEE as the reference does.
 * A point is refused by its own wave or workgroup -- status = ORBFE_MP_REFUSED, best = -1, every other selected output zero, no other
 * point touched -- when n_obs is negative or beyond ORBFE_MP_MAX_OBS, its observations do not lie inside the observation array, an
 * observation names a keyframe outside the table or a keypoint outside that keyframe (or a descriptor block that is not 4-byte
 * aligned), ref is not in [0, n_obs) or ref_octave not in [0, n_levels).  n_obs == 0 (an empty or bad point): ORBFE_MP_UNCHANGED, the
 * same outputs.  Deterministic: integer arithmetic and one sequential float sum per point, no floating-point atomics; a point's bytes
 * do not depend on P, on its position in the batch or on the run.  No CPU fallback.
 * Limits, each refused with ORBFE_ERR_INVALID one step past it, before any device call (pinned by tests/test_mappoint_cpu.py):
 *   ORBFE_MP_MAX_OBS         1 024 observations of one point: its descriptors are staged in 32 KiB of LDS; the reference's own
 *                            `float Distances[N][N]` leaves an 8 MiB stack at N = 1 448
 *   ORBFE_MP_MAX_POINTS      1 048 576 points per call: 64 MiB of update records; point indices and grid sizes stay far inside int32
 *   ORBFE_MP_MAX_TOTAL_OBS   16 777 216 observations per call: the host form stages 40 bytes for each (640 MiB)
 *   ORBFE_MP_MAX_KEYFRAMES   1 048 576 rows of the keyframe table (32 MiB) */
#define ORBFE_MP_MAX_OBS 1024
#define ORBFE_MP_MAX_POINTS 1048576
#define ORBFE_MP_MAX_TOTAL_OBS 16777216
#define ORBFE_MP_MAX_KEYFRAMES 1048576
#define ORBFE_MP_DESCRIPTOR 1             /* flags: best, n_live, desc are computed and written */
#define ORBFE_MP_NORMAL_DEPTH 2           /* flags: normal, min_distance, max_distance are; what a flag does not select is not touched */
enum { ORBFE_MP_UPDATED = 0, ORBFE_MP_UNCHANGED = 1, ORBFE_MP_REFUSED = 2 };   /* orbfe_mp_update.status, always written */
typedef struct orbfe_mp_keyframe {        /* one row of the keyframe table; 32 bytes, 8-byte aligned */
  uint64_t desc;                          /* address of mDescriptors, n_keys x 32 bytes: DEVICE memory for the device form, HOST for the host form */
  int32_t n_keys;                         /* rows of it */
  int32_t bad;                            /* isBad() */
  float Ow[3];                            /* GetCameraCenter() */
  int32_t reserved;
} orbfe_mp_keyframe;
typedef struct orbfe_mp_obs {             /* 8 bytes */
  int32_t kf, idx;                        /* row of the keyframe table, keypoint index in that keyframe */
} orbfe_mp_obs;
typedef struct orbfe_mp_point {           /* 16 bytes */
  int32_t obs_offset, n_obs;              /* its observations in the observation array, in map order */
  int32_t ref;                            /* position of mpRefKF in its list */
  int32_t ref_octave;                     /* mvKeysUn[observations[pRefKF]].octave */
} orbfe_mp_point;
typedef struct orbfe_mp_update {          /* 64 bytes */
  float normal[3];                        /* mNormalVector */
  float min_distance, max_distance;       /* mfMinDistance, mfMaxDistance */
  int32_t best;                           /* position in the caller's list of the chosen descriptor, -1: none */
  int32_t n_live;
  int32_t status;                         /* ORBFE_MP_* */
  uint8_t desc[32];                       /* mDescriptor */
} orbfe_mp_update;
/* P points.  HOST pointers, synchronous, on the calling thread's current device.  positions: P x 3 floats (GetWorldPos);
 * scale_factors: n_levels floats (mvScaleFactors).  Only the descriptor rows some observation names are staged: one upload, the
 * launches, one download.  In updates[p] the status and the halves `flags` selects are written.
 * Limits (ORBFE_ERR_INVALID): the ORBFE_MP_MAX_* above (a point's n_obs beyond ORBFE_MP_MAX_OBS included), P, n_kf, n_obs_total >= 0,
 * 1 <= n_levels <= ORBFE_MAX_LEVELS, flags a non-empty subset of the two, null arrays with a count > 0, null scale_factors, a keyframe
 * with n_keys < 0 or with n_keys > 0 and no descriptors while ORBFE_MP_DESCRIPTOR is set. */
int orbfe_refresh_map_points(const orbfe_mp_keyframe* keyframes, int n_kf, const orbfe_mp_obs* obs, int n_obs_total,
                             const orbfe_mp_point* points, const float* positions, int P, const float* scale_factors, int n_levels,
                             int flags, orbfe_mp_update* updates);
/* The same with DEVICE pointers (scale_factors stays a HOST pointer, read before the call returns), asynchronous on `stream` (NULL:
 * the NULL stream).  The keyframes' descriptor blocks are resident in device memory.  Point p's position is the first three floats of
 * the record at d_points_pos + p * point_stride (orbfe_map_point: 72, orbfe_kf_point: 72, orbfe_new_point: 44, or 12 for bare
 * positions).  Nothing outside the stated arrays is read or written; inputs are not modified.
 * Limits (ORBFE_ERR_INVALID): as above, except that a point's n_obs is checked on the device; point_stride >= 12 and a multiple of 4;
 * null pointers with a count > 0; records not 4-byte (the keyframe table: 8-byte) aligned. */
int orbfe_refresh_map_points_batch_device(int P, const orbfe_mp_keyframe* d_keyframes, int n_kf, const orbfe_mp_obs* d_obs,
                                          int n_obs_total, const orbfe_mp_point* d_points, const void* d_points_pos, int point_stride,
                                          const float* scale_factors, int n_levels, int flags, orbfe_mp_update* d_updates, void* stream);

/* ---- The covisibility graph: KeyFrame::UpdateConnections (L/src/KeyFrame.cc:268-354), the vote of Tracking::UpdateLocalKeyFrames
 * (L/src/Tracking.cc:1115-1159) and LocalMapping::KeyFrameCulling (L/src/LocalMapping.cc:595-655) ---------------------------------------
 * Both operations read the tables of orbfe_refresh_map_points*: the observation array orbfe_mp_obs[] and, of orbfe_mp_point, obs_offset
 * and n_obs (ref and ref_octave are not read).  Beside them: point_bad[p] (one byte per point, MapPoint::isBad()), and per keyframe ROW
 * of the table kf_order[row] and kf_bad[row] (KeyFrame::isBad()).  kf_order is the row's position in the iteration order of the
 * reference's std::map<KeyFrame*, ...> over the table's keyframes: the caller sorts the pointers and states the positions, which are
 * DISTINCT values in [0, n_kf).  With that order an input, every output is decided to the bit by a plain reading
 * (csrc/covis_internal.h); no tolerance applies.
 *
 * 1. Counts.  A subject is a slice of the slot array (int32 point indices, -1 = an empty slot: mvpMapPoints of a keyframe or of a
 *    frame), a keyframe row `self` or -1, and a mode.  Every non-empty slot whose point is not bad adds 1 to the counter of each
 *    keyframe row in that point's observation list, except the row `self`.  The reference compares mnId (:295); the rows of the table
 *    are distinct keyframes, so row equality is the same test.  Per subject one orbfe_cov_header and up to conn_cap orbfe_cov_entry
 *    (kf, weight) at entries[s * conn_cap ..]:
 *      ORBFE_COV_CONNECTIONS  all n_counted rows with a counter > 0 (mConnectedKeyFrameWeights), sorted by weight descending and among
 *                 equal weights by kf_order descending: sort(vPairs) on pair<int, KeyFrame*> followed by push_front (:332-338).
 *                 n_ordered = the entries with weight >= 15, which are the first n_ordered of the list and the reference's
 *                 mvpOrderedConnectedKeyFrames / mvOrderedWeights.  kf_max / w_max: the first row in ascending kf_order that holds the
 *                 strict maximum (:317-320).  n_ordered == 0 with n_counted > 0: the reference's ordered list is the one pair (kf_max,
 *                 w_max); header.single = 1 says so and the entry list stays the full counter.  n_counted == 0: status EMPTY (the
 *                 early return :302-303).
 *      ORBFE_COV_VOTES  `self` is not read.  The entries are the counted rows whose keyframe is not bad, in ascending kf_order: the order
 *                 in which mvpLocalKeyFrames is filled (Tracking.cc:1144-1159).  n_ordered = their number; kf_max / w_max the first
 *                 strict maximum among them (-1 / 0 when there is none); n_counted counts the bad rows too and n_counted == 0 is EMPTY.
 *    Status: OK; EMPTY; OVERFLOW -- more than conn_cap entries exist: the header is exact, the first conn_cap entries of the stated
 *    order are written and nothing beyond them is touched; REFUSED -- decided by the subject's own workgroup, header zero but for the
 *    status and kf_max = -1, no entry written, no other subject touched: an unknown mode, a slice outside the slot array, self outside
 *    [-1, n_kf) (CONNECTIONS), a slot < -1 or >= n_points, a good point whose list lies outside the observation array, an observation
 *    whose kf is outside [0, n_kf), or a kf_order outside [0, n_kf) on an observed row.  Entries behind n_written are never written.
 *    With the caller stay: the reciprocal AddConnection calls, UpdateBestCovisibles of the other keyframes, the spanning-tree parent,
 *    the neighbour / child / parent expansion of UpdateLocalKeyFrames up to 80 keyframes (or orbfe_local_map* below, which takes it
 *    and UpdateLocalPoints to the device), and clearing bad points out of the frame;
 *    csrc/host/Covisibility_hip.h replays them in the reference's order.
 *
 * 2. Keyframe culling, one problem per current keyframe: an ordered list of DISTINCT local keyframe rows
 *    (GetVectorCovisibleKeyFrames()) and `monocular`.  Each point also carries n_obs_weighted = MapPoint::Observations() (a stereo
 *    observation counts 2, so it is not the list length).  :603-654 read literally, with the sequential side effects: rows flagged
 *    IS_ID0 are skipped; for every other row the slots are walked: an empty slot or a bad point is passed over; unless monocular the
 *    slot is passed over when `depth > th_depth || depth < 0` (float); nMPs++; if Observations() > 3 the observations of the point in
 *    OTHER rows with `octave_i <= octave + 1` are counted up to 3, and 3 make the slot redundant.  The row is redundant when
 *    `nRedundant > 0.9 * nMPs` in double.  A redundant row without NOT_ERASE is CULLED before the next row is examined
 *    (KeyFrame::SetBadFlag :416-434): each point that holds an observation of it loses that observation, its Observations() drops by 2
 *    if the culled row's mvuRight[idx] >= 0 and by 1 otherwise, and it becomes bad when the result is <= 2
 *    (MapPoint::EraseObservation, L/src/MapPoint.cc:112-136).  A redundant row with NOT_ERASE is MARKED and changes nothing.
 *    No input is modified: with the set of rows culled so far, removed = the sum of 1 or 2 over a point's observations of culled rows,
 *    Observations() = n_obs_weighted - removed, bad = bad_in || (removed > 0 && n_obs_weighted - removed <= 2), and observations of
 *    culled rows are passed over; tests/np_covis.py states both readings and shows them equal.
 *    Stated input domain: slot i of row k holds point p exactly when the list of p holds (k, i); bad points have empty lists; the
 *    local rows of a problem are distinct.  Outside it only memory safety is promised.  A row is REFUSED (n_mps = n_redundant = 0,
 *    nothing culled) when it lies outside the table, has n_keys < 0, lacks the slot or keypoint array with n_keys > 0 or the depth
 *    array when not monocular, or one of its slots names a point, a list, a keyframe row or a keypoint index outside its table.  A null
 *    u_right reads as -1 everywhere (a monocular keyframe).  A problem whose local range lies outside the local array writes nothing.
 *
 * Deterministic: integer LDS atomics only, whose order does not reach the result; the output order comes from the sort keys alone;
 * a subject's or problem's bytes do not depend on S or Q, on its position in the batch or on the run.  No CPU fallback.
 * Limits, each refused with ORBFE_ERR_INVALID one step past it, before any device call (pinned by tests/test_covis_cpu.py):
 *   ORBFE_COV_MAX_KEYFRAMES    32 768 rows of the keyframe table: the counters are 32-bit words in LDS, 128 KiB of the 160 KiB; the
 *                              culled set is one bit per row, 4 KiB
 *   ORBFE_COV_MAX_CONN         conn_cap 1 .. 2 048: the entries are ordered in LDS beside the counters, 12 bytes each (24 KiB)
 *   ORBFE_COV_MAX_POINTS       1 048 576 points and
 *   ORBFE_COV_MAX_TOTAL_OBS    16 777 216 observations per call: the limits of the tables orbfe_refresh_map_points* defines
 *   ORBFE_COV_MAX_TOTAL_SLOTS  16 777 216 slots per call (64 MiB of indices; offsets stay far inside int32)
 *   ORBFE_COV_MAX_SUBJECTS     65 535 subjects and
 *   ORBFE_COV_MAX_PROBLEMS     65 535 problems per launch: one workgroup each, the grid limit the other batch forms use
 *   ORBFE_COV_MAX_TOTAL_LOCAL  1 048 576 local keyframes over all problems of a call (16 MiB of verdicts)
 *   ORBFE_COV_MAX_KEYS         65 535 keypoints per keyframe (host form; the descriptor limit of the searches that fill the slots)
 *   ORBFE_COV_MAX_TOTAL_KEYS   4 194 304 keypoints over all rows of the table (host culling form: it stages 40 bytes for each, 160 MiB;
 *                              2 048 keyframes of 2 048 keypoints)
 *   ORBFE_COV_MAX_TOTAL_ENTRIES  S x conn_cap <= 4 194 304 (host counting form: the entry block, 32 MiB, comes back in one copy) */
#define ORBFE_COV_MAX_KEYFRAMES 32768
#define ORBFE_COV_MAX_CONN 2048
#define ORBFE_COV_MAX_POINTS 1048576
#define ORBFE_COV_MAX_TOTAL_OBS 16777216
#define ORBFE_COV_MAX_TOTAL_SLOTS 16777216
#define ORBFE_COV_MAX_SUBJECTS 65535
#define ORBFE_COV_MAX_PROBLEMS 65535
#define ORBFE_COV_MAX_TOTAL_LOCAL 1048576
#define ORBFE_COV_MAX_KEYS 65535
#define ORBFE_COV_MAX_TOTAL_KEYS 4194304
#define ORBFE_COV_MAX_TOTAL_ENTRIES 4194304
#define ORBFE_COV_TH 15                   /* `int th = 15`, KeyFrame.cc:310 */
enum { ORBFE_COV_CONNECTIONS = 0, ORBFE_COV_VOTES = 1 };                                               /* orbfe_cov_subject.mode */
enum { ORBFE_COV_OK = 0, ORBFE_COV_EMPTY = 1, ORBFE_COV_OVERFLOW = 2, ORBFE_COV_REFUSED = 3 };         /* orbfe_cov_header.status */
enum { ORBFE_COV_KEPT = 0, ORBFE_COV_CULLED = 1, ORBFE_COV_MARKED = 2, ORBFE_COV_SKIPPED_ID0 = 3, ORBFE_COV_ROW_REFUSED = 4 };   /* verdict */
#define ORBFE_COV_IS_ID0 1                /* orbfe_cov_keyframe.flags: mnId == 0 */
#define ORBFE_COV_NOT_ERASE 2             /* mbNotErase */
typedef struct orbfe_cov_subject {        /* 16 bytes */
  int32_t slot_offset, n_slots;           /* its slice of the slot array */
  int32_t self;                           /* its own keyframe row, or -1 (a frame) */
  int32_t mode;                           /* ORBFE_COV_CONNECTIONS or ORBFE_COV_VOTES */
} orbfe_cov_subject;
typedef struct orbfe_cov_header {         /* 32 bytes */
  int32_t n_counted;                      /* rows with a counter > 0 */
  int32_t n_ordered;                      /* CONNECTIONS: entries with weight >= 15; VOTES: entries (keyframe not bad) */
  int32_t kf_max, w_max;                  /* pKFmax, nmax; -1, 0 when nothing is eligible */
  int32_t status;                         /* ORBFE_COV_OK .. ORBFE_COV_REFUSED */
  int32_t n_written;                      /* entries written: min(entries that exist, conn_cap) */
  int32_t single;                         /* CONNECTIONS, n_ordered == 0 < n_counted: the ordered list is the pair (kf_max, w_max) */
  int32_t reserved;                       /* 0 */
} orbfe_cov_header;
typedef struct orbfe_cov_entry {          /* 8 bytes */
  int32_t kf, weight;                     /* row of the keyframe table, its counter */
} orbfe_cov_entry;
typedef struct orbfe_cov_keyframe {       /* one row of the culling table; 48 bytes, 8-byte aligned */
  uint64_t keys_un;                       /* address of mvKeysUn, n_keys orbfe_keypoint (only octave is read) */
  uint64_t u_right;                       /* address of mvuRight, n_keys floats; 0: every value reads as -1 */
  uint64_t depth;                         /* address of mvDepth, n_keys floats; 0 is accepted only when monocular */
  uint64_t slots;                         /* address of n_keys int32: the point index of mvpMapPoints[i], or -1 */
  int32_t n_keys;                         /* DEVICE addresses for the device form, HOST addresses for the host form */
  float th_depth;                         /* mThDepth */
  int32_t flags;                          /* ORBFE_COV_IS_ID0 | ORBFE_COV_NOT_ERASE */
  int32_t reserved;
} orbfe_cov_keyframe;
typedef struct orbfe_cov_problem {        /* 16 bytes */
  int32_t local_offset, n_local;          /* its rows in the local array, in GetVectorCovisibleKeyFrames() order */
  int32_t monocular;                      /* mbMonocular */
  int32_t reserved;
} orbfe_cov_problem;
typedef struct orbfe_cov_verdict {        /* 16 bytes, one per element of the local array */
  int32_t n_mps, n_redundant;             /* nMPs, nRedundantObservations */
  int32_t verdict;                        /* ORBFE_COV_KEPT .. ORBFE_COV_ROW_REFUSED */
  int32_t reserved;                       /* 0 */
} orbfe_cov_verdict;
/* S subjects.  HOST pointers, synchronous, on the calling thread's current device: one upload, one launch, one download.  headers: S
 * records, all written; entries: S x conn_cap records, of which the first headers[s].n_written of each subject are written.
 * Limits (ORBFE_ERR_INVALID): the ORBFE_COV_MAX_* above, every count >= 0, 1 <= conn_cap <= ORBFE_COV_MAX_CONN, null arrays with a
 * count > 0, S x conn_cap <= ORBFE_COV_MAX_TOTAL_ENTRIES.  S == 0: nothing is launched and nothing behind a pointer is read. */
int orbfe_covis_count(const orbfe_mp_obs* obs, int n_obs_total, const orbfe_mp_point* points, const uint8_t* point_bad, int n_points,
                      const int32_t* kf_order, const uint8_t* kf_bad, int n_kf, const int32_t* slots, int n_slots_total,
                      const orbfe_cov_subject* subjects, int S, int conn_cap, orbfe_cov_header* headers, orbfe_cov_entry* entries);
/* The same with DEVICE pointers, asynchronous on `stream` (NULL: the NULL stream), S subjects in one launch.  Nothing outside the
 * stated arrays is read or written; inputs are not modified.  Limits: as above; records not 4-byte aligned. */
int orbfe_covis_count_batch_device(int S, const orbfe_mp_obs* d_obs, int n_obs_total, const orbfe_mp_point* d_points,
                                   const uint8_t* d_point_bad, int n_points, const int32_t* d_kf_order, const uint8_t* d_kf_bad, int n_kf,
                                   const int32_t* d_slots, int n_slots_total, const orbfe_cov_subject* d_subjects, int conn_cap,
                                   orbfe_cov_header* d_headers, orbfe_cov_entry* d_entries, void* stream);
/* Q culling problems.  HOST pointers (the table's addresses too: every keyframe's four arrays are staged with the tables), synchronous:
 * one upload, one launch, one download.  verdicts: n_local_total records, one per element of `local`; those of a problem's range
 * are written.  A row's slot array is needed only when a problem lists the row; without it that row is REFUSED.
 * Limits (ORBFE_ERR_INVALID): the ORBFE_COV_MAX_* above; every count >= 0; null arrays with a count > 0; a row with n_keys outside
 * 0 .. ORBFE_COV_MAX_KEYS, or with n_keys > 0 and no keypoint array; the n_keys of all rows summing to more than
 * ORBFE_COV_MAX_TOTAL_KEYS; a problem whose range lies outside the local array.  Q == 0: nothing is launched and nothing behind a
 * pointer is read. */
int orbfe_covis_cull_keyframes(const orbfe_mp_obs* obs, int n_obs_total, const orbfe_mp_point* points, const uint8_t* point_bad,
                               const int32_t* n_obs_weighted, int n_points, const orbfe_cov_keyframe* keyframes, int n_kf,
                               const int32_t* local, int n_local_total, const orbfe_cov_problem* problems, int Q,
                               orbfe_cov_verdict* verdicts);
/* The same with DEVICE pointers and device addresses in the table, asynchronous on `stream`, Q problems in one launch.  Limits: as
 * above except what lies behind a pointer, which the device checks; records not 4-byte (the keyframe table: 8-byte) aligned. */
int orbfe_covis_cull_keyframes_batch_device(int Q, const orbfe_mp_obs* d_obs, int n_obs_total, const orbfe_mp_point* d_points,
                                            const uint8_t* d_point_bad, const int32_t* d_n_obs_weighted, int n_points,
                                            const orbfe_cov_keyframe* d_keyframes, int n_kf, const int32_t* d_local, int n_local_total,
                                            const orbfe_cov_problem* d_problems, orbfe_cov_verdict* d_verdicts, void* stream);

/* ---- The local map of a tracked frame: Tracking::UpdateLocalKeyFrames behind its vote (L/src/Tracking.cc:1161-1214),
 * Tracking::UpdateLocalPoints (:1090-1113) and the skip flag of Tracking::SearchLocalPoints (:1036-1049, :1057-1060) ----------------------
 * One frame is one subject of the vote (mode ORBFE_COV_VOTES): the call consumes the vote's headers and entries exactly as
 * orbfe_covis_count* left them (conn_cap included) and reads, beside the tables the vote read (kf_bad, point_bad, the slot array and
 * the frame's orbfe_cov_subject), one orbfe_lm_graph row per keyframe row, the children array, and of the orbfe_cov_keyframe table
 * `slots` and `n_keys` alone.  Per frame, read literally (csrc/localmap_internal.h states it once):
 *   Expansion.  The list starts as the vote's entries, all marked.  For each VOTED entry in order (the reference takes its end
 *     iterator before the loop): stop if the list holds more than 80 rows; append and mark the first of best[0 .. n_best) that is
 *     not bad and not marked (GetBestCovisibilityKeyFrames(10)); append and mark the first child, in the children slice's order
 *     (std::set<KeyFrame*>: ascending kf_order), that is not bad and not marked; if the parent exists and is not marked append and
 *     mark it -- its badness is NOT tested -- and END THE OUTER LOOP (the `break` at :1206 leaves the for over keyframes).
 *     ref_kf = the vote's kf_max (mpReferenceKF; -1 leaves the previous one in place).
 *   Points.  The local keyframes in list order, their slots in index order: a slot of -1 and a point already marked are passed over;
 *     a point that is not bad is appended and marked; a bad point is neither.  A keyframe's own badness is not tested.
 *   Skip.  skip = 1 for a local point that the frame holds in a slot, and for one the caller lists as also seen: the outliers that
 *     TrackWithMotionModel / TrackReferenceKeyFrame took out of the frame after setting mnLastFrameSeen (:711, :825).  A bad point in
 *     a frame slot reads as empty (:1041-1042, :1127-1129).
 * Stated input domain: that of the vote, and a point occupies at most one slot of a keyframe.  Outside it memory safety and
 * run-to-run determinism are promised and nothing else.  No input is modified.
 * Status of a frame: OK; EMPTY -- the vote was ORBFE_COV_EMPTY: the header alone is written (ref_kf = -1); the reference returns early
 * (:1133) and keeps the previous frame's lists, which stays the caller's; OVERFLOW -- more than kf_cap keyframes or p_cap points
 * exist: the counts are exact, the first cap of the stated order are written and nothing behind them is touched; REFUSED -- decided
 * by the frame's own workgroup before anything else of the frame is written, no other frame touched, counts 0, ref_kf = -1,
 * d_n_points = 0: a vote header that is OVERFLOW or REFUSED or whose n_written lies outside 0 .. conn_cap or kf_max outside
 * [-1, n_kf); a voted row, a best row, a child or a parent outside the table (parent: [-1, n_kf)); n_best outside 0 .. 10; a children
 * slice, a frame's slot slice or an also-seen slice outside its array; a local keyframe with n_keys < 0 or with n_keys > 0 and a
 * null or misaligned slot address; a slot of a local keyframe or of the frame < -1 or >= n_points; an also-seen index outside
 * [0, n_points).
 * Deterministic: integer LDS atomics only, whose order does not reach the result; a frame's bytes do not depend on S, on its
 * position in the batch or on the run.  No CPU fallback.
 * Limits, each refused with ORBFE_ERR_INVALID one step past it, before any device call (pinned by tests/test_localmap_cpu.py):
 *   ORBFE_LM_MAX_FRAMES          65 535 frames per launch: one workgroup each, the grid limit the other batch forms use
 *   ORBFE_LM_MAX_KEYFRAMES       = ORBFE_COV_MAX_KEYFRAMES: the same table; the marks are one bit per row in LDS (4 KiB)
 *   ORBFE_LM_MAX_POINTS          = ORBFE_COV_MAX_POINTS: the same table; the marks are one bit per point in LDS (128 KiB of the 160)
 *   ORBFE_LM_MAX_TOTAL_SLOTS     = ORBFE_COV_MAX_TOTAL_SLOTS: the slot array of the vote
 *   ORBFE_LM_MAX_TOTAL_CHILDREN  = ORBFE_COV_MAX_KEYFRAMES: a spanning tree gives a row to one parent
 *   ORBFE_LM_MAX_TOTAL_SEEN      16 777 216 also-seen indices per call (64 MiB; offsets stay far inside int32)
 *   ORBFE_LM_MAX_KF_CAP          kf_cap 1 .. ORBFE_COV_MAX_CONN + 3: the list exceeds max(n_voted, 83) by nothing and lives in LDS (8 KiB)
 *   ORBFE_LM_MAX_P_CAP           p_cap 1 .. ORBFE_COV_MAX_POINTS: a list holds a point once
 *   ORBFE_LM_MAX_TOTAL_RECORDS   S x p_cap <= 4 194 304 (host form: 288 MiB of records come back in one copy)
 *   the host form also keeps ORBFE_COV_MAX_KEYS per row and ORBFE_COV_MAX_TOTAL_KEYS over the table, whose slot arrays it stages */
#define ORBFE_LM_MAX_FRAMES 65535
#define ORBFE_LM_MAX_KEYFRAMES ORBFE_COV_MAX_KEYFRAMES
#define ORBFE_LM_MAX_POINTS ORBFE_COV_MAX_POINTS
#define ORBFE_LM_MAX_TOTAL_SLOTS ORBFE_COV_MAX_TOTAL_SLOTS
#define ORBFE_LM_MAX_TOTAL_CHILDREN ORBFE_COV_MAX_KEYFRAMES
#define ORBFE_LM_MAX_TOTAL_SEEN 16777216
#define ORBFE_LM_MAX_KF_CAP (ORBFE_COV_MAX_CONN + 3)
#define ORBFE_LM_MAX_P_CAP ORBFE_COV_MAX_POINTS
#define ORBFE_LM_MAX_TOTAL_RECORDS 4194304
#define ORBFE_LM_BEST 10                  /* GetBestCovisibilityKeyFrames(10), Tracking.cc:1172 */
#define ORBFE_LM_SIZE 80                  /* `mvpLocalKeyFrames.size() > 80`, :1167 */
enum { ORBFE_LM_OK = 0, ORBFE_LM_EMPTY = 1, ORBFE_LM_OVERFLOW = 2, ORBFE_LM_REFUSED = 3 };             /* orbfe_lm_header.status */
enum { ORBFE_LM_STOP_EXHAUSTED = 0, ORBFE_LM_STOP_SIZE = 1, ORBFE_LM_STOP_PARENT = 2 };                /* orbfe_lm_header.stop */
typedef struct orbfe_lm_graph {           /* one per keyframe row; 56 bytes */
  int32_t parent;                         /* GetParent(): its row, or -1 */
  int32_t child_offset, n_children;       /* GetChilds(): its slice of the children array, rows in ascending kf_order */
  int32_t n_best;                         /* 0 .. 10 */
  int32_t best[ORBFE_LM_BEST];            /* GetBestCovisibilityKeyFrames(10), in its order */
} orbfe_lm_graph;
typedef struct orbfe_lm_frame {           /* 8 bytes */
  int32_t seen_offset, n_seen;            /* its slice of the also-seen array (point indices) */
} orbfe_lm_frame;
typedef struct orbfe_lm_header {          /* 32 bytes, always written */
  int32_t n_voted;                        /* entries of the vote */
  int32_t n_local_kf, n_local_points;     /* exact, even beyond kf_cap / p_cap */
  int32_t ref_kf;                         /* the vote's kf_max */
  int32_t stop;                           /* ORBFE_LM_STOP_*: the rule that ended the expansion */
  int32_t status;                         /* ORBFE_LM_OK .. ORBFE_LM_REFUSED */
  int32_t reserved[2];                    /* 0 */
} orbfe_lm_header;
/* S frames, DEVICE pointers (the keyframe table holds device addresses), asynchronous on `stream` (NULL: the NULL stream), one
 * launch.  d_headers [S] / d_entries [S][conn_cap]: the vote's output.  d_subjects [S]: the frames' slices of d_slots.  d_frames
 * [S] and d_seen: the also-seen slices; d_frames NULL: no frame has one.  Outputs: d_lm_headers [S]; d_local_kf [S][kf_cap] rows;
 * d_local_points [S][p_cap] point indices; d_n_points [S] = min(n_local_points, p_cap); and, when d_point_records (a resident
 * orbfe_map_point[n_points], indexed by point) is not NULL, d_map_points [S][p_cap]: each record copied from the resident one with
 * `skip` replaced.  d_map_points, d_n_points and p_cap feed orbfe_search_local_points_batch_device unchanged.
 * Limits (ORBFE_ERR_INVALID): the ORBFE_LM_MAX_* above, every count >= 0, 1 <= conn_cap <= ORBFE_COV_MAX_CONN, null arrays with a
 * count > 0, d_map_points null with d_point_records, records not 4-byte (the keyframe table: 8-byte) aligned.  S == 0: nothing is
 * launched. */
int orbfe_local_map_batch_device(int S, const orbfe_cov_header* d_headers, const orbfe_cov_entry* d_entries, int conn_cap,
                                 const orbfe_lm_graph* d_graph, const int32_t* d_children, int n_children_total,
                                 const orbfe_cov_keyframe* d_keyframes, const uint8_t* d_kf_bad, int n_kf, const uint8_t* d_point_bad,
                                 int n_points, const int32_t* d_slots, int n_slots_total, const orbfe_cov_subject* d_subjects,
                                 const orbfe_lm_frame* d_frames, const int32_t* d_seen, int n_seen_total,
                                 const orbfe_map_point* d_point_records, int kf_cap, int p_cap, orbfe_lm_header* d_lm_headers,
                                 int32_t* d_local_kf, int32_t* d_local_points, int32_t* d_n_points, orbfe_map_point* d_map_points,
                                 void* stream);
/* The same from HOST arrays (the table's `slots` are host addresses and are staged with it), synchronous, on the calling thread's
 * current device: one upload, one launch, one download.  Of each frame the header, n_points and the written head of each list come
 * back; what lies behind stays the caller's.  Limits: as above, and the host-form limits of the list. */
int orbfe_local_map(const orbfe_cov_header* headers, const orbfe_cov_entry* entries, int conn_cap, const orbfe_lm_graph* graph,
                    const int32_t* children, int n_children_total, const orbfe_cov_keyframe* keyframes, const uint8_t* kf_bad, int n_kf,
                    const uint8_t* point_bad, int n_points, const int32_t* slots, int n_slots_total, const orbfe_cov_subject* subjects,
                    const orbfe_lm_frame* frames, const int32_t* seen, int n_seen_total, const orbfe_map_point* point_records, int S,
                    int kf_cap, int p_cap, orbfe_lm_header* lm_headers, int32_t* local_kf, int32_t* local_points, int32_t* n_points_out,
                    orbfe_map_point* map_points);

/* ---- Keyframe decision and close stereo points: the statistics tail of Tracking::TrackLocalMap (L/src/Tracking.cc:851-877),
 * Tracking::NeedNewKeyFrame (:880-962), the depth-ordered point creation of Tracking::CreateNewKeyFrame (:973-1024), the temporal
 * points of Tracking::UpdateLastFrame (:732-777) and the points of Tracking::StereoInitialization (:455-479) ------------------------------
 * One frame is one workgroup; csrc/keyframe_internal.h states every rule once, for the kernel and for host code.  The arrays are
 * those of orbfe_pose_optimization_batch_device, so a frame goes from orbfe_local_map_batch_device over
 * orbfe_search_local_points_batch_device and orbfe_pose_optimization_batch_device to this call on one stream, and its new points are
 * orbfe_map_point records that the search, fuse and refresh stages take unchanged.  Which parts run is `flags`:
 *   ORBFE_KF_STATISTICS   n_matches_inliers = the slots i < n that are occupied (assigned[i] >= 0) and not outlier and, when
 *     only_tracking == 0, hold an observed point (:854-866); track_ok = !(recent && n_matches_inliers < 50) && n_matches_inliers >= 30
 *     with recent = frame_id < last_reloc_frame_id + max_frames (:870-877).  IncreaseFound and the stereo sensor's clearing of outlier
 *     slots (:857, :863-864) stay with the caller: ORBFE_POSE_DISCARD of the pose stage does the latter, and it has to be done
 *     before this call where the creation is to see those slots empty.
 *   ORBFE_KF_DECISION     (requires STATISTICS, whose count it reads) n_tracked_close / n_non_tracked_close over the keypoints with
 *     depth > 0 && depth < th_depth -- strict, an entry exactly at th_depth is in neither -- tracked = occupied and not outlier, both 0
 *     for a monocular sensor (:906-917); n_ref_matches = KeyFrame::TrackedMapPoints(n_kfs <= 2 ? 2 : 3) of table row ref_kf (0 for
 *     ref_kf == -1): its slots p >= 0 with !point_bad[p] && point_observations[p] >= nMinObs (L/src/KeyFrame.cc:237-256); then
 *     :881-961 with every comparison in the source's types: the frame id unsigned 64-bit against a 32-bit unsigned sum that wraps,
 *     `n_matches_inliers < n_ref_matches * 0.25` in double, `n_matches_inliers < n_ref_matches * thRefRatio` in float.  early: the
 *     return before the conditions that was taken (ORBFE_KF_EARLY_*: only_tracking :881, mapper stopped :885, recent relocalisation
 *     with n_kfs > max_frames :892); the counts are written all the same.  conditions: c1a | c1b << 1 | c1c << 2 | c2 << 3;
 *     need: the return value; interrupt_ba: :951 was reached -- InterruptBA() and SetNotStop stay with the caller.
 *   ORBFE_KF_CREATE       the selection and the new points, by `mode`.  With DECISION it runs only for frames whose need is 1; the
 *     others get M = c = L = n_created = n_cleared = 0, d_n_new = 0 and d_depth_selected = -1.
 *     The sensor is not asked (:973, :728): a monocular frame has no positive depth, and a caller whose arrays hold some tests it.
 * Selection (:979-1022, identical at :734-777).  Candidates: i < n with depth[i] > 0 (NaN and non-positive out, +inf in), M of them,
 * ordered as std::sort orders pair<float, int>: ascending depth, ties by ascending index -- for positive floats the ascending order of
 * the 64-bit key (bits(depth) << 32) | i, which has no equal keys.  The loop counts nPoints in both branches and breaks after an entry
 * with depth > th_depth && nPoints > 100, so the selected prefix has L = min(M, max(100, c) + 1) entries, c = the candidates with
 * depth <= th_depth (note <=: an entry exactly at th_depth does not stop the loop).  An entry of the prefix is CREATED when its slot is
 * empty or holds a point that is not observed (a temporal point; ORBFE_KF_MODE_KEYFRAME clears that slot first and counts it in
 * n_cleared, :1002; ORBFE_KF_MODE_LAST_FRAME does not); an entry whose slot holds an observed point is kept: nothing is written for it,
 * but it counts.  ORBFE_KF_MODE_STEREO_INIT (:455-479): only when n > 500, every candidate in INDEX order, whatever its slot holds; no
 * sort, L = M, c as above.
 * New point records, in creation order (the order of mnId, of mlpTemporalPoints and of Map::AddMapPoint): d_new_points [S][new_cap],
 * d_new_index [S][new_cap] the keypoint index of each, d_n_new [S] = min(n_created, new_cap).  pos = Frame::UnprojectStereo(i)
 * (L/src/Frame.cc:668-679) in the arithmetic of orbfe_unproject_stereo_device, byte-equal to its row i.  KEYFRAME and STEREO_INIT
 * (MapPoint(x3D, pKF, pMap), AddObservation, ComputeDistinctiveDescriptors, UpdateNormalAndDepth): one observation, so desc = row i,
 * normal = (0.0f + unit) * (float)(1.0 / 1), max_distance = dist * scale_factors[octave], min_distance = max_distance /
 * scale_factors[n_levels - 1] -- byte-equal to orbfe_refresh_map_points of the same one-observation point; observed = 1.  LAST_FRAME
 * (MapPoint(x3D, pMap, &mLastFrame, i), L/src/MapPoint.cc:49-77): the same expressions without the sum and the division by the count,
 * which changes one thing: a normal component of -0.0f stays -0.0f here and is +0.0f in the keyframe form; observed = 0.  skip = 0.
 * d_depth_selected [S][cap] (nullable): depth[i] for every entry of the prefix, created or kept, -1 elsewhere (rows at and behind n
 * included); orbfe_track_queries_stereo_device takes it in place of d_depth and so gets the reference's point set.
 * d_assigned (nullable: every slot is empty) is written in KEYFRAME and STEREO_INIT mode only: a cleared slot becomes -1, a created
 * slot whose record was written becomes d_n_points_base[f] (NULL: 0) + its position in the created list.  No other input is modified.
 * Arrays: frame f owns rows [f * cap, f * cap + d_n[f]) of d_keys_un / d_desc / d_depth / d_assigned / d_outlier (nullable: no
 * outliers); d_n[f] is clamped to [0, cap].  Assigned values index the records of frame (f - frame_shift) mod S at d_points + that
 * frame * p_cap * point_stride, of which d_n_points[that frame] (clamped to [0, p_cap]) exist; observed_offset is the byte offset of
 * the record's int32 `observed` field (orbfe_map_point: 36, orbfe_last_point: 16), -1: every occupied slot counts as observed.
 * d_ref_kf: an int32 per frame, ref_kf_stride bytes apart (the ref_kf field of an orbfe_lm_header array: the address of the first
 * one and 32).  Of the orbfe_cov_keyframe table `slots` and `n_keys` are read, of rows some frame names.
 * Status of a frame: OK; OVERFLOW -- more than new_cap created: the counts are exact, the first new_cap records are written and
 * nothing behind them is touched; REFUSED -- decided before anything else of the frame is written, every count 0, d_n_new = 0: an
 * assigned value >= the record count; an octave outside [0, n_levels) on a created entry; ref_kf outside [-1, n_kf); a reference row
 * with n_keys < 0, or n_keys > 0 and a null or misaligned slot address, or a slot < -1 or >= n_map_points.
 * Deterministic: ballots and integer sums only; a frame's bytes do not depend on S, on its position in the batch or on the run.
 * No CPU fallback.  Limits, each refused with ORBFE_ERR_INVALID one step past it, before any device call (tests/test_keyframe_cpu.py):
 *   ORBFE_KF_MAX_FRAMES   65 535 frames per launch: one workgroup each, the grid limit the other batch forms use
 *   ORBFE_KF_MAX_CAP      1 <= cap <= 9 500: the frame limit of the projection searches and the pose stage; the keys of a frame, 8
 *                         bytes each, are sorted in LDS (padded to a power of two: 16 384 keys, 128 KiB of the 160)
 *   1 <= new_cap <= cap; p_cap >= 1; frame_shift >= 0; point_stride >= 12 and a multiple of 4; observed_offset -1, or a multiple of 4
 *   in [0, point_stride - 4]; ref_kf_stride >= 4 and a multiple of 4; n_kf 0 .. ORBFE_COV_MAX_KEYFRAMES; n_map_points 0 ..
 *   ORBFE_COV_MAX_POINTS; n_levels 1 .. ORBFE_MAX_LEVELS; mode 0 .. 2; flags a non-empty subset of the three, DECISION only with
 *   STATISTICS; null arrays that the flags need with S > 0 (the tables with a count > 0); records not 4-byte (the decision records and
 *   the keyframe table: 8-byte) aligned.  S == 0: nothing is launched and nothing behind a pointer is read. */
#define ORBFE_KF_MAX_FRAMES 65535
#define ORBFE_KF_MAX_CAP 9500
#define ORBFE_KF_MAX_TOTAL_ROWS 4194304   /* host form: S x cap keypoint rows (272 MiB staged), S x p_cap point records */
#define ORBFE_KF_STATISTICS 1
#define ORBFE_KF_DECISION 2
#define ORBFE_KF_CREATE 4
enum { ORBFE_KF_MODE_KEYFRAME = 0, ORBFE_KF_MODE_LAST_FRAME = 1, ORBFE_KF_MODE_STEREO_INIT = 2 };
enum { ORBFE_KF_SENSOR_MONOCULAR = 0, ORBFE_KF_SENSOR_STEREO = 1, ORBFE_KF_SENSOR_RGBD = 2 };          /* System::eSensor */
enum { ORBFE_KF_OK = 0, ORBFE_KF_OVERFLOW = 2, ORBFE_KF_REFUSED = 3 };                                 /* orbfe_kf_header.status */
enum { ORBFE_KF_EARLY_NONE = 0, ORBFE_KF_EARLY_ONLY_TRACKING = 1, ORBFE_KF_EARLY_STOPPED = 2, ORBFE_KF_EARLY_RELOCALISED = 3 };
#define ORBFE_KF_C1A 1
#define ORBFE_KF_C1B 2
#define ORBFE_KF_C1C 4
#define ORBFE_KF_C2 8
#define ORBFE_KF_CLOSE_POINTS 100         /* `nPoints > 100`, :1020 and :775; `nTrackedClose < 100`, :919 */
#define ORBFE_KF_INIT_MIN_KEYS 500        /* `mCurrentFrame.N > 500`, :455 */
typedef struct orbfe_kf_decision_in {     /* what :851-961 read beside the frame; 56 bytes, 8-byte aligned */
  uint64_t frame_id;                      /* mCurrentFrame.mnId (long unsigned int) */
  uint32_t last_reloc_frame_id;           /* mnLastRelocFrameId (unsigned int) */
  uint32_t last_keyframe_id;              /* mnLastKeyFrameId (unsigned int) */
  int32_t max_frames, min_frames;         /* mMaxFrames, mMinFrames */
  int32_t sensor;                         /* ORBFE_KF_SENSOR_* */
  int32_t only_tracking;                  /* mbOnlyTracking */
  int32_t mapper_stopped;                 /* mpLocalMapper->isStopped() || mpLocalMapper->stopRequested() */
  int32_t accept_keyframes;               /* mpLocalMapper->AcceptKeyFrames() */
  int32_t keyframes_in_queue;             /* mpLocalMapper->KeyframesInQueue() */
  int32_t n_kfs;                          /* mpMap->KeyFramesInMap() */
  int32_t reserved[2];
} orbfe_kf_decision_in;
typedef struct orbfe_kf_scales {          /* 72 bytes; read on the host before the call returns */
  int32_t n_levels;                       /* mnScaleLevels, 1 .. ORBFE_MAX_LEVELS */
  float th_depth;                         /* mThDepth */
  float scale_factors[ORBFE_MAX_LEVELS];  /* mvScaleFactors */
} orbfe_kf_scales;
typedef struct orbfe_kf_header {          /* 64 bytes, always written */
  int32_t n_matches_inliers;              /* mnMatchesInliers */
  int32_t track_ok;                       /* the return value of TrackLocalMap */
  int32_t n_tracked_close, n_non_tracked_close, n_ref_matches;
  int32_t early;                          /* ORBFE_KF_EARLY_* */
  int32_t conditions;                     /* ORBFE_KF_C1A | C1B | C1C | C2 */
  int32_t need;                           /* the return value of NeedNewKeyFrame */
  int32_t interrupt_ba;                   /* :951 was reached */
  int32_t M, c, L;                        /* candidates, those with depth <= th_depth, length of the selected prefix */
  int32_t n_created, n_cleared;           /* exact, even beyond new_cap */
  int32_t status;                         /* ORBFE_KF_OK .. ORBFE_KF_REFUSED */
  int32_t reserved;                       /* 0 */
} orbfe_kf_header;
typedef struct orbfe_kf_call {            /* the arrays and counts of one call; 8-byte aligned */
  const orbfe_keypoint* keys_un;          /* [S][cap] mvKeysUn (x, y, octave are read) */
  const uint8_t* desc;                    /* [S][cap][32] mDescriptors */
  const float* depth;                     /* [S][cap] mvDepth */
  const int32_t* n;                       /* [S] N */
  const orbfe_unproject_cam* cam;         /* [S] */
  int32_t* assigned;                      /* [S][cap] in/out, nullable */
  const void* points;                     /* the records the assigned values index */
  const int32_t* n_points;                /* [S] */
  const uint8_t* outlier;                 /* [S][cap] mvbOutlier, nullable */
  const orbfe_kf_decision_in* decision;   /* [S]; STATISTICS and DECISION */
  const void* ref_kf;                     /* DECISION: see above */
  const orbfe_cov_keyframe* keyframes;    /* [n_kf]; DECISION */
  const uint8_t* point_bad;               /* [n_map_points] MapPoint::isBad(); DECISION */
  const int32_t* point_observations;      /* [n_map_points] MapPoint::Observations(): nObs, a stereo observation counts 2; DECISION */
  const int32_t* n_points_base;           /* [S], nullable; CREATE */
  orbfe_kf_header* headers;               /* [S] out */
  orbfe_map_point* new_points;            /* [S][new_cap] out; CREATE */
  int32_t* new_index;                     /* [S][new_cap] out; CREATE */
  int32_t* n_new;                         /* [S] out; CREATE */
  float* depth_selected;                  /* [S][cap] out, nullable; CREATE */
  int32_t S, cap, new_cap, p_cap, frame_shift, point_stride, observed_offset, ref_kf_stride, n_kf, n_map_points, mode, flags;
} orbfe_kf_call;
/* S frames in one launch.  Every pointer of `call` is a DEVICE pointer (the keyframe table holds device addresses); `call` and
 * `camera` themselves are HOST records, read before the call returns.  Asynchronous on `stream` (NULL: the NULL stream). */
int orbfe_keyframe_insertion_batch_device(const orbfe_kf_call* call, const orbfe_kf_scales* camera, void* stream);
/* The same from HOST arrays (the table's `slots` are host addresses; the slot arrays of the rows some frame names are staged with
 * it), synchronous, on the calling thread's current device: one upload, one launch, one download.  Of each frame the header, n_new,
 * the written head of the two lists, its row of depth_selected and (KEYFRAME and STEREO_INIT mode) its rows of assigned come back;
 * a REFUSED frame brings back its header and n_new alone.  Host-form limits (ORBFE_ERR_INVALID): S x cap and, with assigned, S x p_cap
 * at most ORBFE_KF_MAX_TOTAL_ROWS; a named reference row with n_keys > ORBFE_COV_MAX_KEYS; the named rows' n_keys summing to more than
 * ORBFE_COV_MAX_TOTAL_KEYS.  ref_kf is read on the host to find those rows; a value outside [-1, n_kf) is refused by the device. */
int orbfe_keyframe_insertion(const orbfe_kf_call* call, const orbfe_kf_scales* camera);

/* SearchForInitialization (L/src/ORBmatcher.cc:388-492), the monocular map-initialisation matcher: level-0
 * keypoints of F1 are searched in a window of `window_size` pixels around prev_matched_xy[2*i..2*i+1] in F2; a
 * closer later keypoint steals an earlier match (vMatchedDistance / vnMatches21).  matches12[i] = F2 index or -1;
 * prev_matched_xy is updated for the matched keypoints (:487-489).  HOST pointers, synchronous. */
int orbfe_search_for_initialization(const orbfe_frame_view* f1, const orbfe_frame_view* f2, float* prev_matched_xy,
                                    int window_size, float nnratio, int check_orientation, int32_t* matches12,
                                    int* n_matches);

/* Both searches for n_frames frames at once, DEVICE pointers, asynchronous on stream (NULL: the handle's).
 * Frame f: keypoints/descriptors/u_right rows [f*cap, f*cap + d_n[f]); queries [f*q_cap, f*q_cap + d_nq[f]).
 * mode 0 = A11 (points, ratio test nnratio), mode 1 = A12 (frame, rotation histogram if check_orientation).
 * d_blocked / d_assigned: n_frames x cap (in/out as above); d_n_matches: n_frames. */
int orbfe_proj_match_batch_device(orbfe_matcher* m, int n_frames, const orbfe_keypoint* d_kps, const uint8_t* d_desc,
                                  const int32_t* d_n, const float* d_u_right, int cap, float min_x, float max_x,
                                  float min_y, float max_y, const orbfe_query* d_q, const int32_t* d_nq, int q_cap,
                                  int mode, float nnratio, int check_orientation, uint8_t* d_blocked,
                                  int32_t* d_assigned, int32_t* d_n_matches, void* stream);

/* Frame::ComputeStereoMatches (L/src/Frame.cc:477-646) for n_pairs stereo frames, DEVICE pointers,
 * asynchronous.  Left/right keypoints+descriptors as produced by orbfe_extract_batch_device with the
 * two extractor handles, whose device pyramids (image p of each) are read for the 11x11 SAD refinement.
 * d_u_right / d_depth: n_pairs x cap floats (-1 = no match); d_n_matched: n_pairs (matches kept). */
int orbfe_stereo_match_device(orbfe_matcher* m, orbfe_extractor* left, orbfe_extractor* right, int n_pairs,
                              const orbfe_keypoint* d_kps_l, const uint8_t* d_desc_l, const int32_t* d_n_l,
                              const orbfe_keypoint* d_kps_r, const uint8_t* d_desc_r, const int32_t* d_n_r,
                              int cap, float mbf, float mb, float* d_u_right, float* d_depth, int32_t* d_n_matched,
                              void* stream);

/* Frame::ComputeStereoMatches (L/src/Frame.cc:477-646) for the ONE stereo pair the two extractors processed last -- the
 * per-frame calling pattern of Frame::Frame (L/src/Frame.cc:91-99: ExtractORB on two threads, then ComputeStereoMatches).
 * HOST pointers, synchronous.  kps / desc are what the two orbfe_extract calls returned (mvKeys, mDescriptors, mvKeysRight,
 * mDescriptorsRight); the row search, the descriptor match, the 11x11 SAD refinement on the pyramids still resident in HBM
 * (no mvImagePyramid download), the parabola and the median cut run on the device.  u_right / depth: n_l floats (mvuRight,
 * mvDepth; -1 = no match); *n_matched (optional) = matches kept.  mb = Frame::mb (minZ, :505), must be > 0.
 * Both extractors must have completed an extraction of the same image size on the calling thread's device. */
int orbfe_stereo_match(orbfe_extractor* left, orbfe_extractor* right, const orbfe_keypoint* kps_l, const uint8_t* desc_l,
                       int n_l, const orbfe_keypoint* kps_r, const uint8_t* desc_r, int n_r, float mbf, float mb,
                       float* u_right, float* depth, int* n_matched);

/* --------------------------------------------------------------------------------------- ORBVocabulary */
/* Frame::ComputeBoW (L/src/Frame.cc:412-417): ORBVocabulary::transform(descriptors, BowVector&, FeatureVector&, 4)
 * = DBoW2::TemplatedVocabulary::transform (Source/ThirdParty/DBoW2/DBoW2-local/include/DBoW2/
 * TemplatedVocabulary.h:1125-1257).  SURVEY.md §8(f) row 2: produces the FeatureVector SearchByBoW consumes. */
typedef struct orbfe_vocabulary orbfe_vocabulary;
/* Tree as arrays: node 0 is the root, parent[i] < i, children keep ascending id order; is_leaf[i] marks words
 * (word ids count leaves in id order); desc = n_nodes x 32 bytes; scoring / weighting = DBoW2::ScoringType /
 * WeightingType values (L1_NORM = 0, TF_IDF = 0). */
int orbfe_vocabulary_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                            const uint8_t* is_leaf, const uint8_t* desc, const double* weight, int device,
                            orbfe_vocabulary** out);
/* ORBVocabulary::loadFromTextFile (L/src/ORBVocabulary.cc:11-127), the ORBvoc.txt format. */
int orbfe_vocabulary_load_text(const char* path, int device, orbfe_vocabulary** out);
/* ORBVocabulary::loadFromBinaryFile (L/src/ORBVocabulary.cc:152-213): the format of saveToBinaryFile (:217-243), float
 * weights, including the duplicate of the last node the reference's eof loop appends. */
int orbfe_vocabulary_load_binary(const char* path, int device, orbfe_vocabulary** out);
int orbfe_vocabulary_destroy(orbfe_vocabulary* v);
int orbfe_vocabulary_info(const orbfe_vocabulary* v, int* k, int* L, int* n_nodes, int* n_words);
/* Tree descent only, DEVICE pointers, asynchronous: per descriptor the word id, the node at level L - levelsup and
 * the word weight.  A descent that ends in a leaf ABOVE level L - levelsup never reaches `*nid = final_id`
 * (TemplatedVocabulary.h:1249) and the reference's caller reads an uninitialised NodeId (:1149); this library reports node 0
 * (the root) for such a feature.  ORBvoc.txt with levelsup = 4 has no leaf above level 2, so the case does not arise there. */
int orbfe_bow_transform_device(orbfe_vocabulary* v, const uint8_t* d_desc, int n, int levelsup, int32_t* d_word,
                               int32_t* d_node, double* d_weight, void* stream);
/* The whole transform for one frame, HOST pointers, synchronous.  BowVector as ascending (bow_ids, bow_vals) pairs,
 * FeatureVector as ascending nodes {node_id, start, count} into fv_idx; every output array holds n entries at
 * most.  word_id / node_id / weight (per feature) are optional. */
int orbfe_compute_bow(orbfe_vocabulary* v, const uint8_t* desc, int n, int levelsup, int32_t* word_id,
                      int32_t* node_id, double* weight, int32_t* bow_ids, double* bow_vals, int* n_bow,
                      orbfe_featvec_node* fv_nodes, int32_t* fv_idx, int* n_fv_nodes);
/* A handle's tree in the layout orbfe_vocabulary_create takes (orbfe_vocabulary_info gives n_nodes); every output is optional.
 * For this and the two save functions EVERY handle, loaded ones included, keeps a host copy of its tree beside the device arrays:
 * 45 bytes per node, about 48 MB for ORBvoc.txt. */
int orbfe_vocabulary_nodes(const orbfe_vocabulary* v, int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight);
/* ORBVocabulary::saveToTextFile / saveToBinaryFile (L/src/ORBVocabulary.cc:131-150, :217-243) of a tree given as arrays; host only, no
 * device needed.  The binary file is the reference's byte for byte (float weights).  The text file is what loadFromTextFile and
 * orbfe_vocabulary_load_text read; DEVIATION: the weight is written with 17 significant digits so that it reads back as the same
 * double, where the reference's stream writes six and loses the rest. */
int orbfe_vocabulary_write_text(const char* path, int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                                const uint8_t* is_leaf, const uint8_t* desc, const double* weight);
int orbfe_vocabulary_write_binary(const char* path, int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                                  const uint8_t* is_leaf, const uint8_t* desc, const double* weight);
/* export, then write */
int orbfe_vocabulary_save_text(const orbfe_vocabulary* v, const char* path);
int orbfe_vocabulary_save_binary(const orbfe_vocabulary* v, const char* path);

/* ------------------------------------------------------------------- DBoW2::TemplatedVocabulary::create on the device */
/* Trains a vocabulary from descriptors: hierarchical k-medians in Hamming space with k-means++ seeding, the bit-majority mean
 * (FORB::meanValue) and IDF weights -- HKmeansStep, initiateClustersKMpp, createWords and setNodeWeights of
 * Source/ThirdParty/DBoW2/DBoW2-local/include/DBoW2/TemplatedVocabulary.h:640-994 in their literal form.  Every value is an integer
 * (or a double that is exact), so the tree equals a plain reading of the reference bit for bit; the weights are log((double)NDocs /
 * Ni) with the host's libm, Ni from the full transform descent of every training feature over the finished tree, NDocs counting
 * empty images too; TF and BINARY give every word weight 1; inner nodes have weight 0, and so has a word with Ni == 0.
 * A node with n <= k features is one cluster per feature, in order; a child is clustered only below level L and with more than one
 * member, so leaves above level L are normal.  Node ids are the reference's creation order (a node's children get consecutive ids
 * when the node is processed; nodes are processed depth first), word ids count leaves in id order.
 * Three DEVIATIONS from the reference:
 *   1. draws          the reference pulls rand() lazily from one stream in depth-first order; the number of draws per node depends
 *                     on the data, which a level-parallel schedule cannot reproduce.  Each node takes its draws from a counter-based
 *                     generator keyed by (seed, level, path, j): level = the current_level of its HKmeansStep (1 for the root's),
 *                     path = the base-k number of the child indices from the root (0 for the root), j = the node's draw counter,
 *                     0 for the first centre; a cut of 0.0 is drawn again with the next j.  The value is
 *                     splitmix64(splitmix64(splitmix64(splitmix64(seed) ^ level) ^ path) ^ j) >> 33, in 0 .. RAND_MAX = 2^31 - 1
 *                     (orbfe_vocabulary_training_draw).  The distribution is the reference's, the sequence is not.
 *   2. empty cluster  when a group loses all its members the reference releases the mean and then reads through a null pointer
 *                     in FORB::distance.  Here an empty cluster keeps the centre it had; it stays a node, possibly one no feature
 *                     reaches, and every mean step that met one is counted in n_empty_clusters.
 *   3. iteration cap  the reference has none; here a node stops after max_iterations association rounds (default
 *                     ORBFE_VOCAB_TRAIN_MAX_ITERATIONS) with the association it has and is counted in n_capped_nodes.
 * Segments (nodes) of at least wide_min descriptors are walked by a grid of workgroups with one launch pair per round; smaller ones
 * are held by one workgroup from seeding to convergence.  wide_min never changes a result; a small value costs workspace (one
 * 1 KiB block of counters per cluster of every wide segment).  There is no CPU path: ORBFE_ERR_NO_DEVICE without a device.
 * ORBFE_ERR_INVALID (with an error string, before the device is looked for): k outside 2..20, L outside 1..10, scoring outside
 * 0..5, weighting outside 0..3, fewer than 1 or more than 2^30 descriptors, n_images < 1, image_start not monotone from 0, a
 * workspace smaller than orbfe_vocabulary_train_workspace_bytes asks for, null pointers. */
#define ORBFE_VOCAB_TRAIN_MAX_ITERATIONS 1000
typedef struct orbfe_vocab_train_config {
  int32_t k, L;                 /* 2..20, 1..10: what loadFromTextFile accepts */
  int32_t scoring, weighting;   /* 0..5, 0..3 */
  uint64_t seed;
  int32_t max_iterations;       /* 0: ORBFE_VOCAB_TRAIN_MAX_ITERATIONS */
  int32_t wide_min;             /* segments of at least this many descriptors take the wide form; 0: the library's choice;
                                   clamped to what the narrow form can hold.  Never changes a result. */
} orbfe_vocab_train_config;    /* 32 bytes */
typedef struct orbfe_vocab_train_stats {
  int32_t n_nodes, n_words, n_kmeans_nodes, n_trivial_nodes, n_short_seedings, n_empty_clusters, n_capped_nodes,
          max_rounds, nodes_per_level[11];
} orbfe_vocab_train_stats;     /* 76 bytes; nodes_per_level[0] = 1, the root; max_rounds counts associations of one node */
/* the 31-bit draw of deviation 1; host only, needs no device */
uint32_t orbfe_vocabulary_training_draw(uint64_t seed, uint32_t level, uint64_t path, uint32_t j);
int orbfe_vocabulary_train_workspace_bytes(const orbfe_vocab_train_config* cfg, int64_t n_desc, int n_images, size_t* bytes);
/* HOST pointers, synchronous: desc = image_start[n_images] x 32 bytes, the images ragged and concatenated (image i holds features
 * image_start[i] .. image_start[i + 1] - 1).  device < 0: the current one; the calling thread's current device is the same after
 * the call as before it.  leaf_node (optional, [n_desc]): the node, in final ids, of
 * the deepest group training feature i ended in.  stats is optional.  *vocabulary is an ordinary handle, usable at once by
 * orbfe_bow_transform_device and everything downstream. */
int orbfe_vocabulary_train(const orbfe_vocab_train_config* cfg, const uint8_t* desc, const int32_t* image_start, int n_images,
                           int device, int32_t* leaf_node, orbfe_vocab_train_stats* stats, orbfe_vocabulary** vocabulary);
/* DEVICE pointers of the calling thread's CURRENT device (the call runs there and does not check where the pointers live), as
 * orbfe_extract_batch_device leaves them: d_desc = [n_frames][cap][32] (16-byte aligned), d_n = [n_frames] counts;
 * whatever lies behind a frame's count is not read.  d_workspace: 256-byte aligned, at least what
 * orbfe_vocabulary_train_workspace_bytes gives for the sum of the counts (n_frames * cap always suffices).  d_leaf_node: optional,
 * [sum of counts], features in frame order.  Synchronous: the host reads one control word per round of a level and the node table
 * per level.  stream: NULL = a stream of the call's own; work queued on `stream` before the call is waited for. */
int orbfe_vocabulary_train_device(const orbfe_vocab_train_config* cfg, const uint8_t* d_desc, const int32_t* d_n, int n_frames, int cap,
                                  void* d_workspace, size_t workspace_bytes, int32_t* d_leaf_node, void* stream,
                                  orbfe_vocab_train_stats* stats, orbfe_vocabulary** vocabulary);
/* Per level of the calling thread's last training call (at most max_levels entries, *n_levels written): wall milliseconds, the
 * association rounds of its slowest node, and how many segments took the wide form, the narrow form and the trivial case. */
int orbfe_debug_vocabulary_train_levels(int max_levels, double* ms, int32_t* rounds, int32_t* wide_segments, int32_t* narrow_segments,
                                        int32_t* trivial_segments, int* n_levels);

/* ------------------------------------------------------------------------------- batched-sequence mode: record gather */
/* Independent frames shard over the GPUs of a node in contiguous chunks of the frame range (the reference
 * walks a sequence one frame at a time in one process, Source/Examples/Stereo/stereo_kitti.cc:88-106): one host thread or
 * process per GPU with its own extractor / matcher handles, no collective inside the step.  The only exchange is the gather
 * of the fixed-size padded records {n[frames]; keypoints[frames][cap]; descriptors[frames][cap][32]} over RCCL (librccl is
 * loaded on first use; ORBFE_ERR_NO_DEVICE without it):
 *   ORBFE_GATHER_ALL   ncclAllGather: every rank receives every rank's records, in rank order = frame order
 *   ORBFE_GATHER_ROOT  grouped ncclSend / ncclRecv: rank 0 alone receives them (the *_all pointers of other ranks may be NULL)
 * `frames` and `cap` are equal on every rank (orbfe_shard_range gives the chunk sizes; pad the short ones).  DEVICE pointers;
 * the collective is enqueued on `stream` (NULL: the handle's own stream, orbfe_gather_sync waits for it) and returns at once.
 * A handle belongs to one device; world = 1 is a valid communicator (the collective degenerates to a copy). */
typedef struct orbfe_gather orbfe_gather;
#define ORBFE_GATHER_ID_BYTES 128
enum { ORBFE_GATHER_ALL = 0, ORBFE_GATHER_ROOT = 1 };
/* [begin, end) of the frames rank `rank` owns: contiguous chunks whose sizes differ by at most one */
int orbfe_shard_range(int n_frames, int rank, int world, int* begin, int* end);
/* one process per GPU: rank 0 makes the id (ncclGetUniqueId) and hands it to the others out of band (MPI, a file, a socket) */
int orbfe_gather_unique_id(uint8_t id[ORBFE_GATHER_ID_BYTES]);
int orbfe_gather_create(const uint8_t* id, int rank, int world, int device, orbfe_gather** out);
/* one process, one host thread per GPU: n_devices handles at once (ncclCommInitAll); devices = NULL: 0 .. n_devices - 1 */
int orbfe_gather_create_all(int n_devices, const int* devices, orbfe_gather** out);
int orbfe_gather_destroy(orbfe_gather* g);
int orbfe_gather_rank(const orbfe_gather* g, int* rank, int* world);
int orbfe_gather_records(orbfe_gather* g, const int32_t* d_n, const orbfe_keypoint* d_kps, const uint8_t* d_desc, int frames,
                         int cap, int mode, int32_t* d_n_all, orbfe_keypoint* d_kps_all, uint8_t* d_desc_all, void* stream);
int orbfe_gather_sync(orbfe_gather* g);

/* ------------------------------------------------------------------------------------------------- warm-up */
/* The first call for an image size builds the plan and its device tables, allocates the work space and the pinned staging
 * buffers, loads the code objects; the third one- or two-image call captures the launch graph.  The reference constructs its
 * extractors once (L/src/Tracking.cc:112-127) and its first Track() already counts (initialisation): do that work when the
 * size is known instead of inside the first frames.  orbfe_extractor_prepare runs the host-API extraction of `n_images`
 * synthetic w x h images four times on handle e (n_images = 1 for ORBextractor::operator(), 2 for a stereo pair through
 * orbfe_extract_batch).  orbfe_frontend_prepare does that for both eyes (right may be NULL: monocular) and, ON THE CALLING
 * THREAD (the handle-less matcher entry points work on a per-thread handle), one stereo pair through orbfe_stereo_match and
 * the two SearchByProjection forms with max_queries queries (<= 0: one per keypoint).  Without them everything still happens
 * on first use.  HOST work only besides the calls themselves; synchronous. */
int orbfe_extractor_prepare(orbfe_extractor* e, int w, int h, int n_images);
int orbfe_frontend_prepare(orbfe_extractor* left, orbfe_extractor* right, int w, int h, int max_queries);

/* ------------------------------------------------------------------------------- batched stereo pipeline for a C / C++ host */
/* The batched-sequence mode (north_star) for a host that does not link the HIP runtime: the whole per-chunk step of
 * `examples/stereo_kitti.py` / `bench.py` -- images H2D, ORBextractor left + right (L/src/ORBextractor.cc:978-1039), Frame::
 * ComputeStereoMatches (L/src/Frame.cc:477-646), Frame::UnprojectStereo of every stereo point (:668-679), its projection into the
 * next frame and SearchByProjection(cur, last) (L/src/ORBmatcher.cc:1247-1383), results D2H -- behind one handle that owns the
 * extractors and matchers (one set per slot), `slots` sets of pinned host and device buffers and its streams -- copy in, left extractor,
 * right extractor (two streams, as the reference's two threads), the matching half (stereo match ... projection search), copy out; the
 * extraction of chunk k + 1 runs beside the matching half of chunk k (DESIGN lesson 47):
 *     orbfe_pipeline_input(p, s, &in)     pinned, pitched host images of slot s (+ the per-frame camera / pose records, pre-filled
 *                                         with the identity pose and the configured intrinsics); the host decodes into them
 *     orbfe_pipeline_submit(p, s, n, hp)  enqueues the chunk (n <= batch frames; hp = 0: frame 0 has no predecessor) and returns
 *     orbfe_pipeline_wait(p, s)           blocks until slot s's results are in its pinned output block
 *     orbfe_pipeline_output(p, s, &out)   the block: counts, keypoints, descriptors, mvuRight / mvDepth, tracked assignments
 * Chunks are processed in submit order; frame 0 of a chunk is searched with the points of the last frame of the previous one.  With
 * two slots the H2D copy of chunk k + 1 and the D2H copy of chunk k - 1 run beside the kernels of chunk k.  The left records of a
 * slot stay in HBM for orbfe_gather_records (orbfe_pipeline_device_records, enqueue it on orbfe_pipeline_stream) until the slot is
 * submitted again.  One host thread per handle at a time; one handle per GPU (orbfe_set_device before orbfe_pipeline_create, or
 * device >= 0). */
typedef struct orbfe_pipeline orbfe_pipeline;
typedef struct orbfe_pipeline_config {
  orbfe_params extractor;          /* both eyes */
  int32_t width, height;
  int32_t batch;                   /* stereo frames per chunk */
  int32_t slots;                   /* buffer sets, 1 .. 4 */
  float fx, fy, cx, cy, bf;        /* Camera.fx .. Camera.bf of the settings file (bf = baseline x fx) */
  float th;                        /* SearchByProjection window factor (7 for stereo, L/src/Tracking.cc:793-798) */
  int32_t check_orientation;       /* ORBmatcher(0.9, true) */
  int32_t output_mask;             /* which blocks of a chunk's results are copied to the slot's pinned host block: 0 = all of them, else
                                      an OR of ORBFE_PIPE_OUT_*; the per-frame counts (n_left, n_right, n_stereo, n_tracked) always are.
                                      A consumer that reads only the matches pays for 4 bytes per keypoint row instead of 72 (37 MB per
                                      256-frame KITTI chunk otherwise); everything stays available in HBM (orbfe_pipeline_device_records) */
} orbfe_pipeline_config;
#define ORBFE_PIPE_OUT_KEYPOINTS 1
#define ORBFE_PIPE_OUT_DESCRIPTORS 2
#define ORBFE_PIPE_OUT_STEREO 4        /* u_right, depth */
#define ORBFE_PIPE_OUT_ASSIGNED 8
#define ORBFE_PIPE_OUT_COUNTS 16       /* nothing but the counts */
typedef struct orbfe_pipeline_input_view {
  uint8_t* left; uint8_t* right;   /* frame f at + f * image_bytes, rows `pitch` bytes apart (pitch = width rounded up to 64) */
  int32_t pitch; size_t image_bytes;
  orbfe_unproject_cam* cams;       /* [batch]: Frame::UnprojectStereo's camera of frame f */
  orbfe_track_pose* poses;         /* [batch]: CurrentFrame members of frame f for the projection of frame f - 1's points */
} orbfe_pipeline_input_view;
typedef struct orbfe_pipeline_output_view {
  int32_t cap;                     /* keypoint rows per frame */
  const int32_t* n_left;           /* [batch] */
  const orbfe_keypoint* kps_left;  /* [batch][cap] */
  const uint8_t* desc_left;        /* [batch][cap][32] */
  const int32_t* n_right;          /* [batch] */
  const float* u_right;            /* [batch][cap] mvuRight (-1: none) */
  const float* depth;              /* [batch][cap] mvDepth */
  const int32_t* n_stereo;         /* [batch] */
  const int32_t* assigned;         /* [batch][cap]: index of the last frame's point matched to keypoint i, or -1 */
  const int32_t* n_tracked;        /* [batch]: SearchByProjection's return value */
} orbfe_pipeline_output_view;
int orbfe_pipeline_create(const orbfe_pipeline_config* cfg, int device, orbfe_pipeline** out);
int orbfe_pipeline_destroy(orbfe_pipeline* p);
int orbfe_pipeline_input(orbfe_pipeline* p, int slot, orbfe_pipeline_input_view* in);
int orbfe_pipeline_submit(orbfe_pipeline* p, int slot, int n_frames, int has_predecessor);
int orbfe_pipeline_wait(orbfe_pipeline* p, int slot);
int orbfe_pipeline_output(orbfe_pipeline* p, int slot, orbfe_pipeline_output_view* out);
/* For producers that already are on the device (a decoder on the GPU, frames from a neighbour over xGMI): the slot's DEVICE image
 * blocks (n-th image at + n * image_bytes, rows `pitch` bytes apart; write them on a stream of your own and synchronise it before the
 * submit, and not before orbfe_pipeline_wait of the slot's previous chunk), and a submit that leaves them as they are -- only the
 * camera / pose records go host to device.  Also what a host uses to run the handle at its kernels' rate on frames uploaded once. */
int orbfe_pipeline_device_input(orbfe_pipeline* p, int slot, uint8_t** d_left, uint8_t** d_right, int* pitch, size_t* image_bytes);
int orbfe_pipeline_submit_resident(orbfe_pipeline* p, int slot, int n_frames, int has_predecessor);
/* Raw (unrectified) stereo input, e.g. EuRoC: an optional rectification stage in front of the extractors.  Called after
 * orbfe_pipeline_create and before the first submit (afterwards: ORBFE_ERR_INVALID); both rectifiers live on the handle's device and
 * their source AND destination sizes equal the pipeline's width x height (the input slots keep their geometry).  From then on the
 * images of orbfe_pipeline_input / orbfe_pipeline_device_input are RAW: each eye's chunk is rectified on that eye's extractor stream
 * into a device block of its own (one more per slot and eye), which the extractor reads.  The rectifiers stay the caller's and must
 * outlive the handle.  Without this call the handle allocates and does exactly what it does without it. */
int orbfe_pipeline_set_rectifiers(orbfe_pipeline* p, orbfe_rectifier* left, orbfe_rectifier* right);
/* DEVICE pointers of slot s's left records ([batch] counts -- rows behind n_frames are zero --, [batch][cap] keypoints and
 * descriptors), valid from the slot's submit until its next submit, ordered on orbfe_pipeline_stream */
int orbfe_pipeline_device_records(orbfe_pipeline* p, int slot, const int32_t** d_n, const orbfe_keypoint** d_kps,
                                  const uint8_t** d_desc, int* cap);
void* orbfe_pipeline_stream(orbfe_pipeline* p);   /* the compute stream (a hipStream_t) */
/* A/B knob of tools/pipeline_rate.py: which stream -> priority level / creation order layout the NEXT orbfe_pipeline_create uses
 * (0 .. 4, see csrc/pipeline.cpp:pipeline_build; the default is the fastest measured).  Results do not depend on it. */
int orbfe_debug_pipeline_streams(int layout);
/* orbfe_gather_records of slot s's left records (`batch` frames of `cap` rows each, every rank alike) on a stream of the
 * pipeline's own, behind the slot's kernels: the collective overlaps the next chunk's kernels and the slot's next submit waits
 * for it.  Every rank calls it once per chunk, in chunk order (a rank whose shard has ended submits empty chunks).  The *_all
 * buffers are the caller's (orbfe_device_malloc); orbfe_pipeline_gather_wait blocks until they are filled. */
int orbfe_pipeline_gather(orbfe_pipeline* p, int slot, orbfe_gather* g, int mode, int32_t* d_n_all, orbfe_keypoint* d_kps_all,
                          uint8_t* d_desc_all);
int orbfe_pipeline_gather_wait(orbfe_pipeline* p, int slot);

/* ---- Initializer (L/src/Initializer.cc) ---------------------------------------------------------------------------------------------
 * The two-view geometry between orbfe_search_for_initialization and a first monocular map (Tracking.cc:505-565): H hypotheses of
 * a homography and of a fundamental matrix from eight matches each (ComputeH21 / ComputeF21, :218-292), scored over all matches
 * (CheckHomography / CheckFundamental, :294-459); the first maximum per model, RH = SH / (SH + SF), H when RH > 0.40; then the
 * eight Faugeras motions (ReconstructH, :562-721) or the four of DecomposeE (ReconstructF, :461-560), each triangulated over the
 * model's inliers (CheckRT, :785-899), and the acceptance rules.  One call is five launches without a host round trip.
 * The caller draws the sets of eight (:80-93; initializer.py: draw_sets); the library holds no random state.
 * csrc/initializer_internal.h states the arithmetic once.  cv::SVDecomp, cv::Mat::inv and cv::determinant are not available where
 * this library is built: the null vector of the 16x9 / 8x9 system and the 3x3 decompositions come from this
 * project's own one-sided Jacobi in double on the float entries, rounded to float; inv and determinant of a 3x3 are the cofactor
 * forms in double.  The sign of a null vector changes no decision (ratios in CheckHomography, squares in CheckFundamental, ratios
 * of singular values, det U * det Vt and both signs of t behind them); it is fixed so that bytes are deterministic.  The ORDER of
 * the motion candidates depends on such signs, their set does not.
 * Normalize (:739-783) sums in float in index order over ALL keypoints of a frame; T1 / T2 are bit-equal to that reading.
 * Where the reference is undefined this library is defined: SH = SF = 0 (the reference passes an empty cv::Mat on and throws) gives
 * model 0; fewer than 8 matches (Tracking asks for 100) gives model 0 and launches nothing; a NaN cosine among the good points
 * (std::sort's behaviour is undefined) sorts last.
 * Deterministic: no float atomics, a problem's bytes do not depend on P or its place in the batch, hypothesis h's record and
 * words do not depend on H.  No CPU fallback. */
#define ORBFE_INIT_MAX_MATCHES 4096      /* keypoints of either frame, hence matches: mpIniORBextractor extracts 2 * nFeatures; 16 bytes
                                            a match, 64 KiB = the LDS a workgroup stages them in */
#define ORBFE_INIT_MAX_HYPOTHESES 1024   /* per model; the reference uses 200 */
typedef struct orbfe_init_params {
  float fx, fy, cx, cy;                  /* mK */
  float sigma;                           /* mSigma (Tracking: 1.0) */
  float min_parallax;                    /* degrees (Initialize: 1.0) */
  int32_t min_triangulated;              /* (Initialize: 50) */
  int32_t reserved;
} orbfe_init_params;                     /* 32 bytes */
typedef struct orbfe_init_hypothesis {
  float M[9];                            /* H21i or F21i row-major, in pixel coordinates */
  float score;                           /* currentScore */
  int32_t n_inliers;                     /* set bits of its words */
  int32_t status;                        /* 1 evaluated; 0: the set is no draw of :80-93 (an index outside [0, N) or a repeated one) and
                                            the whole record and its words are zero */
  int32_t reserved[4];
} orbfe_init_hypothesis;                 /* 64 bytes */
typedef struct orbfe_init_candidate {
  float R[9], t[3];                      /* one motion of DecomposeE / Faugeras */
  int32_t n_good;                        /* CheckRT's return value */
  float parallax;                        /* degrees */
  int32_t reserved[2];
} orbfe_init_candidate;                  /* 64 bytes */
/* orbfe_init_result.reason: one bit per condition that failed (0 on success) */
#define ORBFE_INIT_FEW_MATCHES 1         /* fewer than 8 matches: no set of eight exists (not a reference exit, Tracking.cc:529 asks for 100) */
#define ORBFE_INIT_NO_MODEL 2            /* SH == 0 and SF == 0, or no hypothesis at all: RH is 0 / 0 (:110) */
#define ORBFE_INIT_H_DEGENERATE 4        /* :590  d1 / d2 < 1.00001 || d2 / d3 < 1.00001 */
#define ORBFE_INIT_F_FEW_GOOD 8          /* :516  maxGood < nMinGood */
#define ORBFE_INIT_F_SIMILAR 16          /* :516  nsimilar > 1 */
#define ORBFE_INIT_F_PARALLAX 32         /* :522, :531, :540, :549  parallax of the first best candidate not > minParallax */
#define ORBFE_INIT_H_SECOND 64           /* :710  not secondBestGood < 0.75 * bestGood */
#define ORBFE_INIT_H_PARALLAX 128        /* :710  not bestParallax >= minParallax */
#define ORBFE_INIT_H_MIN_TRIANGULATED 256 /* :711  not bestGood > minTriangulated */
#define ORBFE_INIT_H_FEW_GOOD 512        /* :711  not bestGood > 0.9 * N */
typedef struct orbfe_init_result {
  int32_t model;                         /* 0 none, 1 homography, 2 fundamental */
  int32_t success;                       /* Initialize's return value */
  int32_t reason;                        /* ORBFE_INIT_* bits */
  int32_t best_h, best_f;                /* first hypothesis with the maximal score > 0 per model, or -1 */
  float score_h, score_f, rh;            /* SH, SF, RH (0 where undefined) */
  int32_t n_matches;                     /* N = mvMatches12.size() */
  int32_t n_inliers;                     /* of the chosen model: N of ReconstructF / ReconstructH */
  int32_t n_candidates;                  /* 4 (F), 8 (H), 0 when none was built */
  int32_t best_candidate;                /* F: the first with maxGood; H: bestSolutionIdx; -1 without one */
  int32_t n_good;                        /* maxGood / bestGood */
  int32_t second_good_or_n_similar;      /* H: secondBestGood; F: nsimilar */
  float parallax;                        /* of best_candidate */
  int32_t n_triangulated;                /* set bits of the triangulated words (0 without success) */
  float H21[9], F21[9];                  /* the two winners (zero without one) */
  float R21[9], t21[3];                  /* zero without success */
  float norm1[4], norm2[4];              /* Normalize of the two frames: meanX, meanY, sX, sY (T = [sX 0 -meanX * sX; 0 sY -meanY * sY; 0 0 1]) */
  int32_t reserved[2];
} orbfe_init_result;                     /* 224 bytes */
/* Initializer::Initialize on host arrays, synchronous: one packed upload, five launches, one packed download.
 * keys1[n1] / keys2[n2]: (x, y) of mvKeysUn of the reference and the current frame; matches12[n1]: index into keys2 or < 0; sets[H][8]:
 * indices into the match list (the pairs (i, matches12[i]) with matches12[i] >= 0, in order of i).
 * Outputs: *result; P3D[n1][3] (zero rows where the reference leaves cv::Point3f's default; all zero without success);
 * triangulated[ceil(n1 / 64)] (bit i = vbTriangulated[i]); inlier_words[ceil(N / 64)] sized for ceil(n1 / 64) (the chosen model's
 * vbMatchesInliers over the match list; zero for model 0).  Optional (NULL to skip): hyps_h / hyps_f [H], words_h / words_f
 * [H][ceil(n1 / 64)] (row stride ceil(n1 / 64) words, the first ceil(N / 64) used), candidates[8].
 * Limits (ORBFE_ERR_INVALID): 0 <= n1, n2 <= ORBFE_INIT_MAX_MATCHES, 0 <= H <= ORBFE_INIT_MAX_HYPOTHESES, matches12[i] < n2, null
 * pointers.  A set that is no draw yields a zero record (status 0) and reads nothing outside its problem. */
int orbfe_initializer_initialize(const orbfe_init_params* params, const float* keys1, int n1, const float* keys2, int n2,
                                 const int32_t* matches12, const int32_t* sets, int H, orbfe_init_result* result, float* P3D,
                                 uint64_t* triangulated, uint64_t* inlier_words, orbfe_init_hypothesis* hyps_h,
                                 orbfe_init_hypothesis* hyps_f, uint64_t* words_h, uint64_t* words_f, orbfe_init_candidate* candidates);
/* Bytes of the workspace of orbfe_initializer_initialize_batch_device for P problems of at most `cap` keypoints a frame.
 * Limits (ORBFE_ERR_INVALID): 0 <= P <= 65 535, 1 <= cap <= ORBFE_INIT_MAX_MATCHES, bytes != NULL. */
int orbfe_initializer_workspace_bytes(int P, int cap, size_t* bytes);
/* P ragged problems from device memory on `stream` (NULL: the NULL stream), asynchronous.  d_params [P]; d_keys1 / d_keys2
 * [P][cap][2]; d_n1 / d_n2 [P] (clamped to [0, cap]); d_matches12 [P][cap] (an entry >= n2 counts as no match); d_sets
 * [P][h_cap][8]; d_H [P] (clamped to [0, h_cap]).  Outputs, all required: d_result [P]; d_P3D [P][cap][3]; d_triangulated and
 * d_inlier_words [P][W], W = ceil(cap / 64); d_hyps [P][2][h_cap] and d_words [P][2][h_cap][W] (model H first); d_candidates [P][8].
 * A problem's bytes equal the host form's on the same problem (rows and words behind a problem's counts are not written, except
 * P3D and the two word rows, which are written for all of n1).  One exception: for a problem with fewer than 8 matches no hypothesis
 * is evaluated and its rows of d_hyps / d_words are left as they were, where the host form hands back zeros; its result record, P3D,
 * word rows and candidates are the host form's.
 * Limits (ORBFE_ERR_INVALID): 0 <= P <= 65 535 (0: nothing is launched), 1 <= cap <= ORBFE_INIT_MAX_MATCHES, 1 <= h_cap <=
 * ORBFE_INIT_MAX_HYPOTHESES, workspace_bytes below orbfe_initializer_workspace_bytes(P, cap), null pointers, pointers not 4-byte
 * (words, workspace: 8-byte) aligned. */
int orbfe_initializer_initialize_batch_device(int P, const orbfe_init_params* d_params, const float* d_keys1, const int32_t* d_n1,
                                              const float* d_keys2, const int32_t* d_n2, int cap, const int32_t* d_matches12,
                                              const int32_t* d_sets, const int32_t* d_H, int h_cap, orbfe_init_result* d_result,
                                              float* d_P3D, uint64_t* d_triangulated, uint64_t* d_inlier_words,
                                              orbfe_init_hypothesis* d_hyps, uint64_t* d_words, orbfe_init_candidate* d_candidates,
                                              void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- Tracking::CreateInitialMapMonocular (L/src/Tracking.cc:546-666) -----------------------------------------------------------------
 * From the outputs of the initialiser above to a first map at the scale the rest of the system works in, in three launches without a
 * host round trip:
 *   build    Tracking.cc:551-556, :584-612: every match i with matches12[i] in [0, n2) and vbTriangulated[i] becomes a map point at
 *            P3D[i], in order of i (its place is the popcount prefix over the words), with two monocular observations: keypoint i of
 *            the initial keyframe (pose1, id 0, fixed) and keypoint matches12[i] of the current one (pose [R21 | t21], free)
 *   adjust   GlobalBundleAdjustemnt(map, n_iterations): ba_kernel above, robust
 *   finish   :620-642: z = Rcw2.dot(x) + zcw of every point in the initial keyframe as a float (cv::Mat::dot accumulates in double in
 *            element order, the sum with zcw is a double, rounded once -- this project's restatement); the depths
 *            sorted, the element at (n - 1) / q; a reset if that median is < 0 or fewer than min_points keypoints of the current
 *            keyframe hold a point (TrackedMapPoints(1)); otherwise the current translation and every point times 1.0f / median
 * Defined where the reference is not: without any point the reference indexes an empty vector -- here a reset with
 * ORBFE_IMAP_NO_POINTS and median_depth 0; a NaN depth sorts last (std::sort is undefined on it), -0 before +0; a median of 0 is no
 * reset and scales by 1.0f / 0 as the float arithmetic has it.  On a reset poses and points are the adjustment's, unscaled.
 * Not taken over: ComputeBoW, the map bookkeeping of :573-612 and :644-665, UpdateNormalAndDepth inside the adjustment
 * (orbfe_refresh_map_points), the stop flag.
 * Deterministic: no atomics; a problem's bytes do not depend on P or on its place in the batch.  No CPU fallback.
 * Limits: ORBFE_INIT_MAX_MATCHES keypoints a frame, ORBFE_LBA_MAX_PROBLEMS problems, 1 <= n_iterations <= ORBFE_BA_MAX_ITERATIONS. */
#define ORBFE_IMAP_MEDIAN_NEGATIVE 1     /* reason bits: medianDepth < 0 */
#define ORBFE_IMAP_FEW_POINTS 2          /* TrackedMapPoints(1) < min_points */
#define ORBFE_IMAP_NO_POINTS 4           /* no match was triangulated */
#define ORBFE_IMAP_REFUSED 8             /* an octave outside the camera's levels: the adjustment refused the problem (ba.rounds = -1) */
typedef struct orbfe_initial_map_result { /* 72 bytes, 8-byte aligned */
  int32_t n_points;                      /* map points = entries of the index list */
  int32_t tracked;                       /* keypoints of the current keyframe that hold a point */
  float median_depth;                    /* before the rescale; 0 without a point */
  int32_t success;                       /* 1: the map stands and is scaled; 0: Tracking resets */
  int32_t reason;                        /* ORBFE_IMAP_* bits, 0 on success */
  int32_t reserved[3];
  orbfe_ba_result ba;                    /* of the adjustment */
} orbfe_initial_map_result;
/* One problem on host arrays, synchronous: one packed upload, three launches, one packed download.  camera: fx fy cx cy, n_levels
 * and inv_level_sigma2 are read; keys1[n1][2], keys2[n2][2], matches12[n1], P3D[n1][3], triangulated[ceil(n1 / 64)] and init (R21, t21
 * are read) as orbfe_initializer_initialize takes and leaves them; octaves1[n1] / octaves2[n2]: the octave of every keypoint;
 * pose1[12]: the initial keyframe's [R | t], NULL for Tracking's identity; q and min_points: Tracking's 2 and 100.
 * Outputs: poses[2][12]; points[n1][3] in match-index order, zero rows where there is no point; index[n1]: the first n_points
 * entries are the matches that became points, the rest -1; poses_ba / points_ba (NULL to skip): the same two arrays before the
 * rescale; *result.
 * Limits (ORBFE_ERR_INVALID): 0 <= n1, n2 <= ORBFE_INIT_MAX_MATCHES, 1 <= n_iterations <= ORBFE_BA_MAX_ITERATIONS, q >= 1, min_points
 * >= 0, matches12[i] < n2, an octave of a keypoint that is used outside [0, n_levels), null pointers. */
int orbfe_create_initial_map(const orbfe_pose_camera* camera, const float* keys1, int n1, const float* keys2, int n2,
                             const int32_t* matches12, const float* P3D, const uint64_t* triangulated, const orbfe_init_result* init,
                             const int32_t* octaves1, const int32_t* octaves2, const float* pose1, int n_iterations, int q,
                             int min_points, float* poses, float* points, int32_t* index, float* poses_ba, float* points_ba,
                             orbfe_initial_map_result* result);
/* Bytes of the workspace of orbfe_create_initial_map_batch_device for P problems of at most `cap` keypoints a frame.
 * Limits (ORBFE_ERR_INVALID): 0 <= P <= ORBFE_LBA_MAX_PROBLEMS, 1 <= cap <= ORBFE_INIT_MAX_MATCHES, bytes != NULL. */
int orbfe_initial_map_workspace_bytes(int P, int cap, size_t* bytes);
/* P problems from device memory on `stream` (NULL: the NULL stream), asynchronous.  d_keys1 .. d_init lie exactly as
 * orbfe_initializer_initialize_batch_device reads and writes them ([P][cap][2], [P], [P][cap], [P][cap][3], [P][ceil(cap / 64)],
 * [P]), so the two calls chain on one stream; d_octaves1 / d_octaves2 [P][cap]; d_pose1 [P][12] or NULL; one camera for all.
 * Outputs: d_poses [P][2][12], d_points [P][cap][3] and d_index [P][cap] (rows below n1 are written), d_poses_ba / d_points_ba the
 * same or NULL, d_result [P].  A problem with an octave outside the camera's levels is a reset with ORBFE_IMAP_REFUSED.
 * Limits (ORBFE_ERR_INVALID): as above, workspace_bytes below orbfe_initial_map_workspace_bytes(P, cap), a workspace not 256-byte
 * aligned, null pointers, pointers not 4-byte (words, d_result: 8-byte) aligned. */
int orbfe_create_initial_map_batch_device(int P, const orbfe_pose_camera* d_camera, const float* d_keys1, const int32_t* d_n1,
                                          const float* d_keys2, const int32_t* d_n2, int cap, const int32_t* d_matches12,
                                          const float* d_P3D, const uint64_t* d_triangulated, const orbfe_init_result* d_init,
                                          const int32_t* d_octaves1, const int32_t* d_octaves2, const float* d_pose1, int n_iterations,
                                          int q, int min_points, float* d_poses, float* d_points, int32_t* d_index, float* d_poses_ba,
                                          float* d_points_ba, orbfe_initial_map_result* d_result, void* d_workspace,
                                          size_t workspace_bytes, void* stream);

/* ---- Optimizer::OptimizeEssentialGraph (L/src/Optimizer.cc:1366, :760-1043, :1052-1362) and the map correction behind it --------------
 * The pose graph of LoopClosing::CorrectLoop: one vertex per keyframe, one edge per spanning-tree, loop and strong covisibility link
 * and per loop connection, information the identity, no robust kernel, ONE optimize(20) of g2o's Levenberg with
 * setUserLambdaInit(1e-16) and at most 10 trials per iteration; fixed vertices and vertices without an edge are left out of the
 * system and keep their record byte for byte.  Without ORBFE_EG_FIX_SCALE it is the 7-DoF form: VertexSim3Expmap, EdgeSim3, error
 * (C * Si * Sj^-1).log(), the NUMERIC Jacobian of G/core/base_fixed_sized_edge.hpp (central differences, step 1e-9: G2O_SIM3_JACOBIAN is
 * defined nowhere in the reference).  With it, the 6-DoF form the reference adds for stereo and RGB-D: VertexSE3Expmap, EdgeSE3Expmap,
 * error (Tj^-1 * C * Ti).log(), the analytic Jacobian of G/types/sba/edge_se3_expmap.cpp.  csrc/egraph_internal.h states the
 * arithmetic once, all in double; the Levenberg rules are csrc/lm_internal.h's.
 * The measurement of an edge is computed once per edge by the kernel: Scw[j] * Scw[i]^-1 for a loop connection, Snc[j] * Snc[i]^-1 for
 * every other edge.
 * The solve: SimplicialLLT with its AMD ordering becomes an unpivoted block L L^T on the ROW ENVELOPE of the free vertices IN THE
 * CALLER'S VERTEX ORDER: the vertex order is the elimination order.  Row r of the factor is stored from the first free vertex it
 * shares an edge with up to its diagonal, and a Cholesky factor never fills outside that envelope.  Keyframes ascending by mnId is
 * what keeps it small: a spanning tree and covisibility links join keyframes of nearby ids, so the envelope is a band plus the few
 * rows that carry a loop edge.  No fill-reducing reordering is applied.  A pivot that is not > 0 fails the trial (g2o's ok2 = false):
 * the estimates are left alone, lambda grows, and ORBFE_EG_FACTOR_FAILED is reported in the result's status.
 * One workgroup per problem here; ONE graph across the whole device is orbfe_essential_graph_grid below, which gives the same bytes
 * and takes envelopes 32 times as large.  Deterministic: no floating-point atomics, every
 * sum has one owner that walks a sorted list; a problem's bytes depend on its own rows only.  No CPU fallback.
 * Limits, each refused with ORBFE_ERR_INVALID one step past it (a per-problem ORBFE_EG_REFUSED on the batch form; pinned by
 * tests/test_egraph_cpu.py and tests/test_egraph_gpu.py):
 *   ORBFE_EG_MAX_KEYFRAMES        32 768 vertices: the keyframe-row limit of the covisibility graph whose links the edges are
 *   ORBFE_EG_MAX_EDGES            262 144 edges: 113 doubles of workspace an edge (measurement, error, both Jacobians) -- 237 MB
 *   ORBFE_EG_MAX_ENVELOPE_BLOCKS  131 072 blocks of 7 x 7 doubles: 51 MB of workspace, its elements indexed in 32 bits, and the ONE
 *                                 workgroup walks the blocks of a row one after the other -- about half a second per trial for
 *                                 the 77 000 blocks of 2 000 keyframes in a band of 20 with 30 loop rows
 *                                 (profiles/essential_graph.md)
 *   ORBFE_EG_MAX_PROBLEMS         65 535 problems per launch
 *   records                       finite, s > 0, a quaternion of non-zero norm; with ORBFE_EG_FIX_SCALE |s - 1| <= 1e-3 for every
 *                                 record and every derived measurement (the reference throws there, Optimizer.cc:1057-1067) */
#define ORBFE_EG_MAX_KEYFRAMES 32768
#define ORBFE_EG_MAX_EDGES 262144
#define ORBFE_EG_MAX_ENVELOPE_BLOCKS 131072
#define ORBFE_EG_MAX_PROBLEMS 65535
#define ORBFE_EG_FIX_SCALE 1              /* flags: bFixScale -- the SE3 form */
#define ORBFE_EG_NORMAL 0                 /* edge kinds: spanning tree, old loop edge, covisibility (Optimizer.cc:1191-1286) */
#define ORBFE_EG_LOOP_CONNECTION 1        /* an entry of LoopConnections (:1146-1183) */
#define ORBFE_EG_DONE 0                   /* status of a result */
#define ORBFE_EG_FACTOR_FAILED 1          /* at least one trial met a pivot that was not > 0 */
#define ORBFE_EG_REFUSED (-1)             /* batch form: the problem breaks a limit; nothing of it was optimised */
typedef struct orbfe_eg_sim3 {            /* g2o::Sim3's own fields; 64 bytes */
  double q[4];                            /* x y z w */
  double t[3];
  double s;
} orbfe_eg_sim3;
typedef struct orbfe_eg_vertex {          /* 136 bytes */
  orbfe_eg_sim3 Scw;                      /* the start estimate and vScw: the CorrectedSim3 entry, else Sim3(Rcw, tcw, 1) */
  orbfe_eg_sim3 Snc;                      /* the NonCorrectedSim3 entry, else equal to Scw */
  uint32_t fixed;                         /* != 0: pLoopKF */
  uint32_t reserved;
} orbfe_eg_vertex;
typedef struct orbfe_eg_edge {            /* 12 bytes */
  int32_t i, j;                           /* vertex 0 and vertex 1 of the g2o edge; i != j */
  uint32_t kind;                          /* ORBFE_EG_NORMAL or ORBFE_EG_LOOP_CONNECTION */
} orbfe_eg_edge;
typedef struct orbfe_eg_problem {         /* where one problem of a batch lies in the batch's arrays; 16 bytes */
  int32_t kf_offset, n_kf;                /* rows of d_vertices / d_sim3_out / d_poses_out */
  int32_t edge_offset, n_edges;           /* rows of d_edges */
} orbfe_eg_problem;
typedef struct orbfe_eg_result {          /* 48 bytes, 8-byte aligned */
  int32_t status;                         /* ORBFE_EG_DONE, ORBFE_EG_FACTOR_FAILED, ORBFE_EG_REFUSED */
  int32_t iterations, trials;             /* Levenberg iterations and trials run (0 without a free vertex with an edge) */
  int32_t n_free;                         /* vertices in the system: not fixed, with an edge */
  int32_t n_edges;
  int32_t envelope_blocks;                /* blocks of the row envelope of this problem */
  double chi2_first, chi2_last;           /* activeChi2 before the first iteration and at the final estimates */
  double lambda;                          /* the final damping */
} orbfe_eg_result;
/* The blocks of the row envelope of a graph: for every vertex that is not fixed and has an edge, one diagonal block and one per free
 * vertex from the earliest it shares an edge with up to itself.  HOST pointers.  fixed[n_kf]: != 0 for a fixed vertex (NULL: none).
 * Limits (ORBFE_ERR_INVALID): the counts within 0 .. ORBFE_EG_MAX_KEYFRAMES / ORBFE_EG_MAX_EDGES, edge indices in range, i != j,
 * null blocks.  The count itself is not limited here. */
int orbfe_essential_graph_envelope_blocks(int n_kf, const uint8_t* fixed, const orbfe_eg_edge* edges, int n_edges, int64_t* blocks);
/* One graph.  HOST pointers, synchronous.  sim3_out[n_kf]: the corrected Siw of every vertex (with ORBFE_EG_FIX_SCALE: the SE3Quat's
 * rotation and translation, s = 1); a vertex that is fixed or has no edge: its Scw as given.  poses_out: n_kf x 12 floats, rows of
 * [R | t / s] as SetPose receives them (:1003-1011; with ORBFE_EG_FIX_SCALE [R | t], :1324-1329).  A problem without a free vertex or
 * without an edge returns its inputs, iterations = 0.  One upload, one launch, one download; the workspace is allocated for the call.
 * Limits (ORBFE_ERR_INVALID): those above, null arrays with a count > 0, null result, flags outside ORBFE_EG_FIX_SCALE. */
int orbfe_essential_graph(const orbfe_eg_vertex* vertices, int n_kf, const orbfe_eg_edge* edges, int n_edges, int flags,
                          orbfe_eg_sim3* sim3_out, float* poses_out, orbfe_eg_result* result);
/* The bytes of workspace a batch of P problems needs whose counts stay within kf_cap vertices, edge_cap edges and env_cap envelope
 * blocks each.  Limits (ORBFE_ERR_INVALID): 0 <= P <= ORBFE_EG_MAX_PROBLEMS, the caps >= 0 and within the ORBFE_EG_MAX_*, null bytes. */
int orbfe_essential_graph_workspace_bytes(int P, int kf_cap, int edge_cap, int env_cap, size_t* bytes);
/* P graphs in one launch, one workgroup each.  DEVICE pointers, asynchronous on `stream` (NULL: the NULL stream).  Problem p lies
 * where d_problems[p] says.  A problem that breaks a limit above, or whose envelope exceeds env_cap, is refused by its workgroup:
 * status ORBFE_EG_REFUSED, its Scw and their poses written through when its rows can be addressed; no other problem is touched.
 * d_workspace: 256-byte aligned, at least what orbfe_essential_graph_workspace_bytes states; its contents mean nothing before or
 * after.  A problem's bytes do not depend on P, on its position or on the run: they are those of the host form. */
int orbfe_essential_graph_batch_device(int P, const orbfe_eg_problem* d_problems, const orbfe_eg_vertex* d_vertices,
                                       const orbfe_eg_edge* d_edges, int kf_cap, int edge_cap, int env_cap, int flags,
                                       orbfe_eg_sim3* d_sim3_out, float* d_poses_out, orbfe_eg_result* d_result, void* d_workspace,
                                       size_t workspace_bytes, void* stream);

/* ---- the same optimisation of ONE graph across the whole device --------------------------------------------------------------------
 * A loop closure has one graph, and one workgroup walks the blocks of its row envelope one after the other (two barriers each).  Here
 * every phase of a trial is a launch over the grid (csrc/egraph_grid_kernels.hip) and the launch boundary is the only grid-wide
 * synchronisation.  The factorisation runs the same up-looking step per block -- a workgroup per block -- level by level: block (r, c)
 * needs row r's blocks before c and the whole of row c, which gives every block a level (csrc/egraph_grid_internal.h; at most
 * 2 n_free + 1 levels, computed once per call on the host from the rows' first blocks), and every level is one launch over its
 * blocks, so every block whose inputs are complete is in flight.  The two triangular solves stay one workgroup in one launch.
 * Records, validation rules, flags and results are those of orbfe_essential_graph, and so are the BYTES of sim3_out, poses_out and
 * the whole result record for a graph both forms take: csrc/egraph_steps.h states every per-item step once for both kernels, every
 * sum keeps its owner and its order, and a one-workgroup control kernel sums the per-edge chi2 and the computeScale terms in the
 * order the one workgroup's lanes would have.  No floating-point atomics, no matrix-core arithmetic, no fill-reducing ordering: the
 * caller's vertex order stays the elimination order.  Both forms are SYNCHRONOUS on their stream: the host reads one control record
 * per trial from pinned memory, at most 20 iterations x 10 trials.  No CPU fallback.
 * Limits, each refused with ORBFE_ERR_INVALID one step past it, before a device is looked for (pinned by
 * tests/test_egraph_grid_cpu.py and tests/test_egraph_grid_gpu.py):
 *   ORBFE_EGRID_MAX_KEYFRAMES        32 768 vertices and
 *   ORBFE_EGRID_MAX_EDGES            262 144 edges: the records and their workspace are those of the one-workgroup form
 *   ORBFE_EGRID_MAX_ENVELOPE_BLOCKS  4 194 304 blocks of 7 x 7 doubles: 1.6 GB of workspace -- the dense envelope of 2 895 free
 *                                    keyframes -- and 34 MB of level plan; block counts stay within 32 bits, element offsets are
 *                                    64-bit
 *   records                          as above */
#define ORBFE_EGRID_MAX_KEYFRAMES 32768
#define ORBFE_EGRID_MAX_EDGES 262144
#define ORBFE_EGRID_MAX_ENVELOPE_BLOCKS 4194304
/* One graph.  HOST pointers, synchronous.  Arguments, results and limits as orbfe_essential_graph's, with
 * ORBFE_EGRID_MAX_ENVELOPE_BLOCKS in place of ORBFE_EG_MAX_ENVELOPE_BLOCKS; the workspace is allocated for the call. */
int orbfe_essential_graph_grid(const orbfe_eg_vertex* vertices, int n_kf, const orbfe_eg_edge* edges, int n_edges, int flags,
                               orbfe_eg_sim3* sim3_out, float* poses_out, orbfe_eg_result* result);
/* The bytes of workspace of a graph of at most kf_cap vertices, edge_cap edges and env_cap envelope blocks
 * (orbfe_essential_graph_envelope_blocks states a graph's).  Monotonic in every cap.
 * Limits (ORBFE_ERR_INVALID): the caps >= 0 and within the ORBFE_EGRID_MAX_*, null bytes. */
int orbfe_essential_graph_grid_workspace_bytes(int kf_cap, int edge_cap, int64_t env_cap, size_t* bytes);
/* The same on DEVICE pointers, SYNCHRONOUS on `stream` (NULL: the NULL stream); the inputs are not modified.  d_workspace: 256-byte
 * aligned; its contents mean nothing before or after.  Its size states the envelope it holds: at least
 * orbfe_essential_graph_grid_workspace_bytes(n_kf, n_edges, 0) bytes or the call is refused with ORBFE_ERR_INVALID, and
 * orbfe_essential_graph_grid_workspace_bytes(n_kf, n_edges, blocks) for a graph of `blocks` envelope blocks.  A graph that breaks a
 * rule only the device can see -- a record or a derived measurement beyond the limits above, an envelope the workspace does not hold
 * or one beyond ORBFE_EGRID_MAX_ENVELOPE_BLOCKS -- comes back with ORBFE_OK, status ORBFE_EG_REFUSED in d_result and its Scw and
 * their poses written through, as the batch form's do.
 * Limits (ORBFE_ERR_INVALID): the counts, flags outside ORBFE_EG_FIX_SCALE, null pointers with a count > 0, null d_result,
 * misaligned records (vertices, sim3_out, result: 8 bytes; the others: 4), a workspace that is null, misaligned or too small. */
int orbfe_essential_graph_grid_device(const orbfe_eg_vertex* d_vertices, int n_kf, const orbfe_eg_edge* d_edges, int n_edges, int flags,
                                      orbfe_eg_sim3* d_sim3_out, float* d_poses_out, orbfe_eg_result* d_result, void* d_workspace,
                                      size_t workspace_bytes, void* stream);
/* Measurement only (tools/egraph_rate.py): copies the calling thread's sums of stream-event times per phase, in milliseconds, to ms
 * (9 floats: prepare, the host's level plan with its two copies, linearise, build, factorisation, solves, update / chi2 / control
 * kernel, control read-back, and last the level count of the latest call; NULL: not copied), clears them, and switches the timing of
 * this thread's later calls of the two forms above on (enable != 0) or off.  Timing synchronises the stream after every phase: the
 * sums are the phases' device times, and a timed call is slower than an untimed one. */
int orbfe_debug_egrid_phases(int enable, float* ms);
/* Test only: the level plan of the factorisation from first[n_free], the first row block of every row's envelope (0 <= first[r] <= r).
 * block_level: one int per envelope block, row by row with columns ascending; *n_levels: the level count.  HOST pointers, no device.
 * Limits (ORBFE_ERR_INVALID): n_free outside 0 .. ORBFE_EGRID_MAX_KEYFRAMES, a first[r] out of range, more than
 * ORBFE_EGRID_MAX_ENVELOPE_BLOCKS blocks, null pointers. */
int orbfe_debug_egrid_level_plan(const int32_t* first, int n_free, int32_t* block_level, int32_t* n_levels);

/* The map correction of OptimizeEssentialGraph (:1014-1042, :1332-1361) and the neighbour propagation of CorrectLoop
 * (L/src/LoopClosing.cc:445-475): points_out[p] = to[ref[p]]^-1 .map( from[ref[p]].map(points[p]) ), with Eigen's quaternion-vector
 * product, the float position widened to double and rounded once to float at the end (Converter::toCvMat).  ref[p] < 0: the point
 * goes through as it is (a bad point, or one CorrectLoop has moved already).  from = vScw (the Scw of the vertices), to = sim3_out of
 * orbfe_essential_graph; n_tables rows each.  One thread per point.  HOST pointers, synchronous.
 * Limits (ORBFE_ERR_INVALID): 0 <= n_points <= 16 777 216, 0 <= n_tables <= ORBFE_EG_MAX_KEYFRAMES, ref[p] < n_tables, null arrays with
 * a count > 0. */
int orbfe_sim3_correct_points(const float* points, int n_points, const int32_t* ref, const orbfe_eg_sim3* from, const orbfe_eg_sim3* to,
                              int n_tables, float* points_out);
/* The same on DEVICE pointers, asynchronous on `stream`: d_to may be the d_sim3_out of orbfe_essential_graph_batch_device, so the chain
 * needs no host round trip.  d_from: `from_stride` bytes apart (sizeof(orbfe_eg_vertex) reads the Scw of a vertex array in place,
 * sizeof(orbfe_eg_sim3) a plain table).  A ref[p] >= n_tables goes through like a negative one (it cannot be checked on the host). */
int orbfe_sim3_correct_points_device(const float* d_points, int n_points, const int32_t* d_ref, const void* d_from, int from_stride,
                                     const orbfe_eg_sim3* d_to, int n_tables, float* d_points_out, void* stream);

/* --------------------------------------------------------------------------------------- sequence driver helpers */
/* Dependency-free PNG input for the dataset drivers (the reference reads with cv::imread(..., IMREAD_UNCHANGED),
 * Source/Examples/Stereo/stereo_kitti.cc:88-89, Source/Examples/RGB-D/rgbd_tum.cc, and converts colour frames in
 * Tracking::GrabImage*, L/src/Tracking.cc:164-178): 8-bit greyscale (+ alpha), or 8-bit RGB(A) converted with cvtColor's
 * RGB2GRAY weights; 16-bit greyscale (TUM depth maps) through orbfe_png_read_gray16; non-interlaced only; zlib only.
 * Images larger than 4095 x 4095 are refused (ORBFE_ERR_INVALID) before anything is allocated; no exception leaves these
 * functions (ORBFE_ERR_ALLOC when the decoder cannot get its memory).  Thread-safe: any number of calls may run at once. */
int orbfe_png_info(const char* path, int* w, int* h);
/* ... with the bit depth (8 / 16) and channel count (1 grey, 2 grey + alpha, 3 RGB, 4 RGBA); any output may be NULL */
int orbfe_png_info2(const char* path, int* w, int* h, int* depth, int* channels);
int orbfe_png_read_gray(const char* path, uint8_t* dst, int stride, int cap_rows, int* w, int* h);
/* Colour files and the settings file's Camera.RGB: the reference converts cv::imread's BGR data with RGB2GRAY when Camera.RGB is 1
 * -- every settings file it ships -- i.e. grey = 0.299 B + 0.587 G + 0.114 R, and with BGR2GRAY (the luminance) when it is 0
 * (L/src/Tracking.cc:164-178).  orbfe_png_read_gray is camera_rgb = 0; pass the file's flag here to get the reference's grey
 * levels (and so its keypoints) on colour input.  Grey files are unaffected. */
int orbfe_png_read_gray2(const char* path, uint8_t* dst, int stride, int cap_rows, int* w, int* h, int camera_rgb);
/* 16-bit greyscale: h rows of w uint16 samples (host byte order), `stride_elems` ELEMENTS apart */
int orbfe_png_read_gray16(const char* path, uint16_t* dst, int stride_elems, int cap_rows, int* w, int* h);

#ifdef __cplusplus
}
#endif
#endif /* ORBFE_H */
