// matcher.cpp -- host side of liborbfe's ORBmatcher path: work-space handle, kernel sequencing, C ABI.
// No CPU fallback: everything that computes runs in the kernel units hamming_, grid_, projection_, bow_ and stereo_kernels.hip.
//
// Reference behaviour (L/ = Source/Libraries/ORB_SLAM2/):
//   DescriptorDistance                         L/src/ORBmatcher.cc:1542-1556
//   SearchByProjection(Frame&, MapPoints)      L/src/ORBmatcher.cc:45-128
//   SearchByProjection(Frame& cur, last)       L/src/ORBmatcher.cc:1247-1383
//   SearchByBoW inner loops                    L/src/ORBmatcher.cc:201-222
//   Frame grid + GetFeaturesInArea             L/src/Frame.cc:250-263,341-410
//   Frame::ComputeStereoMatches                L/src/Frame.cc:477-646
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "host_internal.h"
#include "pipeline_internal.h"
#include "match_internal.h"

int orbfe_internal_pyr_view(const orbfe_extractor* e, PyrView* v, int* n_images);
int orbfe_internal_tables(const orbfe_extractor* e, float* scale, float* inv_scale, int* n_levels, int* device);

#define ORBFE_MAX_CAND 64  // stored candidates per query; longer lists are re-enumerated by the resolver

struct MBuf {
  void* p = nullptr;
  size_t bytes = 0;
};
static int mb_alloc(MBuf& b, size_t bytes) {
  if (b.p && bytes <= b.bytes) return ORBFE_OK;
  if (b.p) HIPCHK(hipFree(b.p));
  b.p = nullptr;
  b.bytes = 0;
  if (bytes < 256) bytes = 256;
  HIPCHK(hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return ORBFE_OK;
}

static int pin_alloc(void*& p, size_t& have, size_t bytes) {
  if (p && bytes <= have) return ORBFE_OK;
  if (p) HIPCHK(hipHostFree(p));
  p = nullptr;
  have = 0;
  bytes = (bytes + 65535) & ~(size_t)65535;
  HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
  have = bytes;
  return ORBFE_OK;
}

struct orbfe_matcher {
  int device = 0;
  hipStream_t stream = nullptr;
  // scratch
  MBuf cell_start, cell_idx, cell_rec, cand, n_cand, push_idx, push_bin, sad, bucket_start, bucket_idx;
  // SearchLocalPoints / the keyframe searches: generated queries
  MBuf lp_q;
  // the one-problem host entry points (HostCall): a device staging block and its pinned host mirror
  MBuf st_in;
  void* h_pin = nullptr;
  size_t h_pin_bytes = 0;
  std::mutex mu;
};

extern "C" int orbfe_matcher_create(int device, orbfe_matcher** out) {
  if (!out) return ORBFE_ERR_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    orbfe_set_error("no HIP device available (liborbfe has no CPU fallback)");
    return ORBFE_ERR_NO_DEVICE;
  }
  if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
  if (device >= ndev) return ORBFE_ERR_INVALID;
  HIPCHK(hipSetDevice(device));
  orbfe_matcher* m = new orbfe_matcher();
  m->device = device;
  hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    orbfe_set_error("hipStreamCreate: %s", hipGetErrorString(e));
    delete m;
    return ORBFE_ERR_HIP;
  }
  *out = m;
  return ORBFE_OK;
}

extern "C" int orbfe_matcher_destroy(orbfe_matcher* m) {
  if (!m) return ORBFE_OK;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  MBuf* bufs[] = {&m->cell_start, &m->cell_idx, &m->cell_rec, &m->cand, &m->n_cand, &m->push_idx, &m->push_bin, &m->sad, &m->bucket_start, &m->bucket_idx,
                  &m->lp_q, &m->st_in};
  for (auto b : bufs)
    if (b->p) (void)hipFree(b->p);
  if (m->h_pin) (void)hipHostFree(m->h_pin);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
  return ORBFE_OK;
}

extern "C" int orbfe_matcher_sync(orbfe_matcher* m) {
  if (!m) return ORBFE_ERR_INVALID;
  HIPCHK(hipStreamSynchronize(m->stream));
  return ORBFE_OK;
}

// ------------------------------------------------------------------------------------------------ Hamming
extern "C" int orbfe_hamming_matrix_device(const uint8_t* d_A, int nA, const uint8_t* d_B, int nB, uint16_t* d_dist,
                                           void* stream) {
  if (!d_A || !d_B || !d_dist || nA < 0 || nB < 0) return ORBFE_ERR_INVALID;
  if (((uintptr_t)d_A & 15) || ((uintptr_t)d_B & 15)) {
    orbfe_set_error("descriptor matrices must be 16-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  orbfe_launch_hamming_matrix(d_A, nA, d_B, nB, d_dist, (hipStream_t)stream);
  return hip_status("kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_hamming_bf_device(const uint8_t* d_A, const int32_t* d_nA, int strideA, int max_nA,
                                       const uint8_t* d_B, const int32_t* d_nB, int strideB, const int32_t* d_groupA,
                                       const int32_t* d_groupB, const uint8_t* d_maskB, int n_sets, orbfe_bf_match* d_out,
                                       void* stream) {
  if (!d_A || !d_B || !d_nA || !d_nB || !d_out || n_sets < 1 || max_nA < 0 || strideA < max_nA) return ORBFE_ERR_INVALID;
  if ((d_groupA == nullptr) != (d_groupB == nullptr) || strideB >= 65536) {
    orbfe_set_error("groupA/groupB must be given together; strideB must be < 65536");
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_A & 15) || ((uintptr_t)d_B & 15)) {
    orbfe_set_error("descriptor matrices must be 16-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  HammingBfParams p{d_A, d_nA, strideA, d_B, d_nB, strideB, d_groupA, d_groupB, d_maskB, d_out};
  orbfe_launch_hamming_bf(p, max_nA, n_sets, (hipStream_t)stream);
  return hip_status("kernel launch failed", hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ projection
static int ensure_proj_scratch(orbfe_matcher* m, int n_frames, int cap, int q_cap) {
  int rc;
  const size_t F = (size_t)n_frames;
  if ((rc = mb_alloc(m->cell_start, F * (GRID_CELLS + 1) * sizeof(int32_t)))) return rc;
  if ((rc = mb_alloc(m->cell_idx, F * cap * sizeof(int32_t)))) return rc;
  if ((rc = mb_alloc(m->cell_rec, F * cap * 16))) return rc;
  if ((rc = mb_alloc(m->cand, F * q_cap * ORBFE_MAX_CAND * sizeof(orbfe_cand)))) return rc;
  if ((rc = mb_alloc(m->n_cand, F * q_cap * sizeof(int32_t)))) return rc;
  if ((rc = mb_alloc(m->push_idx, F * q_cap * sizeof(int32_t)))) return rc;
  if ((rc = mb_alloc(m->push_bin, F * q_cap))) return rc;
  return ORBFE_OK;
}

static void fill_frame_batch(orbfe_matcher* m, FrameBatch& fb, const orbfe_keypoint* d_kps, const uint8_t* d_desc,
                             const int32_t* d_n, const float* d_ur, int cap, float min_x, float max_x, float min_y,
                             float max_y) {
  fb.keys = d_kps;
  fb.desc = d_desc;
  fb.u_right = d_ur;
  fb.n = d_n;
  fb.cell_start = (int32_t*)m->cell_start.p;
  fb.cell_idx = (int32_t*)m->cell_idx.p;
  fb.cell_rec = (uint32_t*)m->cell_rec.p;
  fb.cap = cap;
  fb.min_x = min_x;
  fb.min_y = min_y;
  // mfGridElementWidthInv / HeightInv, L/src/Frame.cc:109-112
  fb.gw_inv = (float)ORBFE_GRID_COLS / (max_x - min_x);
  fb.gh_inv = (float)ORBFE_GRID_ROWS / (max_y - min_y);
}

static int proj_enqueue(orbfe_matcher* m, int n_frames, const orbfe_keypoint* d_kps, const uint8_t* d_desc,
                        const int32_t* d_n, const float* d_ur, int cap, float min_x, float max_x, float min_y,
                        float max_y, const orbfe_query* d_q, const int32_t* d_nq, int q_cap, int mode, float nnratio,
                        int check_ori, uint8_t* d_blocked, int32_t* d_assigned, int32_t* d_nm, bool resolve,
                        hipStream_t s, int th_high = ORBFE_TH_HIGH) {
  if (cap > 9500) {  // blocked[] + two claim buffers (9 bytes per keypoint) live in LDS next to the 64 KiB staging area
    orbfe_set_error("frame capacity %d too large for the LDS-resident resolver state (cap <= 9500)", cap);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_desc & 15) || ((uintptr_t)d_q & 3) || ((uintptr_t)d_kps & 3)) {
    orbfe_set_error("descriptors must be 16-byte aligned, queries/keypoints 4-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  int rc;
  if ((rc = ensure_proj_scratch(m, n_frames, cap, q_cap))) return rc;
  FrameBatch fb;
  fill_frame_batch(m, fb, d_kps, d_desc, d_n, d_ur, cap, min_x, max_x, min_y, max_y);
  QueryBatch qb{d_q, d_nq, q_cap};
  orbfe_launch_grid_build(fb, n_frames, s);
  orbfe_launch_proj_candidates(fb, qb, (orbfe_cand*)m->cand.p, (int32_t*)m->n_cand.p, ORBFE_MAX_CAND, n_frames, s);
  if (resolve)
    orbfe_launch_proj_resolve(fb, qb, (const orbfe_cand*)m->cand.p, (const int32_t*)m->n_cand.p, ORBFE_MAX_CAND, mode,
                              th_high, nnratio, check_ori, d_blocked, d_assigned, d_nm, (int32_t*)m->push_idx.p,
                              (uint8_t*)m->push_bin.p, n_frames, s);
  return hip_status("kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_proj_match_batch_device(orbfe_matcher* m, int n_frames, const orbfe_keypoint* d_kps,
                                             const uint8_t* d_desc, const int32_t* d_n, const float* d_u_right, int cap,
                                             float min_x, float max_x, float min_y, float max_y, const orbfe_query* d_q,
                                             const int32_t* d_nq, int q_cap, int mode, float nnratio,
                                             int check_orientation, uint8_t* d_blocked, int32_t* d_assigned,
                                             int32_t* d_n_matches, void* stream) {
  if (!m || !d_kps || !d_desc || !d_n || !d_q || !d_nq || !d_blocked || !d_assigned || !d_n_matches || n_frames < 1 ||
      cap < 1 || q_cap < 1 || (mode != 0 && mode != 1) || !(max_x > min_x) || !(max_y > min_y))
    return ORBFE_ERR_INVALID;
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  return proj_enqueue(m, n_frames, d_kps, d_desc, d_n, d_u_right, cap, min_x, max_x, min_y, max_y, d_q, d_nq, q_cap, mode,
                      nnratio, check_orientation, d_blocked, d_assigned, d_n_matches, true, s);
}

// Thread-local handle behind the handle-less host entry points (one HIP stream + scratch HBM + pinned staging per calling
// thread).  Not destroyed at thread exit: the HIP runtime may already be gone when thread_local destructors of the main thread
// run.  ORB-SLAM2's three long-lived threads (Tracking, LocalMapping, LoopClosing) hold three of them for the life of the
// process; a caller with transient threads gives the handle back with orbfe_thread_release() before the thread ends.
struct TlsMatcher {
  orbfe_matcher* m = nullptr;
};
static thread_local TlsMatcher t_tls_matcher;
static int tls_matcher(orbfe_matcher** out) {
  TlsMatcher& t = t_tls_matcher;
  if (!t.m) {
    int rc = orbfe_matcher_create(-1, &t.m);
    if (rc) return rc;
  }
  *out = t.m;
  return ORBFE_OK;
}
void orbfe_fuse_release_spare();   // fuse.cpp: what the thread's last fuse batch left for the next
extern "C" int orbfe_thread_release(void) {
  orbfe_fuse_release_spare();
  TlsMatcher& t = t_tls_matcher;
  if (!t.m) return ORBFE_OK;
  orbfe_matcher* m = t.m;
  t.m = nullptr;
  return orbfe_matcher_destroy(m);
}

// ------------------------------------------------------------------------------------------------ HostCall (host_internal.h)
int HostCall::open() {
  int rc;
  if ((rc = tls_matcher(&m))) return rc;
  lk = std::unique_lock<std::mutex>(m->mu);
  HIPCHK(hipSetDevice(m->device));
  if ((rc = mb_alloc(m->st_in, total())) || (rc = pin_alloc(m->h_pin, m->h_pin_bytes, total()))) return rc;
  stream = m->stream;
  d = (uint8_t*)m->st_in.p;
  h = (uint8_t*)m->h_pin;
  return ORBFE_OK;
}

int HostCall::upload(bool through_output) {
  in_flight = true;
  return status(hipMemcpyAsync(d, h, through_output ? total() : in_end(), hipMemcpyHostToDevice, stream));
}

// HOST_COPY_KERNEL: the runtime's device-to-host path costs ~8 us more per call than a copy kernel of four workgroups writing the
// pinned mirror (ComputeStereoMatches 0.088 -> 0.080 ms, SearchByProjection(cur, last) 0.181 -> 0.179 per frame; the same kernel for
// the packed INPUT -- reads over the link -- measured no gain, so the upload is always a DMA copy).
int HostCall::finish(size_t bytes, HostDownload how) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && bytes) {
    if (how == HOST_COPY_KERNEL) {
      orbfe_launch_copy_block(d + out_begin(), h + out_begin(), bytes, 4, stream);
      e = hipGetLastError();
    } else {
      e = hipMemcpyAsync(h + out_begin(), d + out_begin(), bytes, hipMemcpyDeviceToHost, stream);
    }
  }
  const hipError_t e2 = hipStreamSynchronize(stream);   // also on an error: the stream may still read the pinned block
  in_flight = false;
  return status(e != hipSuccess ? e : e2);
}

HostCall::~HostCall() {
  if (in_flight) (void)hipStreamSynchronize(stream);
}

// The input regions of one host frame in front of a projection search: [n, nq | keys | desc | mvuRight], sized for at least one
// keypoint so that an empty frame still hands the kernels addresses inside the block.
struct FrameRegions {
  size_t hdr, keys, desc, ur;
  int cap;
  bool has_ur;
};
static FrameRegions frame_regions(HostCall& c, const orbfe_frame_view* f, bool with_ur) {
  FrameRegions r;
  r.cap = std::max(f->n, 1);
  r.has_ur = with_ur && f->u_right;
  r.hdr = c.in(16);
  r.keys = c.in(sizeof(orbfe_keypoint) * (size_t)r.cap);
  r.desc = c.in((size_t)32 * r.cap);
  r.ur = c.in(r.has_ur ? sizeof(float) * (size_t)r.cap : 0);
  return r;
}
static void frame_fill(const HostCall& c, const FrameRegions& r, const orbfe_frame_view* f, int nq) {
  c.host<int32_t>(r.hdr)[0] = f->n;
  c.host<int32_t>(r.hdr)[1] = nq;
  if (f->n == 0) return;
  memcpy(c.host(r.keys), f->keys_un, sizeof(orbfe_keypoint) * (size_t)f->n);
  memcpy(c.host(r.desc), f->desc, (size_t)32 * f->n);
  if (r.has_ur) memcpy(c.host(r.ur), f->u_right, sizeof(float) * (size_t)f->n);
}
static const int32_t* frame_n(const HostCall& c, const FrameRegions& r) { return c.dev<const int32_t>(r.hdr); }
static const int32_t* frame_nq(const HostCall& c, const FrameRegions& r) { return c.dev<const int32_t>(r.hdr) + 1; }

static bool frame_ok(const orbfe_frame_view* f) {
  if (f && f->n > 65535) {   // keypoint indices travel as 16-bit fields next to the distance
    orbfe_set_error("frame of %d keypoints: at most 65535", f->n);
    return false;
  }
  return f && f->n >= 0 && (f->n == 0 || (f->keys_un && f->desc)) && f->max_x > f->min_x && f->max_y > f->min_y;
}

extern "C" int orbfe_proj_candidates(const orbfe_frame_view* f, const orbfe_query* q, int nq, orbfe_cand* cand,
                                     int32_t* n_cand, int max_cand) {
  if (!frame_ok(f) || nq < 0 || (nq > 0 && (!q || !cand || !n_cand)) || max_cand < 1) return ORBFE_ERR_INVALID;
  if (nq == 0) return ORBFE_OK;
  HostCall c("orbfe_proj_candidates");
  const FrameRegions fr = frame_regions(c, f, true);
  const size_t b_cand = sizeof(orbfe_cand) * (size_t)nq * max_cand;
  const size_t o_q = c.in(sizeof(orbfe_query) * (size_t)nq), o_cand = c.out(b_cand), o_nc = c.out(sizeof(int32_t) * (size_t)nq);
  int rc;
  if ((rc = c.open()) || (rc = ensure_proj_scratch(c.m, 1, fr.cap, nq))) return rc;
  frame_fill(c, fr, f, nq);
  memcpy(c.host(o_q), q, sizeof(orbfe_query) * (size_t)nq);
  if ((rc = c.upload())) return rc;
  FrameBatch fb;
  fill_frame_batch(c.m, fb, c.dev<const orbfe_keypoint>(fr.keys), c.dev(fr.desc), frame_n(c, fr), fr.has_ur ? c.dev<const float>(fr.ur) : nullptr,
                   fr.cap, f->min_x, f->max_x, f->min_y, f->max_y);
  QueryBatch qb{c.dev<const orbfe_query>(o_q), frame_nq(c, fr), nq};
  orbfe_launch_grid_build(fb, 1, c.stream);
  orbfe_launch_proj_candidates(fb, qb, c.dev<orbfe_cand>(o_cand), c.dev<int32_t>(o_nc), max_cand, 1, c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(cand, c.host(o_cand), b_cand);
  memcpy(n_cand, c.host(o_nc), sizeof(int32_t) * (size_t)nq);
  // the kernel keeps the candidate's octave in bits 16..19 of dist for the resolver; the public field is the distance
  for (int i = 0; i < nq; i++)
    for (int c = 0; c < std::min(n_cand[i], max_cand); c++) cand[(size_t)i * max_cand + c].dist &= 0xffff;
  return ORBFE_OK;
}

static int search_host(const orbfe_frame_view* f, const orbfe_query* q, int nq, int mode, float nnratio, int check_ori,
                       uint8_t* blocked, int32_t* assigned, int* n_matches, int th_high = ORBFE_TH_HIGH,
                       bool stereo_gate = true) {
  if (!frame_ok(f) || nq < 0 || (nq > 0 && !q) || !blocked || !assigned || !n_matches) return ORBFE_ERR_INVALID;
  *n_matches = 0;
  if (nq == 0 || f->n == 0) return ORBFE_OK;
  // one packed upload [n, nq | keys | desc | mvuRight | queries | blocked | assigned | n_matches], the three kernels, one packed
  // download of the tail [blocked | assigned | n_matches]
  const size_t n = (size_t)f->n;
  HostCall c("search by projection");
  const FrameRegions fr = frame_regions(c, f, stereo_gate);
  const size_t o_q = c.in(sizeof(orbfe_query) * (size_t)nq);
  const size_t o_blocked = c.out(n), o_assigned = c.out(sizeof(int32_t) * n), o_nm = c.out(16);
  int rc;
  if ((rc = c.open())) return rc;
  frame_fill(c, fr, f, nq);
  memcpy(c.host(o_q), q, sizeof(orbfe_query) * (size_t)nq);
  memcpy(c.host(o_blocked), blocked, n);
  memcpy(c.host(o_assigned), assigned, sizeof(int32_t) * n);
  *c.host<int32_t>(o_nm) = 0;
  if ((rc = c.upload(true))) return rc;
  rc = proj_enqueue(c.m, 1, c.dev<const orbfe_keypoint>(fr.keys), c.dev(fr.desc), frame_n(c, fr), fr.has_ur ? c.dev<const float>(fr.ur) : nullptr,
                    f->n, f->min_x, f->max_x, f->min_y, f->max_y, c.dev<const orbfe_query>(o_q), frame_nq(c, fr), nq, mode, nnratio, check_ori,
                    c.dev(o_blocked), c.dev<int32_t>(o_assigned), c.dev<int32_t>(o_nm), true, c.stream, th_high);
  if (rc || (rc = c.finish(c.out_bytes(), HOST_COPY_KERNEL))) return rc;
  memcpy(blocked, c.host(o_blocked), n);
  memcpy(assigned, c.host(o_assigned), sizeof(int32_t) * n);
  *n_matches = *c.host<const int32_t>(o_nm);
  return ORBFE_OK;
}

extern "C" int orbfe_search_by_projection_points(const orbfe_frame_view* f, const orbfe_query* q, int nq, float nnratio,
                                                 uint8_t* blocked, int32_t* assigned, int* n_matches) {
  return search_host(f, q, nq, 0, nnratio, 0, blocked, assigned, n_matches);
}
extern "C" int orbfe_search_by_projection_frame(const orbfe_frame_view* f, const orbfe_query* q, int nq,
                                                int check_orientation, uint8_t* blocked, int32_t* assigned,
                                                int* n_matches) {
  return search_host(f, q, nq, 1, 0.f, check_orientation, blocked, assigned, n_matches);
}

// ---- motion-model tracking: UnprojectStereo + the projection part of SearchByProjection(cur, last)
extern "C" int orbfe_unproject_stereo_device(int n_frames, const orbfe_keypoint* d_kps, const uint8_t* d_desc,
                                             const int32_t* d_n, const float* d_depth, int cap,
                                             const orbfe_unproject_cam* d_cam, int observed, orbfe_last_point* d_points,
                                             void* stream) {
  if (!d_kps || !d_desc || !d_n || !d_depth || !d_cam || !d_points || n_frames < 1 || cap < 1) return ORBFE_ERR_INVALID;
  if (((uintptr_t)d_desc & 15) || ((uintptr_t)d_kps & 3) || ((uintptr_t)d_points & 3) || ((uintptr_t)d_cam & 3)) {
    orbfe_set_error("descriptors must be 16-byte aligned, records 4-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  orbfe_launch_unproject_stereo(d_kps, d_desc, d_n, d_depth, cap, d_cam, observed, d_points, n_frames, (hipStream_t)stream);
  return hip_status("kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_track_queries_device(int n_frames, const orbfe_track_pose* d_pose, const orbfe_last_point* d_points,
                                          const int32_t* d_n_points, int p_cap, int frame_shift, orbfe_query* d_queries,
                                          int32_t* d_nq, void* stream) {
  if (!d_pose || !d_points || !d_n_points || !d_queries || !d_nq || n_frames < 1 || p_cap < 1) return ORBFE_ERR_INVALID;
  if (((uintptr_t)d_pose & 3) || ((uintptr_t)d_points & 3) || ((uintptr_t)d_queries & 3)) return ORBFE_ERR_INVALID;
  orbfe_launch_track_queries(d_pose, d_points, d_n_points, p_cap, frame_shift, d_queries, d_nq, n_frames, (hipStream_t)stream);
  return hip_status("kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_track_queries_stereo_device(int n_frames, const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
                                                 const float* d_depth, int cap, const orbfe_unproject_cam* d_cam, int observed,
                                                 const orbfe_keypoint* d_carry_kps, const uint8_t* d_carry_desc,
                                                 const int32_t* d_carry_n, const float* d_carry_depth,
                                                 const orbfe_unproject_cam* d_carry_cam, const orbfe_track_pose* d_pose,
                                                 int frame_shift, orbfe_query* d_queries, int32_t* d_nq, void* stream) {
  if (!d_kps || !d_desc || !d_n || !d_depth || !d_cam || !d_pose || !d_queries || !d_nq || n_frames < 1 || cap < 1 || frame_shift < 0)
    return ORBFE_ERR_INVALID;
  const bool carry = d_carry_kps || d_carry_desc || d_carry_n || d_carry_depth || d_carry_cam;
  if (carry && !(d_carry_kps && d_carry_desc && d_carry_n && d_carry_depth && d_carry_cam)) {
    orbfe_set_error("the carry frame needs all five arrays (keypoints, descriptors, count, depth, camera) or none");
    return ORBFE_ERR_INVALID;
  }
  if (carry && frame_shift > 1) {   // the carry holds one frame: frames 0 .. frame_shift-2 would read it in place of their own source
    orbfe_set_error("a carry frame holds one frame: frame_shift %d > 1 needs the batch's own tail (no carry)", frame_shift);
    return ORBFE_ERR_INVALID;
  }
  if (((uintptr_t)d_desc & 15) || ((uintptr_t)d_carry_desc & 15) || ((uintptr_t)d_kps & 3) || ((uintptr_t)d_carry_kps & 3) ||
      ((uintptr_t)d_cam & 3) || ((uintptr_t)d_carry_cam & 3) || ((uintptr_t)d_pose & 3) || ((uintptr_t)d_queries & 3)) {
    orbfe_set_error("descriptors must be 16-byte aligned, records 4-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  orbfe_launch_track_queries_stereo(d_kps, d_desc, d_n, d_depth, cap, d_cam, observed, d_carry_kps, d_carry_desc, d_carry_n, d_carry_depth,
                                    d_carry_cam, d_pose, frame_shift, d_queries, d_nq, n_frames, (hipStream_t)stream);
  return hip_status("kernel launch failed", hipGetLastError());
}

// ---- Tracking::SearchLocalPoints (L/src/Tracking.cc:1050-1078): isInFrustum -> queries (in HBM) -> SearchByProjection
static int local_points_enqueue(orbfe_matcher* m, int n_frames, const orbfe_keypoint* d_kps, const uint8_t* d_desc,
                                const int32_t* d_n, const float* d_ur, int cap, float min_x, float max_x, float min_y,
                                float max_y, const orbfe_frustum* d_fr, const orbfe_map_point* d_pts, const int32_t* d_np,
                                int p_cap, float th, float nnratio, orbfe_track* d_track, uint8_t* d_blocked,
                                int32_t* d_assigned, int32_t* d_ntm, int32_t* d_nm, hipStream_t s) {
  int rc;
  if ((rc = mb_alloc(m->lp_q, (size_t)n_frames * p_cap * sizeof(orbfe_query)))) return rc;
  HIPCHK(hipMemsetAsync(d_ntm, 0, sizeof(int32_t) * n_frames, s));
  orbfe_launch_frustum_queries(d_fr, d_pts, d_np, p_cap, th, 0.5f, d_track, (orbfe_query*)m->lp_q.p, d_ntm, n_frames, s);
  return proj_enqueue(m, n_frames, d_kps, d_desc, d_n, d_ur, cap, min_x, max_x, min_y, max_y, (const orbfe_query*)m->lp_q.p,
                      d_np, p_cap, 0, nnratio, 0, d_blocked, d_assigned, d_nm, true, s);
}

extern "C" int orbfe_search_local_points_batch_device(orbfe_matcher* m, int n_frames, const orbfe_keypoint* d_kps,
                                                      const uint8_t* d_desc, const int32_t* d_n, const float* d_u_right,
                                                      int cap, float min_x, float max_x, float min_y, float max_y,
                                                      const orbfe_frustum* d_frustum, const orbfe_map_point* d_points,
                                                      const int32_t* d_n_points, int p_cap, float th, float nnratio,
                                                      orbfe_track* d_track, uint8_t* d_blocked, int32_t* d_assigned,
                                                      int32_t* d_n_to_match, int32_t* d_n_matches, void* stream) {
  if (!m || !d_kps || !d_desc || !d_n || !d_frustum || !d_points || !d_n_points || !d_track || !d_blocked || !d_assigned ||
      !d_n_to_match || !d_n_matches || n_frames < 1 || cap < 1 || p_cap < 1 || !(max_x > min_x) || !(max_y > min_y))
    return ORBFE_ERR_INVALID;
  if (((uintptr_t)d_frustum & 3) || ((uintptr_t)d_points & 3) || ((uintptr_t)d_track & 3)) return ORBFE_ERR_INVALID;
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  return local_points_enqueue(m, n_frames, d_kps, d_desc, d_n, d_u_right, cap, min_x, max_x, min_y, max_y, d_frustum,
                              d_points, d_n_points, p_cap, th, nnratio, d_track, d_blocked, d_assigned, d_n_to_match,
                              d_n_matches, s);
}

extern "C" int orbfe_search_local_points(const orbfe_frame_view* f, const orbfe_frustum* fr, const orbfe_map_point* mp,
                                         int n_points, float th, float nnratio, orbfe_track* track, uint8_t* blocked,
                                         int32_t* assigned, int* n_to_match, int* n_matches) {
  if (!frame_ok(f) || !fr || n_points < 0 || (n_points > 0 && (!mp || !track)) || !blocked || !assigned || !n_to_match ||
      !n_matches || fr->n_levels < 1 || fr->n_levels > ORBFE_MAX_LEVELS)
    return ORBFE_ERR_INVALID;
  *n_to_match = 0;
  *n_matches = 0;
  if (n_points == 0) return ORBFE_OK;
  // one packed upload [frame | points | frustum | blocked | assigned], one packed download [blocked | assigned | track | counts]
  HostCall c("orbfe_search_local_points");
  const FrameRegions r = frame_regions(c, f, true);
  const size_t o_pts = c.in(sizeof(orbfe_map_point) * (size_t)n_points), o_fr = c.in(sizeof(orbfe_frustum));
  const size_t o_blocked = c.out((size_t)r.cap), o_assigned = c.out(sizeof(int32_t) * (size_t)r.cap),
               o_track = c.out(sizeof(orbfe_track) * (size_t)n_points), o_cnt = c.out(16);   // n_matches, n_to_match
  int rc;
  if ((rc = c.open())) return rc;
  frame_fill(c, r, f, n_points);
  memcpy(c.host(o_pts), mp, sizeof(orbfe_map_point) * (size_t)n_points);
  memcpy(c.host(o_fr), fr, sizeof(orbfe_frustum));
  if (f->n > 0) {
    memcpy(c.host(o_blocked), blocked, (size_t)f->n);
    memcpy(c.host(o_assigned), assigned, sizeof(int32_t) * (size_t)f->n);
  }
  if ((rc = c.upload(true))) return rc;
  rc = local_points_enqueue(c.m, 1, c.dev<const orbfe_keypoint>(r.keys), c.dev(r.desc), frame_n(c, r), r.has_ur ? c.dev<const float>(r.ur) : nullptr,
                            r.cap, f->min_x, f->max_x, f->min_y, f->max_y, c.dev<const orbfe_frustum>(o_fr), c.dev<const orbfe_map_point>(o_pts),
                            frame_nq(c, r), n_points, th, nnratio, c.dev<orbfe_track>(o_track), c.dev(o_blocked), c.dev<int32_t>(o_assigned),
                            c.dev<int32_t>(o_cnt) + 1, c.dev<int32_t>(o_cnt), c.stream);
  if (rc || (rc = c.finish(c.out_bytes()))) return rc;
  memcpy(track, c.host(o_track), sizeof(orbfe_track) * (size_t)n_points);
  if (f->n > 0) {
    memcpy(blocked, c.host(o_blocked), (size_t)f->n);
    memcpy(assigned, c.host(o_assigned), sizeof(int32_t) * (size_t)f->n);
  }
  *n_matches = c.host<const int32_t>(o_cnt)[0];
  *n_to_match = c.host<const int32_t>(o_cnt)[1];
  return ORBFE_OK;
}

// SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>&, th, ORBdist) (L/src/ORBmatcher.cc:1385-1504): the
// frame-to-frame walk without the stereo gate and with the caller's distance bound
extern "C" int orbfe_search_by_projection_keyframe(const orbfe_frame_view* f, const orbfe_query* q, int nq,
                                                   int check_orientation, int max_dist, uint8_t* blocked,
                                                   int32_t* assigned, int* n_matches) {
  if (max_dist < 0 || max_dist > 255) return ORBFE_ERR_INVALID;
  return search_host(f, q, nq, 1, 0.f, check_orientation, blocked, assigned, n_matches, max_dist, false);
}

// SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (L/src/ORBmatcher.cc:161-273), host pointers, synchronous
static int bow_impl(const uint8_t* descA, const float* angleA, const uint8_t* validA, int nA,
                    const orbfe_featvec_node* nodesA, int n_nodesA, const int32_t* idxA, const uint8_t* descB,
                    const float* angleB, const uint8_t* validB, int nB, const orbfe_featvec_node* nodesB, int n_nodesB,
                    const int32_t* idxB, float nnratio, int check_orientation, int kf_mode, int32_t* matchA_out,
                    int32_t* matchB, int* n_matches) {
  if (nA < 0 || nB < 0 || n_nodesA < 0 || n_nodesB < 0 || !n_matches || (nB > 0 && !matchB)) return ORBFE_ERR_INVALID;
  *n_matches = 0;
  for (int j = 0; j < nB; j++) matchB[j] = -1;
  if (kf_mode)
    for (int i = 0; i < nA; i++) matchA_out[i] = -1;
  if (nA == 0 || nB == 0 || n_nodesA == 0 || n_nodesB == 0) return ORBFE_OK;
  if (!descA || !angleA || !validA || !nodesA || !idxA || !descB || !angleB || !nodesB || !idxB) return ORBFE_ERR_INVALID;
  // the merge-join of the two FeatureVectors on NodeId, the bounds checks, the replay decision and the scratch size (search_plan.h)
  BowSearchPlan plan;
  if (int prc = orbfe_bow_search_plan(nA, nodesA, n_nodesA, idxA, nB, nodesB, n_nodesB, idxB, kf_mode, plan)) {
    if (plan.maxB > ORBFE_NODE_MAX_B) orbfe_set_error("a vocabulary node lists %d frame features (at most %d)", plan.maxB, ORBFE_NODE_MAX_B);
    return prc;
  }
  const std::vector<BowPair>& pairs = plan.pairs;
  const int totA = plan.totA, totB = plan.totB, maxB = plan.maxB, sequential = plan.sequential;
  if (pairs.empty()) return ORBFE_OK;
  // one packed upload [pairs | descA | descB | angleA | angleB | idxA | idxB | validA | validB | scratch | counters | matchB | matchA]
  // (the match tables go up filled with -1, the counters zero), one packed download of the tail from the counters on
  const size_t b_pairs = pairs.size() * sizeof(BowPair);
  HostCall c(kf_mode ? "orbfe_search_by_bow_kf" : "orbfe_search_by_bow");
  const size_t o_pairs = c.in(b_pairs), o_dA = c.in((size_t)nA * 32), o_dB = c.in((size_t)nB * 32), o_aA = c.in((size_t)nA * 4),
               o_aB = c.in((size_t)nB * 4), o_iA = c.in((size_t)totA * 4), o_iB = c.in((size_t)totB * 4), o_vA = c.in((size_t)nA),
               o_vB = c.in(kf_mode ? (size_t)nB : 0);
  const size_t o_pi = c.scratch((size_t)plan.push_cap * 4), o_pb = c.scratch((size_t)plan.push_cap);   // one entry per visit of an A feature
  const size_t o_cnt = c.out(256), o_mB = c.out((size_t)nB * 4), o_mA = c.out(kf_mode ? (size_t)nA * 4 : 0);
  int rc;
  if ((rc = c.open())) return rc;
  memcpy(c.host(o_pairs), pairs.data(), b_pairs);
  memcpy(c.host(o_dA), descA, (size_t)nA * 32);
  memcpy(c.host(o_dB), descB, (size_t)nB * 32);
  memcpy(c.host(o_aA), angleA, (size_t)nA * 4);
  memcpy(c.host(o_aB), angleB, (size_t)nB * 4);
  memcpy(c.host(o_iA), idxA, (size_t)totA * 4);
  memcpy(c.host(o_iB), idxB, (size_t)totB * 4);
  memcpy(c.host(o_vA), validA, (size_t)nA);
  if (kf_mode) memcpy(c.host(o_vB), validB, (size_t)nB);
  memset(c.host(o_cnt), 0, 256);
  memset(c.host(o_mB), 0xff, (size_t)nB * 4);
  if (kf_mode) memset(c.host(o_mA), 0xff, (size_t)nA * 4);
  if ((rc = c.upload(true))) return rc;
  BowParams p;
  p.pairs = c.dev<const BowPair>(o_pairs);
  p.descA = c.dev(o_dA); p.angleA = c.dev<const float>(o_aA); p.validA = c.dev(o_vA); p.idxA = c.dev<const int32_t>(o_iA);
  p.descB = c.dev(o_dB); p.angleB = c.dev<const float>(o_aB); p.idxB = c.dev<const int32_t>(o_iB);
  p.nnratio = nnratio; p.check_ori = check_orientation;
  p.sequential = sequential; p.n_pairs = (int)pairs.size();
  p.kf_mode = kf_mode; p.validB = kf_mode ? c.dev(o_vB) : nullptr; p.matchA = kf_mode ? c.dev<int32_t>(o_mA) : nullptr;
  p.matchB = c.dev<int32_t>(o_mB); p.counters = c.dev<int32_t>(o_cnt);
  p.push_idx = c.dev<int32_t>(o_pi); p.push_bin = c.dev(o_pb);
  orbfe_launch_bow(p, (int)pairs.size(), maxB, c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(matchB, c.host(o_mB), (size_t)nB * 4);
  if (kf_mode) memcpy(matchA_out, c.host(o_mA), (size_t)nA * 4);
  *n_matches = c.host<const int32_t>(o_cnt)[1];
  return ORBFE_OK;
}

extern "C" int orbfe_search_by_bow(const uint8_t* descA, const float* angleA, const uint8_t* validA, int nA,
                                   const orbfe_featvec_node* nodesA, int n_nodesA, const int32_t* idxA,
                                   const uint8_t* descB, const float* angleB, int nB, const orbfe_featvec_node* nodesB,
                                   int n_nodesB, const int32_t* idxB, float nnratio, int check_orientation,
                                   int32_t* matchB, int* n_matches) {
  return bow_impl(descA, angleA, validA, nA, nodesA, n_nodesA, idxA, descB, angleB, nullptr, nB, nodesB, n_nodesB, idxB,
                  nnratio, check_orientation, 0, nullptr, matchB, n_matches);
}

// SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (L/src/ORBmatcher.cc:494-612)
extern "C" int orbfe_search_by_bow_kf(const uint8_t* descA, const float* angleA, const uint8_t* validA, int nA,
                                      const orbfe_featvec_node* nodesA, int n_nodesA, const int32_t* idxA,
                                      const uint8_t* descB, const float* angleB, const uint8_t* validB, int nB,
                                      const orbfe_featvec_node* nodesB, int n_nodesB, const int32_t* idxB, float nnratio,
                                      int check_orientation, int32_t* matchA, int* n_matches) {
  if (!matchA && nA > 0) return ORBFE_ERR_INVALID;
  if (nB > 0 && !validB) return ORBFE_ERR_INVALID;
  std::vector<int32_t> matchB((size_t)std::max(nB, 1));
  return bow_impl(descA, angleA, validA, nA, nodesA, n_nodesA, idxA, descB, angleB, validB, nB, nodesB, n_nodesB, idxB,
                  nnratio, check_orientation, 1, matchA, matchB.data(), n_matches);
}

// Independent arg-min searches (Fuse, Fuse(Sim3), SearchBySim3), host pointers, synchronous
extern "C" int orbfe_proj_best(const orbfe_frame_view* f, const orbfe_query* q, int nq, int gate, const float* inv_level_sigma2,
                               int n_levels, int32_t* best_idx, int32_t* best_dist) {
  if (!frame_ok(f) || nq < 0 || (nq > 0 && (!q || !best_idx || !best_dist)) || (gate != ORBFE_GATE_NONE && gate != ORBFE_GATE_FUSE_CHI2) ||
      (gate == ORBFE_GATE_FUSE_CHI2 && (!inv_level_sigma2 || n_levels < 1 || n_levels > ORBFE_MAX_LEVELS)))
    return ORBFE_ERR_INVALID;
  for (int i = 0; i < nq; i++) { best_idx[i] = -1; best_dist[i] = 256; }
  if (nq == 0 || f->n == 0) return ORBFE_OK;
  HostCall c("orbfe_proj_best");
  const FrameRegions fr = frame_regions(c, f, true);
  const size_t o_q = c.in(sizeof(orbfe_query) * (size_t)nq), o_inv = c.in(sizeof(float) * ORBFE_MAX_LEVELS);
  const size_t o_bi = c.out(sizeof(int32_t) * (size_t)nq), o_bd = c.out(sizeof(int32_t) * (size_t)nq);
  int rc;
  if ((rc = c.open()) || (rc = ensure_proj_scratch(c.m, 1, fr.cap, nq))) return rc;
  frame_fill(c, fr, f, nq);
  memcpy(c.host(o_q), q, sizeof(orbfe_query) * (size_t)nq);
  memset(c.host(o_inv), 0, sizeof(float) * ORBFE_MAX_LEVELS);
  if (gate == ORBFE_GATE_FUSE_CHI2) memcpy(c.host(o_inv), inv_level_sigma2, sizeof(float) * n_levels);
  if ((rc = c.upload())) return rc;
  FrameBatch fb;
  fill_frame_batch(c.m, fb, c.dev<const orbfe_keypoint>(fr.keys), c.dev(fr.desc), frame_n(c, fr), fr.has_ur ? c.dev<const float>(fr.ur) : nullptr,
                   fr.cap, f->min_x, f->max_x, f->min_y, f->max_y);
  QueryBatch qb{c.dev<const orbfe_query>(o_q), frame_nq(c, fr), nq};
  orbfe_launch_grid_build(fb, 1, c.stream);
  orbfe_launch_proj_best(fb, qb, gate, c.dev<const float>(o_inv), c.dev<int32_t>(o_bi), c.dev<int32_t>(o_bd), 1, c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(best_idx, c.host(o_bi), sizeof(int32_t) * (size_t)nq);
  memcpy(best_dist, c.host(o_bd), sizeof(int32_t) * (size_t)nq);
  return ORBFE_OK;
}

// Fuse / Fuse(Sim3) / SearchBySim3 / SearchByProjection(KF,Scw) / SearchByProjection(Frame,KF,...) from the projection on
// (L/src/ORBmatcher.cc:766-1245, 275-386, 1385-1504): prologue kernel -> queries in HBM -> window search, host pointers
extern "C" int orbfe_kf_search(const orbfe_frame_view* f, const float* inv_level_sigma2, const orbfe_kf_camera* cam,
                               const orbfe_kf_point* points, int n_points, int mode, int check_orientation, int max_dist,
                               uint8_t* blocked, orbfe_kf_result* results, int* n_matches) {
  const bool seq = mode == ORBFE_KF_LOOP || mode == ORBFE_KF_RELOC;   // earlier points block later ones
  if (!frame_ok(f) || !cam || n_points < 0 || (n_points > 0 && (!points || !results)) || !n_matches || mode < ORBFE_KF_FUSE ||
      mode > ORBFE_KF_RELOC || cam->n_levels < 1 || cam->n_levels > ORBFE_MAX_LEVELS || (mode == ORBFE_KF_FUSE && !inv_level_sigma2) ||
      (seq && f->n > 0 && !blocked))
    return ORBFE_ERR_INVALID;
  *n_matches = 0;
  for (int i = 0; i < n_points; i++) {
    results[i].best_idx = -1; results[i].best_dist = 256; results[i].level = -1;
    results[i].u = results[i].v = results[i].u_r = 0.f;
  }
  if (n_points == 0) return ORBFE_OK;
  // one packed upload [frame | points | camera | 1 / sigma2], the prologue and the search, one packed download: the prologue's results
  // (no later kernel writes them), then [best_idx | best_dist] of the independent searches or, for the sequential modes, the
  // greedy resolver's [blocked | assigned | n_matches], which also go up
  const int gate = mode == ORBFE_KF_FUSE ? ORBFE_GATE_FUSE_CHI2 : ORBFE_GATE_NONE;
  const size_t b_res = sizeof(orbfe_kf_result) * (size_t)n_points, b_int = sizeof(int32_t) * (size_t)n_points;
  HostCall c("orbfe_kf_search");
  const FrameRegions fr = frame_regions(c, f, !seq && gate == ORBFE_GATE_FUSE_CHI2);
  const int cap = fr.cap;
  const size_t o_pts = c.in(sizeof(orbfe_kf_point) * (size_t)n_points), o_cam = c.in(sizeof(orbfe_kf_camera)),
               o_inv = c.in(sizeof(float) * ORBFE_MAX_LEVELS);
  const size_t o_res = c.out(b_res), o_bi = c.out(seq ? 0 : b_int), o_bd = c.out(seq ? 0 : b_int), o_blocked = c.out(seq ? (size_t)cap : 0),
               o_assigned = c.out(seq ? sizeof(int32_t) * (size_t)cap : 0), o_nm = c.out(seq ? 16 : 0);
  int rc;
  if ((rc = c.open()) || (rc = mb_alloc(c.m->lp_q, sizeof(orbfe_query) * (size_t)n_points))) return rc;
  frame_fill(c, fr, f, n_points);
  memcpy(c.host(o_pts), points, sizeof(orbfe_kf_point) * (size_t)n_points);
  memcpy(c.host(o_cam), cam, sizeof(orbfe_kf_camera));
  memset(c.host(o_inv), 0, sizeof(float) * ORBFE_MAX_LEVELS);
  if (gate == ORBFE_GATE_FUSE_CHI2) memcpy(c.host(o_inv), inv_level_sigma2, sizeof(float) * cam->n_levels);
  if (seq && f->n > 0) {
    memcpy(c.host(o_blocked), blocked, (size_t)cap);
    std::fill_n(c.host<int32_t>(o_assigned), cap, -2);
  }
  if ((rc = c.upload(seq))) return rc;
  const orbfe_query* d_q = (const orbfe_query*)c.m->lp_q.p;
  orbfe_launch_kf_queries(c.dev<const orbfe_kf_camera>(o_cam), c.dev<const orbfe_kf_point>(o_pts), n_points, mode, (orbfe_query*)c.m->lp_q.p,
                          c.dev<orbfe_kf_result>(o_res), c.stream);
  if (f->n == 0) {
    if ((rc = c.finish(b_res))) return rc;
    memcpy(results, c.host(o_res), b_res);
    return ORBFE_OK;
  }
  if (!seq) {
    if ((rc = ensure_proj_scratch(c.m, 1, cap, n_points))) return rc;
    FrameBatch fb;
    fill_frame_batch(c.m, fb, c.dev<const orbfe_keypoint>(fr.keys), c.dev(fr.desc), frame_n(c, fr), fr.has_ur ? c.dev<const float>(fr.ur) : nullptr,
                     cap, f->min_x, f->max_x, f->min_y, f->max_y);
    QueryBatch qb{d_q, frame_nq(c, fr), n_points};
    orbfe_launch_grid_build(fb, 1, c.stream);
    orbfe_launch_proj_best(fb, qb, gate, c.dev<const float>(o_inv), c.dev<int32_t>(o_bi), c.dev<int32_t>(o_bd), 1, c.stream);
    if ((rc = c.finish(c.out_bytes()))) return rc;
    memcpy(results, c.host(o_res), b_res);
    const int32_t *bi = c.host<const int32_t>(o_bi), *bd = c.host<const int32_t>(o_bd);
    int cnt = 0;
    for (int i = 0; i < n_points; i++) {
      results[i].best_idx = bi[i];
      results[i].best_dist = bd[i];
      cnt += bi[i] >= 0;
    }
    *n_matches = cnt;
    return ORBFE_OK;
  }
  // sequential modes: the greedy resolver of SearchByProjection(cur, last) with the caller's distance bound, no stereo gate
  rc = proj_enqueue(c.m, 1, c.dev<const orbfe_keypoint>(fr.keys), c.dev(fr.desc), frame_n(c, fr), nullptr, cap, f->min_x, f->max_x, f->min_y,
                    f->max_y, d_q, frame_nq(c, fr), n_points, 1, 0.f, mode == ORBFE_KF_RELOC ? check_orientation : 0, c.dev(o_blocked),
                    c.dev<int32_t>(o_assigned), c.dev<int32_t>(o_nm), true, c.stream, max_dist);
  if (rc || (rc = c.finish(c.out_bytes()))) return rc;
  memcpy(results, c.host(o_res), b_res);
  memcpy(blocked, c.host(o_blocked), (size_t)cap);
  const int32_t* assigned = c.host<const int32_t>(o_assigned);
  for (int j = 0; j < cap; j++)
    if (assigned[j] >= 0 && assigned[j] < n_points) results[assigned[j]].best_idx = j;
  *n_matches = *c.host<const int32_t>(o_nm);
  return ORBFE_OK;
}

// The enqueue half: the search and its rotation-histogram pass on stream s, every pointer a device pointer
int orbfe_tri_search_enqueue(const TriSearchBuffers& b, const orbfe_epipolar* ep, int check_orientation, int sequential, hipStream_t s) {
  TriParams t;
  memset(&t, 0, sizeof(t));
  t.b.pairs = b.pairs;
  t.b.descA = b.descA; t.b.validA = b.validA; t.b.idxA = b.idxA;
  t.b.descB = b.descB; t.b.validB = b.validB; t.b.idxB = b.idxB;
  t.b.check_ori = check_orientation; t.b.sequential = sequential; t.b.n_pairs = b.n_pairs;
  t.b.kf_mode = 1;   // bow_finish_kernel: rotation rejects clear matchA[push_idx]
  t.b.matchA = b.matchA; t.b.matchB = nullptr;
  t.b.counters = b.counters; t.b.push_idx = b.push_idx; t.b.push_bin = b.push_bin;
  t.keysA = b.keysA; t.keysB = b.keysB;
  t.stereoA = b.stereoA; t.stereoB = b.stereoB;
  t.ep = *ep;
  orbfe_launch_triangulation(t, b.n_pairs, s);
  return hip_status("kernel launch failed", hipGetLastError());
}

// SearchForTriangulation (L/src/ORBmatcher.cc:614-764), host pointers, synchronous
extern "C" int orbfe_search_for_triangulation(const orbfe_keypoint* keysA, const uint8_t* descA, const float* u_rightA,
                                              const uint8_t* has_mpA, int nA, const orbfe_featvec_node* nodesA, int n_nodesA,
                                              const int32_t* idxA, const orbfe_keypoint* keysB, const uint8_t* descB,
                                              const float* u_rightB, const uint8_t* has_mpB, int nB,
                                              const orbfe_featvec_node* nodesB, int n_nodesB, const int32_t* idxB,
                                              const orbfe_epipolar* ep, int only_stereo, int check_orientation,
                                              int32_t* matchA, int* n_matches) {
  if (nA < 0 || nB < 0 || n_nodesA < 0 || n_nodesB < 0 || !n_matches || (nA > 0 && !matchA) || !ep) return ORBFE_ERR_INVALID;
  *n_matches = 0;
  for (int i = 0; i < nA; i++) matchA[i] = -1;
  if (nA == 0 || nB == 0 || n_nodesA == 0 || n_nodesB == 0) return ORBFE_OK;
  if (!keysA || !descA || !has_mpA || !nodesA || !idxA || !keysB || !descB || !has_mpB || !nodesB || !idxB) return ORBFE_ERR_INVALID;
  TriSearchPlan plan;
  int rc;
  if ((rc = orbfe_tri_search_plan(nA, nodesA, n_nodesA, idxA, nB, nodesB, n_nodesB, idxB, plan))) return rc;
  const std::vector<BowPair>& pairs = plan.pairs;
  const int totA = plan.totA, totB = plan.totB;
  if (pairs.empty()) return ORBFE_OK;
  // one packed upload [pairs | descA | descB | keysA | keysB | idxA | idxB | validA | validB | stereoA | stereoB | scratch | matchA | counters]
  // (matchA goes up filled with -1, the counters zero), one packed download of [matchA | counters]
  const size_t b_pairs = pairs.size() * sizeof(BowPair), push_n = (size_t)plan.push_cap;
  HostCall c("orbfe_search_for_triangulation");
  const size_t o_pairs = c.in(b_pairs), o_dA = c.in((size_t)nA * 32), o_dB = c.in((size_t)nB * 32), o_kA = c.in((size_t)nA * sizeof(orbfe_keypoint)),
               o_kB = c.in((size_t)nB * sizeof(orbfe_keypoint)), o_iA = c.in((size_t)totA * 4), o_iB = c.in((size_t)totB * 4),
               o_vA = c.in((size_t)nA), o_vB = c.in((size_t)nB), o_sA = c.in((size_t)nA), o_sB = c.in((size_t)nB);
  const size_t o_pi = c.scratch(push_n * 4), o_pb = c.scratch(push_n);
  const size_t o_mA = c.out((size_t)nA * 4), o_cnt = c.out(256);
  if ((rc = c.open())) return rc;
  memcpy(c.host(o_pairs), pairs.data(), b_pairs);
  memcpy(c.host(o_dA), descA, (size_t)nA * 32);
  memcpy(c.host(o_dB), descB, (size_t)nB * 32);
  memcpy(c.host(o_kA), keysA, (size_t)nA * sizeof(orbfe_keypoint));
  memcpy(c.host(o_kB), keysB, (size_t)nB * sizeof(orbfe_keypoint));
  memcpy(c.host(o_iA), idxA, (size_t)totA * 4);
  memcpy(c.host(o_iB), idxB, (size_t)totB * 4);
  // candidate masks and stereo flags (:655-664, 677-686)
  uint8_t *vA = c.host(o_vA), *vB = c.host(o_vB), *sA = c.host(o_sA), *sB = c.host(o_sB);
  for (int i = 0; i < nA; i++) { sA[i] = u_rightA && u_rightA[i] >= 0; vA[i] = !has_mpA[i] && (!only_stereo || sA[i]); }
  for (int i = 0; i < nB; i++) { sB[i] = u_rightB && u_rightB[i] >= 0; vB[i] = !has_mpB[i] && (!only_stereo || sB[i]); }
  memset(c.host(o_mA), 0xff, (size_t)nA * 4);
  memset(c.host(o_cnt), 0, 256);
  if ((rc = c.upload(true))) return rc;
  TriSearchBuffers b;
  b.pairs = c.dev<const BowPair>(o_pairs); b.n_pairs = (int)pairs.size();
  b.descA = c.dev(o_dA); b.descB = c.dev(o_dB);
  b.keysA = c.dev<const orbfe_keypoint>(o_kA); b.keysB = c.dev<const orbfe_keypoint>(o_kB);
  b.idxA = c.dev<const int32_t>(o_iA); b.idxB = c.dev<const int32_t>(o_iB);
  b.validA = c.dev(o_vA); b.validB = c.dev(o_vB); b.stereoA = c.dev(o_sA); b.stereoB = c.dev(o_sB);
  b.matchA = c.dev<int32_t>(o_mA); b.counters = c.dev<int32_t>(o_cnt);
  b.push_idx = c.dev<int32_t>(o_pi); b.push_bin = c.dev(o_pb);
  if ((rc = orbfe_tri_search_enqueue(b, ep, check_orientation, plan.sequential, c.stream)) || (rc = c.finish(c.out_bytes()))) return rc;
  memcpy(matchA, c.host(o_mA), (size_t)nA * 4);
  *n_matches = c.host<const int32_t>(o_cnt)[1];
  return ORBFE_OK;
}

// SearchForInitialization (L/src/ORBmatcher.cc:388-492), host pointers, synchronous
extern "C" int orbfe_search_for_initialization(const orbfe_frame_view* f1, const orbfe_frame_view* f2, float* prev_matched_xy,
                                               int window_size, float nnratio, int check_orientation, int32_t* matches12,
                                               int* n_matches) {
  if (!frame_ok(f2) || !f1 || f1->n < 0 || (f1->n > 0 && (!f1->keys_un || !f1->desc || !prev_matched_xy || !matches12)) ||
      !n_matches || window_size < 0)
    return ORBFE_ERR_INVALID;
  *n_matches = 0;
  const int n1 = f1->n;
  for (int i = 0; i < n1; i++) matches12[i] = -1;
  if (n1 == 0 || f2->n == 0) return ORBFE_OK;
  // one packed upload [F2 | queries | vbPrevMatched], one packed download [vbPrevMatched | matches12 | n_matches]
  HostCall c("orbfe_search_for_initialization");
  const FrameRegions fr = frame_regions(c, f2, false);   // no stereo gate in this search
  const int cap = f2->n;
  const size_t o_q = c.in(sizeof(orbfe_query) * (size_t)n1);
  const size_t o_prev = c.out(sizeof(float) * 2 * (size_t)n1), o_m12 = c.out(sizeof(int32_t) * (size_t)n1), o_nm = c.out(16);
  int rc;
  if ((rc = c.open()) || (rc = ensure_proj_scratch(c.m, 1, cap, n1))) return rc;
  if ((size_t)cap * 8 > 60 * 1024) {
    orbfe_set_error("SearchForInitialization: frame with %d keypoints exceeds the LDS-resident tables", cap);
    return ORBFE_ERR_INVALID;
  }
  frame_fill(c, fr, f2, n1);
  // one query per F1 keypoint: window around vbPrevMatched[i1], level filter (level1, level1) (:403-410)
  orbfe_query* q = c.host<orbfe_query>(o_q);
  for (int i = 0; i < n1; i++) {
    orbfe_query& e = q[i];
    memset(&e, 0, sizeof(e));
    const int level1 = f1->keys_un[i].octave;
    if (level1 > 0) continue;
    e.u = prev_matched_xy[2 * i];
    e.v = prev_matched_xy[2 * i + 1];
    e.radius = (float)window_size;
    e.min_level = level1;
    e.max_level = level1;
    e.valid = 1;
    e.angle = f1->keys_un[i].angle;
    memcpy(e.desc, f1->desc + (size_t)i * 32, 32);
  }
  memcpy(c.host(o_prev), prev_matched_xy, sizeof(float) * 2 * (size_t)n1);
  if ((rc = c.upload(true))) return rc;
  FrameBatch fb;
  fill_frame_batch(c.m, fb, c.dev<const orbfe_keypoint>(fr.keys), c.dev(fr.desc), frame_n(c, fr), nullptr, cap, f2->min_x, f2->max_x, f2->min_y,
                   f2->max_y);
  QueryBatch qb{c.dev<const orbfe_query>(o_q), frame_nq(c, fr), n1};
  orbfe_launch_grid_build(fb, 1, c.stream);
  orbfe_launch_proj_candidates(fb, qb, (orbfe_cand*)c.m->cand.p, (int32_t*)c.m->n_cand.p, ORBFE_MAX_CAND, 1, c.stream);
  orbfe_launch_init_resolve(fb, qb, (const orbfe_cand*)c.m->cand.p, (const int32_t*)c.m->n_cand.p, ORBFE_MAX_CAND, nnratio, check_orientation,
                            c.dev<int32_t>(o_m12), c.dev<float>(o_prev), c.dev<int32_t>(o_nm), (int32_t*)c.m->push_idx.p,
                            (uint8_t*)c.m->push_bin.p, c.stream);
  if ((rc = c.finish(c.out_bytes()))) return rc;
  memcpy(matches12, c.host(o_m12), sizeof(int32_t) * (size_t)n1);
  memcpy(prev_matched_xy, c.host(o_prev), sizeof(float) * 2 * (size_t)n1);
  *n_matches = *c.host<const int32_t>(o_nm);
  return ORBFE_OK;
}

// ------------------------------------------------------------------------------------------------ stereo
// the three stereo kernels for n_pairs pairs; the caller holds m->mu and has selected the device
static int stereo_enqueue(orbfe_matcher* m, orbfe_extractor* left, orbfe_extractor* right, int n_pairs,
                          const orbfe_keypoint* d_kps_l, const uint8_t* d_desc_l, const int32_t* d_n_l,
                          const orbfe_keypoint* d_kps_r, const uint8_t* d_desc_r, const int32_t* d_n_r, int cap, float mbf,
                          float mb, float* d_u_right, float* d_depth, int32_t* d_n_matched, hipStream_t stream) {
  StereoParams p;
  memset(&p, 0, sizeof(p));
  int nl = 0, nr = 0, il = 0, ir = 0, devl = 0, devr = 0;
  int rc;
  if ((rc = orbfe_internal_pyr_view(left, &p.pyrL, &il)) || (rc = orbfe_internal_pyr_view(right, &p.pyrR, &ir))) {
    orbfe_set_error("stereo match needs both extractors to have processed a device batch");
    return ORBFE_ERR_INVALID;
  }
  float sr[ORBFE_MAX_LEVELS], isr[ORBFE_MAX_LEVELS];
  orbfe_internal_tables(left, p.scale, p.inv_scale, &nl, &devl);
  orbfe_internal_tables(right, sr, isr, &nr, &devr);
  if (nl != nr || devl != m->device || devr != m->device || il < n_pairs || ir < n_pairs) {
    orbfe_set_error("stereo match: extractors must share levels/device and hold >= n_pairs images");
    return ORBFE_ERR_INVALID;
  }
  for (int l = 0; l < nl; l++)
    if (p.pyrL.w[l] != p.pyrR.w[l] || p.pyrL.h[l] != p.pyrR.h[l]) {
      orbfe_set_error("stereo match: left/right pyramids differ in size");
      return ORBFE_ERR_INVALID;
    }
  if ((rc = mb_alloc(m->sad, sizeof(int32_t) * (size_t)n_pairs * cap))) return rc;
  p.n_buckets = (p.pyrL.h[0] + 7) / 8;
  p.n_levels = nl;
  p.n_keys = p.n_buckets * nl;
  if (p.n_buckets > STEREO_MAX_BUCKETS || p.n_keys > STEREO_MAX_KEYS) {
    orbfe_set_error("stereo match: %d row buckets x %d levels exceed %d keys", p.n_buckets, nl, STEREO_MAX_KEYS);
    return ORBFE_ERR_INVALID;
  }
  if ((rc = mb_alloc(m->bucket_start, sizeof(int32_t) * (size_t)n_pairs * (p.n_keys + 1)))) return rc;
  if ((rc = mb_alloc(m->bucket_idx, 16 * (size_t)n_pairs * cap * STEREO_BUCKET_SPAN))) return rc;  // int4 records
  p.bucket_start = (int32_t*)m->bucket_start.p;
  p.bucket_idx = (int32_t*)m->bucket_idx.p;
  for (int l = 0; l < nl; l++)
    if (2.0f * p.scale[l] + 2.0f > 8.0f * (STEREO_BUCKET_SPAN - 1) / 2.0f) {
      orbfe_set_error("stereo match: pyramid scale %.2f too large for the row buckets", p.scale[l]);
      return ORBFE_ERR_INVALID;
    }
  p.kpsL = d_kps_l; p.descL = d_desc_l; p.nL = d_n_l;
  p.kpsR = d_kps_r; p.descR = d_desc_r; p.nR = d_n_r;
  p.cap = cap;
  p.mbf = mbf;
  p.maxD = mbf / mb;  // minZ = mb, maxD = mbf / minZ (L/src/Frame.cc:505-507)
  p.u_right = d_u_right;
  p.depth = d_depth;
  p.sad = (int32_t*)m->sad.p;
  p.n_matched = d_n_matched;
  orbfe_launch_stereo(p, n_pairs, stream);
  return hip_status("kernel launch failed", hipGetLastError());
}

extern "C" int orbfe_stereo_match_device(orbfe_matcher* m, orbfe_extractor* left, orbfe_extractor* right, int n_pairs,
                                         const orbfe_keypoint* d_kps_l, const uint8_t* d_desc_l, const int32_t* d_n_l,
                                         const orbfe_keypoint* d_kps_r, const uint8_t* d_desc_r, const int32_t* d_n_r,
                                         int cap, float mbf, float mb, float* d_u_right, float* d_depth,
                                         int32_t* d_n_matched, void* stream) {
  if (!m || !left || !right || n_pairs < 1 || !d_kps_l || !d_desc_l || !d_n_l || !d_kps_r || !d_desc_r || !d_n_r ||
      cap < 1 || cap >= 65536 || !d_u_right || !d_depth || !d_n_matched || !(mb > 0))
    return ORBFE_ERR_INVALID;
  if (((uintptr_t)d_desc_l & 15) || ((uintptr_t)d_desc_r & 15)) {
    orbfe_set_error("descriptor matrices must be 16-byte aligned");
    return ORBFE_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipSetDevice(m->device));
  return stereo_enqueue(m, left, right, n_pairs, d_kps_l, d_desc_l, d_n_l, d_kps_r, d_desc_r, d_n_r, cap, mbf, mb, d_u_right,
                        d_depth, d_n_matched, stream ? (hipStream_t)stream : m->stream);
}

// Frame::ComputeStereoMatches for the ONE pair the two extractors processed last (L/src/Frame.cc:91-99: the two ExtractORB
// threads, then ComputeStereoMatches): host keypoints / descriptors in, mvuRight / mvDepth out, the SAD refinement reads the
// pyramids that are still in HBM.  One packed upload, three kernels, one packed download on the calling thread's matcher.
extern "C" int orbfe_stereo_match(orbfe_extractor* left, orbfe_extractor* right, const orbfe_keypoint* kps_l,
                                  const uint8_t* desc_l, int n_l, const orbfe_keypoint* kps_r, const uint8_t* desc_r, int n_r,
                                  float mbf, float mb, float* u_right, float* depth, int* n_matched) {
  if (!left || !right || n_l < 0 || n_r < 0 || (n_l > 0 && (!kps_l || !desc_l || !u_right || !depth)) ||
      (n_r > 0 && (!kps_r || !desc_r)) || n_l >= 65536 || n_r >= 65536 || !(mb > 0))
    return ORBFE_ERR_INVALID;
  if (n_matched) *n_matched = 0;
  for (int i = 0; i < n_l; i++) u_right[i] = depth[i] = -1.0f;   // L/src/Frame.cc:478-479
  if (n_l == 0 || n_r == 0) return ORBFE_OK;
  const size_t cap = (size_t)std::max(n_l, n_r);
  // one packed upload [n_l, n_r | keys_l | keys_r | desc_l | desc_r], three kernels, one packed download [u_right | depth | n]
  HostCall c("orbfe_stereo_match");
  const size_t o_hdr = c.in(16), o_kl = c.in(sizeof(orbfe_keypoint) * cap), o_kr = c.in(sizeof(orbfe_keypoint) * cap), o_dl = c.in(32 * cap),
               o_dr = c.in(32 * cap);
  const size_t o_ur = c.out(sizeof(float) * cap), o_dp = c.out(sizeof(float) * cap), o_nm = c.out(16);
  int rc;
  if ((rc = c.open())) return rc;
  c.host<int32_t>(o_hdr)[0] = n_l;
  c.host<int32_t>(o_hdr)[1] = n_r;
  memcpy(c.host(o_kl), kps_l, sizeof(orbfe_keypoint) * (size_t)n_l);
  memcpy(c.host(o_kr), kps_r, sizeof(orbfe_keypoint) * (size_t)n_r);
  memcpy(c.host(o_dl), desc_l, (size_t)32 * n_l);
  memcpy(c.host(o_dr), desc_r, (size_t)32 * n_r);
  if ((rc = c.upload())) return rc;
  rc = stereo_enqueue(c.m, left, right, 1, c.dev<const orbfe_keypoint>(o_kl), c.dev(o_dl), c.dev<const int32_t>(o_hdr),
                      c.dev<const orbfe_keypoint>(o_kr), c.dev(o_dr), c.dev<const int32_t>(o_hdr) + 1, (int)cap, mbf, mb, c.dev<float>(o_ur),
                      c.dev<float>(o_dp), c.dev<int32_t>(o_nm), c.stream);
  if (rc || (rc = c.finish(c.out_bytes(), HOST_COPY_KERNEL))) return rc;
  memcpy(u_right, c.host(o_ur), sizeof(float) * (size_t)n_l);
  memcpy(depth, c.host(o_dp), sizeof(float) * (size_t)n_l);
  if (n_matched) *n_matched = *c.host<const int32_t>(o_nm);
  return ORBFE_OK;
}
