// keyframe_kernels.hip -- the keyframe decision and the close stereo points of a tracked frame (the statistics tail of
// Tracking::TrackLocalMap, NeedNewKeyFrame, the point creation of CreateNewKeyFrame / UpdateLastFrame / StereoInitialization) for
// gfx950.  One frame is one workgroup of KF_THREADS threads; the rules are those of keyframe_internal.h, spread over lanes.
//
// LDS (dynamic, sized by the call's cap): the candidate keys (8 bytes each, a power of two of them), one mark bit per keypoint row,
// the scale factors, per-wave counts and sums.
//   0. everything behind an index is range-checked, so that a refused frame has written nothing but its header and n_new
//   1. one pass over the rows for the four counts; every thread then holds the sums and evaluates the decision alike
//   2. the candidates are compacted in index order (a ballot per wave, per-wave counts), padded to the next power of two of the
//      frame's own M and sorted by a bitonic network in LDS: a frame pays for its M, not for cap
//   3. the octave of every created entry of the prefix is checked; nothing of the frame has been written so far
//   4. the prefix in rounds of KF_THREADS: a ballot per wave and the per-wave counts give each created entry its place in the
//      order of the prefix; its thread writes the record, the index and the slot
//   5. depth_selected from the marks, the header
// The keys are distinct, so the network's result is the one sorted order; ballots and integer sums carry no order into the result.
#include <atomic>

#include "keyframe_internal.h"

static_assert(sizeof(orbfe_map_point) == 4 * KF_RECORD_DWORDS && sizeof(orbfe_kf_header) == 64 && sizeof(orbfe_kf_decision_in) == 56 &&
              sizeof(orbfe_kf_scales) == 72, "record layout");

namespace {

constexpr int KF_WAVES = KF_THREADS / 64;

__host__ __device__ inline int kf_pow2(int m) {
  int p = 1;
  while (p < m) p <<= 1;
  return p;
}
__host__ __device__ inline int kf_mark_words(int cap) { return ((cap + 31) / 32 + 3) & ~3; }
__host__ __device__ inline size_t kf_lds_bytes(int cap) {
  return (size_t)kf_pow2(cap) * 8 + ((size_t)kf_mark_words(cap) + ORBFE_MAX_LEVELS + 6 * KF_WAVES) * 4;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// the sum of v over the workgroup, in every thread; red: KF_WAVES words that nobody else uses
__device__ __forceinline__ int block_sum(int v, int* red, int lane, int wave) {
  v = wave_sum(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < KF_WAVES; w++) s += red[w];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(KF_THREADS) void keyframe_insertion_kernel(const KfLaunch L) {
  extern __shared__ __attribute__((aligned(16))) uint64_t kf_smem[];
  const orbfe_kf_call& C = L.C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.x;
  uint64_t* keys = kf_smem;
  uint32_t* mark = reinterpret_cast<uint32_t*>(keys + kf_pow2(C.cap));
  float* sf = reinterpret_cast<float*>(mark + kf_mark_words(C.cap));
  int* red = reinterpret_cast<int*>(sf + ORBFE_MAX_LEVELS);           // [4][KF_WAVES]
  int* wsum = red + 4 * KF_WAVES;                                      // [2][KF_WAVES]

  const int flags = C.flags, mode = C.mode, cap = C.cap, new_cap = C.new_cap;
  const bool stats = flags & ORBFE_KF_STATISTICS, decide = flags & ORBFE_KF_DECISION, create = flags & ORBFE_KF_CREATE;
  const bool init = mode == ORBFE_KF_MODE_STEREO_INIT;
  const int n = kf_clamp(C.n[f], cap);
  const int fs = kf_source_frame(f, C.frame_shift, C.S);
  const size_t row = (size_t)f * cap;
  int32_t* asg = C.assigned ? C.assigned + row : nullptr;
  const int n_pts = asg ? kf_clamp(C.n_points[fs], C.p_cap) : 0;
  const uint8_t* records = reinterpret_cast<const uint8_t*>(C.points) + (size_t)fs * C.p_cap * C.point_stride;
  const int point_stride = C.point_stride, observed_offset = C.observed_offset;
  const float* depth = C.depth + row;
  const uint8_t* outlier = C.outlier ? C.outlier + row : nullptr;
  const float th_depth = L.cam.th_depth;
  const int n_levels = L.cam.n_levels;
  orbfe_kf_header* Hout = C.headers + f;

  auto refuse = [&]() {
    if (tid == 0) {
      orbfe_kf_header R;
      kf_header_clear(R, ORBFE_KF_REFUSED);
      *Hout = R;
      if (create) C.n_new[f] = 0;
    }
  };

  // 0. everything behind an index
  const int32_t* rslots = nullptr;
  int rkeys = 0;
  {
    bool bad = false;
    if (asg)
      for (int i = tid; i < n; i += KF_THREADS) bad = asg[i] >= n_pts || bad;
    if (decide) {
      const int32_t r = *reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(C.ref_kf) + (size_t)f * C.ref_kf_stride);
      if (r < -1 || r >= C.n_kf) bad = true;   // uniform
      else if (r >= 0) {
        const orbfe_cov_keyframe* K = C.keyframes + r;
        const int32_t n_keys = K->n_keys;
        const uint64_t at = K->slots;
        if (!(n_keys == 0 || (n_keys > 0 && at && !(at & 3)))) bad = true;   // uniform
        else {
          rslots = kf_slots_at(at);
          rkeys = n_keys;
          for (int i = tid; i < rkeys; i += KF_THREADS) bad = !kf_ref_slot_ok(rslots[i], C.n_map_points) || bad;
        }
      }
    }
    if (tid == 0) {   // constant indices: a per-lane index into a kernel argument would be private memory
#pragma unroll
      for (int k = 0; k < ORBFE_MAX_LEVELS; k++) sf[k] = L.cam.scale_factors[k];
    }
    if (__syncthreads_or(bad ? 1 : 0)) {   // uniform
      refuse();
      return;
    }
  }

  // 1. the counts and the decision
  orbfe_kf_header H;
  kf_header_clear(H, ORBFE_KF_OK);
  if (stats) {   // uniform
    const orbfe_kf_decision_in D = C.decision[f];
    const bool close_counts = decide && D.sensor != ORBFE_KF_SENSOR_MONOCULAR, only_tracking = D.only_tracking != 0;
    int inl = 0, tc = 0, ntc = 0, refm = 0;
    for (int i = tid; i < n; i += KF_THREADS) {
      const int32_t a = asg ? asg[i] : -1;
      const bool occupied = a >= 0, out = outlier && outlier[i];
      const bool observed = occupied && kf_observed(records, point_stride, observed_offset, a);
      inl += kf_inlier(occupied, out, observed, only_tracking) ? 1 : 0;
      if (close_counts && kf_close(depth[i], th_depth)) {
        const bool tracked = occupied && !out;
        tc += tracked ? 1 : 0;
        ntc += tracked ? 0 : 1;
      }
    }
    if (decide) {
      const int min_obs = kf_min_obs(D.n_kfs);
      for (int i = tid; i < rkeys; i += KF_THREADS) refm += kf_ref_counts(rslots[i], C.point_bad, C.point_observations, min_obs) ? 1 : 0;
    }
    inl = wave_sum(inl); tc = wave_sum(tc); ntc = wave_sum(ntc); refm = wave_sum(refm);
    if (lane == 0) { red[wave] = inl; red[KF_WAVES + wave] = tc; red[2 * KF_WAVES + wave] = ntc; red[3 * KF_WAVES + wave] = refm; }
    __syncthreads();
    inl = tc = ntc = refm = 0;
#pragma unroll
    for (int w = 0; w < KF_WAVES; w++) { inl += red[w]; tc += red[KF_WAVES + w]; ntc += red[2 * KF_WAVES + w]; refm += red[3 * KF_WAVES + w]; }
    __syncthreads();
    H.n_matches_inliers = inl; H.n_tracked_close = tc; H.n_non_tracked_close = ntc; H.n_ref_matches = refm;
    H.track_ok = kf_track_ok(D, inl);
    if (decide) kf_decide(D, H);
  }

  const bool run = create && (!decide || H.need) && (!init || kf_init_runs(n));   // uniform
  const bool selected_out = create && C.depth_selected;
  if (selected_out)
    for (int w = tid; w < (cap + 31) / 32; w += KF_THREADS) mark[w] = 0u;
  int n_created = 0, n_cleared = 0;
  if (run) {
    // 2. compaction in index order, then the sort
    int base = 0, within = 0, round = 0;
    for (int i0 = 0; i0 < n; i0 += KF_THREADS, round ^= 1) {
      const int i = i0 + tid;
      const float z = i < n ? depth[i] : 0.0f;
      const bool cand = kf_candidate(z);
      within += (cand && kf_within(z, th_depth)) ? 1 : 0;
      const unsigned long long hit = __ballot(cand);
      if (lane == 0) wsum[round * KF_WAVES + wave] = __popcll(hit);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < KF_WAVES; w++) {
        const int cnt = wsum[round * KF_WAVES + w];
        before += w < wave ? cnt : 0;
        total += cnt;
      }
      if (cand) keys[base + before + __popcll(hit & ((1ull << lane) - 1ull))] = kf_key(z, i);   // < n <= cap <= kf_pow2(cap)
      base += total;
    }
    const int M = base;
    const int c = block_sum(within, red, lane, wave);   // its barriers also order the keys
    const int P = kf_pow2(M);                           // <= kf_pow2(cap): M <= n <= cap
    for (int t = M + tid; t < P; t += KF_THREADS) keys[t] = KF_KEY_PAD;
    __syncthreads();
    if (!init)
      for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int t = tid; t < (P >> 1); t += KF_THREADS) {
            const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // bit j clear; its partner is lo + j < P
            const uint64_t a = keys[lo], b = keys[lo + j];
            if ((a > b) == ((lo & k) == 0)) { keys[lo] = b; keys[lo + j] = a; }
          }
          __syncthreads();
        }
    const int Lp = init ? M : kf_prefix(M, c);

    // 3. the octaves of what will be created
    bool bad = false;
    for (int j = tid; j < Lp; j += KF_THREADS) {
      const int i = kf_key_index(keys[j]);
      const int32_t a = (init || !asg) ? -1 : asg[i];
      const bool occupied = a >= 0, observed = occupied && kf_observed(records, point_stride, observed_offset, a);
      if (kf_creates(occupied, observed)) {
        const int32_t octave = C.keys_un[row + i].octave;
        bad = octave < 0 || octave >= n_levels || bad;
      }
    }
    if (__syncthreads_or(bad ? 1 : 0)) {   // uniform
      refuse();
      return;
    }

    // 4. the records, in the order of the prefix
    const orbfe_unproject_cam cam = C.cam[f];
    const float sf_top = sf[n_levels - 1];
    const int32_t id_base = C.n_points_base ? C.n_points_base[f] : 0;
    const bool frame_form = mode == ORBFE_KF_MODE_LAST_FRAME;
    int cleared = 0;
    base = 0;
    for (int j0 = 0; j0 < Lp; j0 += KF_THREADS, round ^= 1) {
      const int j = j0 + tid;
      int i = 0;
      bool creates = false, occupied = false;
      if (j < Lp) {
        i = kf_key_index(keys[j]);
        const int32_t a = (init || !asg) ? -1 : asg[i];
        occupied = a >= 0;
        creates = kf_creates(occupied, occupied && kf_observed(records, point_stride, observed_offset, a));
        if (selected_out) atomicOr(mark + (i >> 5), 1u << (i & 31));
      }
      const unsigned long long hit = __ballot(creates);
      if (lane == 0) wsum[round * KF_WAVES + wave] = __popcll(hit);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < KF_WAVES; w++) {
        const int cnt = wsum[round * KF_WAVES + w];
        before += w < wave ? cnt : 0;
        total += cnt;
      }
      if (creates) {
        const int at = base + before + __popcll(hit & ((1ull << lane) - 1ull));
        if (occupied && mode == ORBFE_KF_MODE_KEYFRAME) {   // :1002
          cleared++;
          asg[i] = -1;
        }
        if (at < new_cap) {
          const orbfe_keypoint* kp = C.keys_un + row + i;
          float v[8];
          kf_point_floats(cam, kp->x, kp->y, depth[i], sf[kp->octave], sf_top, frame_form, v);
          uint32_t* dst = reinterpret_cast<uint32_t*>(C.new_points + (size_t)f * new_cap + at);
#pragma unroll
          for (int d = 0; d < 8; d++) dst[d] = kf_float_bits(v[d]);
          dst[8] = 0u;                       // skip
          dst[9] = frame_form ? 0u : 1u;     // observed
          const uint32_t* src = reinterpret_cast<const uint32_t*>(C.desc + (row + i) * 32);
#pragma unroll
          for (int d = 0; d < 8; d++) dst[10 + d] = src[d];
          C.new_index[(size_t)f * new_cap + at] = i;
          if (asg && !frame_form) asg[i] = id_base + at;
        }
      }
      base += total;
    }
    n_created = base;
    n_cleared = block_sum(cleared, red, lane, wave);   // its barriers also order the marks
    H.M = M; H.c = c; H.L = Lp; H.n_created = n_created; H.n_cleared = n_cleared;
    if (n_created > new_cap) H.status = ORBFE_KF_OVERFLOW;
  } else {
    __syncthreads();   // the marks are zero
  }

  // 5. depth_selected and the header
  if (selected_out) {
    float* out = C.depth_selected + row;
    for (int i = tid; i < cap; i += KF_THREADS) out[i] = ((mark[i >> 5] >> (i & 31)) & 1u) ? depth[i] : -1.0f;
  }
  if (tid == 0) {
    *Hout = H;
    if (create) C.n_new[f] = n_created < new_cap ? n_created : new_cap;
  }
}

// hipFuncSetAttribute applies to the device that is current when it is called; one bit per device ordinal (covis_kernels.hip)
hipError_t raise_dynamic_lds(const void* kernel, int bytes, std::atomic<unsigned long long>& done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  const unsigned long long bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
  return e;
}

}  // namespace

hipError_t orbfe_launch_keyframe_insertion(const KfLaunch& L, hipStream_t s) {
  if (L.C.S <= 0) return hipSuccess;
  static std::atomic<unsigned long long> raised{0};
  const hipError_t e = raise_dynamic_lds(reinterpret_cast<const void*>(keyframe_insertion_kernel), (int)kf_lds_bytes(ORBFE_KF_MAX_CAP), raised);
  if (e != hipSuccess) return e;   // nothing is launched
  hipLaunchKernelGGL(keyframe_insertion_kernel, dim3((unsigned)L.C.S), dim3(KF_THREADS), kf_lds_bytes(L.C.cap), s, L);
  return hipSuccess;
}
