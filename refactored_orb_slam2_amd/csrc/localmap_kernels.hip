// localmap_kernels.hip -- the local map of a tracked frame (Tracking::UpdateLocalKeyFrames behind its vote, UpdateLocalPoints, the skip
// flag of SearchLocalPoints) for gfx950.  One frame is one workgroup of LM_THREADS threads; the rules are those of
// localmap_internal.h, spread over lanes.
//
// LDS (dynamic): one mark bit per point, one per keyframe row, the list of local keyframes, two sets of per-wave counts and a few
// words.  Only the words n_points / n_kf need are zeroed.
//   1. the vote's entries become the head of the list and are marked (all threads)
//   2. the expansion is sequential over the voted entries and runs on wave 0: the ten best rows in ten lanes and one ballot, the
//      children in chunks of 64 and a ballot per chunk, the parent by every lane alike; the other waves wait at the barrier behind it
//   3. every slot of every local keyframe, of the frame and of the also-seen slice is range-checked, so that a refused frame has
//      written nothing but its header
//   4. the union: one keyframe at a time, its slots in rounds of LM_THREADS.  A thread reads its point's mark; behind a barrier the
//      marks of the round are set; a ballot per wave and the per-wave counts give each new point its place in slot order.  Reading
//      before the barrier and setting behind it keeps the result free of the atomics' order even where a keyframe names a point twice
//   5. the marks are cleared and set again for the frame's good slots and the also-seen slice; the gather copies the 72-byte
//      records as dwords, consecutive lanes consecutive dwords, and takes `skip` from the marks
#include <atomic>

#include "localmap_internal.h"

namespace {

constexpr int LM_WAVES = LM_THREADS / 64;
constexpr int LM_LIST_WORDS = (LM_LIST_MAX + 3) & ~3;

__host__ __device__ inline size_t lm_words(int n) { return ((size_t)(n + 31) / 32 + 3) & ~(size_t)3; }   // 16-byte multiples
__host__ __device__ inline size_t lm_lds_bytes(int n_kf, int n_points) {
  return (lm_words(n_points) + lm_words(n_kf) + LM_LIST_WORDS + 2 * LM_WAVES + 16) * 4;
}

__device__ __forceinline__ uint32_t lds_read(const uint32_t* p) { return *reinterpret_cast<const volatile uint32_t*>(p); }
__device__ __forceinline__ bool marked(const uint32_t* bits, int32_t i) { return (lds_read(bits + (i >> 5)) >> (i & 31)) & 1u; }
__device__ __forceinline__ void mark(uint32_t* bits, int32_t i) { atomicOr(bits + (i >> 5), lm_mask(i)); }
__device__ __forceinline__ int first_lane(unsigned long long ballot) { return __ffsll((long long)ballot) - 1; }

__global__ __launch_bounds__(LM_THREADS) void local_map_kernel(const LmLaunch L) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lm_smem[];
  const LmTables& T = L.T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.x;
  uint32_t* pbits = lm_smem;
  uint32_t* kbits = pbits + lm_words(T.n_points);
  int32_t* list = reinterpret_cast<int32_t*>(kbits + lm_words(T.n_kf));
  int* wsum = reinterpret_cast<int*>(list + LM_LIST_WORDS);   // [2][LM_WAVES]
  int* word = wsum + 2 * LM_WAVES;                                         // [0] refused [1] list length [2] stop

  orbfe_lm_header* H = L.headers + s;
  const orbfe_cov_header V = L.votes[s];
  const int vote = lm_vote_status(V, L.conn_cap, T.n_kf);
  if (vote == ORBFE_LM_EMPTY) {   // uniform
    if (tid == 0) lm_header_set(*H, 0, 0, 0, -1, 0, ORBFE_LM_EMPTY);
    return;
  }
  const orbfe_cov_subject S = L.subjects[s];
  orbfe_lm_frame F = {0, 0};
  if (L.frames) F = L.frames[s];
  auto refuse = [&]() {
    if (tid == 0) { lm_header_set(*H, 0, 0, 0, -1, 0, ORBFE_LM_REFUSED); L.n_points_out[s] = 0; }
  };
  if (vote != ORBFE_LM_OK || !lm_slice_ok(S.slot_offset, S.n_slots, T.n_slots_total) ||
      !lm_slice_ok(F.seen_offset, F.n_seen, T.n_seen_total)) {   // uniform
    refuse();
    return;
  }
  const int n_voted = V.n_written;
  const int p_words = (T.n_points + 31) / 32;
  for (int w = tid; w < p_words; w += LM_THREADS) pbits[w] = 0u;
  for (int w = tid; w < (T.n_kf + 31) / 32; w += LM_THREADS) kbits[w] = 0u;
  if (tid < 3) word[tid] = 0;
  __syncthreads();

  // 1. the voted rows
  const orbfe_cov_entry* E = L.entries + (size_t)s * L.conn_cap;
  for (int i = tid; i < n_voted; i += LM_THREADS) {
    const int32_t k = E[i].kf;
    if (lm_row_ok(k, T.n_kf)) { list[i] = k; mark(kbits, k); } else word[0] = 1;
  }
  __syncthreads();

  // 2. the expansion, on wave 0; every branch is uniform over the wave
  if (wave == 0 && !word[0]) {
    int size = n_voted, stop = ORBFE_LM_STOP_EXHAUSTED;
    bool bad = false;
    for (int i = 0; i < n_voted; i++) {
      if (lm_size_stops(size)) { stop = ORBFE_LM_STOP_SIZE; break; }
      const orbfe_lm_graph* G = T.graph + list[i];
      const int32_t parent = G->parent, child_offset = G->child_offset, n_children = G->n_children, n_best = G->n_best;
      if (n_best < 0 || n_best > ORBFE_LM_BEST || !lm_slice_ok(child_offset, n_children, T.n_children_total) || parent < -1 ||
          parent >= T.n_kf) { bad = true; break; }
      int32_t r = -1;
      bool out = false, take = false;
      if (lane < n_best) {
        r = G->best[lane];
        out = !lm_row_ok(r, T.n_kf);
        take = !out && !T.kf_bad[r] && !marked(kbits, r);
      }
      if (__ballot(out)) { bad = true; break; }
      unsigned long long hit = __ballot(take);
      if (hit) {
        const int32_t b = __shfl(r, first_lane(hit));
        if (lane == 0) { list[size] = b; mark(kbits, b); }
        size++;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
      for (int c0 = 0; c0 < n_children; c0 += 64) {
        out = take = false;
        if (c0 + lane < n_children) {
          r = T.children[child_offset + c0 + lane];
          out = !lm_row_ok(r, T.n_kf);
          take = !out && !T.kf_bad[r] && !marked(kbits, r);
        }
        if (__ballot(out)) { bad = true; break; }
        hit = __ballot(take);
        if (hit) {
          const int32_t c = __shfl(r, first_lane(hit));
          if (lane == 0) { list[size] = c; mark(kbits, c); }
          size++;
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          break;
        }
      }
      if (bad) break;
      if (parent >= 0 && !marked(kbits, parent)) {
        if (lane == 0) { list[size] = parent; mark(kbits, parent); }
        size++;
        stop = ORBFE_LM_STOP_PARENT;
        break;
      }
    }
    if (lane == 0) { word[0] = bad ? 1 : 0; word[1] = size; word[2] = stop; }
  }
  __syncthreads();
  if (word[0]) {   // uniform
    refuse();
    return;
  }
  const int n_local = word[1], stop = word[2];   // <= LM_LIST_MAX: at most 3 rows are appended per voted entry while size <= 80

  // 3. everything behind an index, before anything is written
  {
    bool ok = true;
    for (int j = 0; j < n_local; j++) {
      const orbfe_cov_keyframe* K = T.kfs + list[j];
      const int32_t n_keys = K->n_keys;
      const uint64_t at = K->slots;
      if (!(n_keys == 0 || (n_keys > 0 && at && !(at & 3)))) { ok = false; break; }   // uniform
      const int32_t* slots = lm_at<int32_t>(at);
      for (int i = tid; i < n_keys; i += LM_THREADS) ok = lm_slot_ok(slots[i], T.n_points) && ok;
    }
    for (int i = tid; i < S.n_slots; i += LM_THREADS) ok = lm_slot_ok(T.slots[S.slot_offset + i], T.n_points) && ok;
    for (int i = tid; i < F.n_seen; i += LM_THREADS) ok = lm_row_ok(T.seen[F.seen_offset + i], T.n_points) && ok;
    if (!ok) word[0] = 1;
  }
  __syncthreads();
  if (word[0]) {   // uniform
    refuse();
    return;
  }
  int32_t* out_kf = L.local_kf + (size_t)s * L.kf_cap;
  for (int j = tid; j < n_local && j < L.kf_cap; j += LM_THREADS) out_kf[j] = list[j];

  // 4. the union
  int32_t* out_p = L.local_points + (size_t)s * L.p_cap;
  int base = 0, round = 0;
  for (int j = 0; j < n_local; j++) {
    const orbfe_cov_keyframe* K = T.kfs + list[j];
    const int32_t n_keys = K->n_keys;
    const int32_t* slots = lm_at<int32_t>(K->slots);
    for (int i0 = 0; i0 < n_keys; i0 += LM_THREADS, round ^= 1) {
      const int i = i0 + tid;
      int32_t p = -1;
      bool fresh = false;
      if (i < n_keys) {
        p = slots[i];
        fresh = p >= 0 && !marked(pbits, p) && !T.point_bad[p];
      }
      __syncthreads();   // every mark of the round is read before one of them is set
      if (fresh) mark(pbits, p);
      const unsigned long long hit = __ballot(fresh);
      if (lane == 0) wsum[round * LM_WAVES + wave] = __popcll(hit);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < LM_WAVES; w++) {
        const int c = wsum[round * LM_WAVES + w];
        before += w < wave ? c : 0;
        total += c;
      }
      if (fresh) {
        const int at = base + before + __popcll(hit & ((1ull << lane) - 1ull));
        if (at < L.p_cap) out_p[at] = p;
      }
      base += total;
    }
  }
  const int n_write = base < L.p_cap ? base : L.p_cap;
  if (tid == 0) {
    L.n_points_out[s] = n_write;
    lm_header_set(*H, n_voted, n_local, base, V.kf_max, stop, (n_local > L.kf_cap || base > L.p_cap) ? ORBFE_LM_OVERFLOW : ORBFE_LM_OK);
  }
  if (!L.records) return;   // uniform

  // 5. skip and the records
  __syncthreads();   // the marks have been read, and the list's points are written
  for (int w = tid; w < p_words; w += LM_THREADS) pbits[w] = 0u;
  __syncthreads();
  for (int i = tid; i < S.n_slots; i += LM_THREADS) {
    const int32_t p = T.slots[S.slot_offset + i];
    if (p >= 0 && !T.point_bad[p]) mark(pbits, p);
  }
  for (int i = tid; i < F.n_seen; i += LM_THREADS) mark(pbits, T.seen[F.seen_offset + i]);
  __syncthreads();
  const uint32_t* src = reinterpret_cast<const uint32_t*>(L.records);
  uint32_t* dst = reinterpret_cast<uint32_t*>(L.map_points + (size_t)s * L.p_cap);
  for (int t = tid; t < n_write * LM_RECORD_DWORDS; t += LM_THREADS) {
    const int e = t / LM_RECORD_DWORDS, d = t - e * LM_RECORD_DWORDS;
    const int32_t p = out_p[e];
    dst[t] = d == LM_SKIP_DWORD ? (marked(pbits, p) ? 1u : 0u) : src[(size_t)p * LM_RECORD_DWORDS + d];
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

hipError_t orbfe_launch_local_map(const LmLaunch& L, hipStream_t s) {
  if (L.S <= 0) return hipSuccess;
  static std::atomic<unsigned long long> raised{0};
  const hipError_t e = raise_dynamic_lds(reinterpret_cast<const void*>(local_map_kernel),
                                         (int)lm_lds_bytes(ORBFE_LM_MAX_KEYFRAMES, ORBFE_LM_MAX_POINTS), raised);
  if (e != hipSuccess) return e;   // nothing is launched
  hipLaunchKernelGGL(local_map_kernel, dim3((unsigned)L.S), dim3(LM_THREADS), lm_lds_bytes(L.T.n_kf, L.T.n_points), s, L);
  return hipSuccess;
}
