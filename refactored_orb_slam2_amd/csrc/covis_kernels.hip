// covis_kernels.hip -- the covisibility counts (KeyFrame::UpdateConnections, the vote of Tracking::UpdateLocalKeyFrames) and
// LocalMapping::KeyFrameCulling for gfx950.  One subject or one problem is one workgroup of COV_THREADS threads; the rules are those of
// covis_internal.h, spread over lanes.
//
// covis_count_kernel: the counters of all keyframe rows live in LDS (n_kf words).  Slots are spread over threads, a thread walks its
// point's list and bumps the rows with integer LDS atomics, whose order does not reach the result.  One pass over the counters gives the
// header (sums and a 64-bit maximum); the rows that have an entry are gathered into the sort area in arrival order with their keys and
// a bitonic network orders them, so the output order comes from the keys alone.  When more entries exist than conn_cap, the conn_cap-th
// greatest key is found first by bisection -- over the weight, then over the order among the rows of that weight --, each round one
// count over the counters, and only keys from it upwards are gathered.
// covis_cull_kernel: the culled set is one bit per row in LDS.  The local rows are walked in order with workgroup barriers between
// them; slots are spread over threads, each thread reads its point's state off the point's list (cov_cull_slot); the two counts are
// summed within a wave by shuffles and across waves by one LDS add per wave.
#include <atomic>

#include "covis_internal.h"

namespace {

// all LDS is dynamic and carved at multiples of 16 bytes
struct CountLds {
  unsigned long long* keys;   // [cap2]
  int32_t* rows;              // [cap2]
  unsigned long long* best;   // the greatest cov_key_max
  int* word;                  // [0] refused [1] n_counted [2] n_ordered [3] n_entries [4] gathered [5] kf_max [6] round count
  uint32_t* counter;          // [n_kf]
};
__host__ __device__ inline int cov_cap2(int conn_cap) {
  int c = 4;
  while (c < conn_cap) c <<= 1;
  return c;
}
__host__ __device__ inline size_t cov_count_lds_bytes(int n_kf, int conn_cap) {
  return (size_t)cov_cap2(conn_cap) * 12 + 64 + (((size_t)n_kf * 4 + 15) & ~(size_t)15);
}

__device__ __forceinline__ uint64_t row_key(const CovTables& T, const uint32_t* counter, int mode, int r) {
  const uint32_t w = counter[r];
  return w ? cov_entry_key(mode, w, T.kf_order[r], T.kf_bad[r] != 0) : 0;
}

__global__ __launch_bounds__(COV_THREADS) void covis_count_kernel(const CovCountLaunch L) {
  extern __shared__ __attribute__((aligned(16))) uint8_t cov_smem[];
  const CovTables& T = L.T;
  const int tid = threadIdx.x, s = blockIdx.x, n_kf = T.n_kf, cap = L.conn_cap, cap2 = cov_cap2(cap);
  CountLds D;
  D.keys = reinterpret_cast<unsigned long long*>(cov_smem);
  D.rows = reinterpret_cast<int32_t*>(cov_smem + (size_t)cap2 * 8);
  D.best = reinterpret_cast<unsigned long long*>(cov_smem + (size_t)cap2 * 12);
  D.word = reinterpret_cast<int*>(cov_smem + (size_t)cap2 * 12 + 8);
  D.counter = reinterpret_cast<uint32_t*>(cov_smem + (size_t)cap2 * 12 + 64);

  const orbfe_cov_subject S = L.subjects[s];
  orbfe_cov_header* H = L.headers + s;
  orbfe_cov_entry* E = L.entries + (size_t)s * cap;
  if (!cov_subject_ok(S, L.n_slots_total, n_kf)) {   // uniform
    if (tid == 0) cov_header_refused(*H);
    return;
  }
  for (int r = tid; r < n_kf; r += COV_THREADS) D.counter[r] = 0u;
  if (tid == 0) *D.best = 0ull;
  if (tid < 7) D.word[tid] = tid == 5 ? -1 : 0;
  __syncthreads();

  // 1. the histogram
  const int32_t self = S.mode == ORBFE_COV_VOTES ? -1 : S.self;
  uint32_t* counter = D.counter;
  bool ok = true;
  for (int i = tid; i < S.n_slots; i += COV_THREADS)
    ok = cov_count_slot(T, L.slots[S.slot_offset + i], self, [counter](int32_t kf) { atomicAdd(&counter[kf], 1u); }) && ok;
  if (!ok) D.word[0] = 1;
  __syncthreads();
  if (D.word[0]) {   // uniform
    if (tid == 0) cov_header_refused(*H);
    return;
  }

  // 2. the header: every observed row has an order in range (cov_count_slot)
  int n_counted = 0, n_ordered = 0, n_entries = 0;
  unsigned long long best = 0ull;
  for (int r = tid; r < n_kf; r += COV_THREADS) {
    const uint32_t w = counter[r];
    if (!w) continue;
    n_counted++;
    const int32_t order = T.kf_order[r];
    if (!cov_entry_key(S.mode, w, order, T.kf_bad[r] != 0)) continue;
    n_entries++;
    n_ordered += (S.mode == ORBFE_COV_VOTES || cov_ordered(w)) ? 1 : 0;
    const unsigned long long m = cov_key_max(w, order);
    best = m > best ? m : best;
  }
  if (n_counted) atomicAdd(&D.word[1], n_counted);
  if (n_ordered) atomicAdd(&D.word[2], n_ordered);
  if (n_entries) atomicAdd(&D.word[3], n_entries);
  if (best) atomicMax(D.best, best);
  __syncthreads();
  n_counted = D.word[1]; n_ordered = D.word[2]; n_entries = D.word[3]; best = *D.best;
  for (int r = tid; r < n_kf; r += COV_THREADS) {
    const uint32_t w = counter[r];
    if (w && best && cov_entry_key(S.mode, w, T.kf_order[r], T.kf_bad[r] != 0) && cov_key_max(w, T.kf_order[r]) == best) D.word[5] = r;
  }
  const int n_write = n_entries < cap ? n_entries : cap;

  // 3. with more entries than room: the least key that is written, the greatest `floor` with |{key >= floor}| >= cap.  CONNECTIONS
  //    finds the weight of the cut first, over the counters in LDS alone (log2 of the greatest weight rounds); then the order, which
  //    lies in [0, n_kf), decides among the rows of that weight (15 rounds at most).  A vote's key is its order alone.
  unsigned long long floor_key = 1ull;
  if (n_entries > cap) {   // uniform
    auto count_rows = [&](auto hit) {   // how many rows satisfy `hit`, the same number in every thread
      __syncthreads();
      if (tid == 0) D.word[6] = 0;
      __syncthreads();
      int c = 0;
      for (int r = tid; r < n_kf; r += COV_THREADS) c += hit(r) ? 1 : 0;
      if (c) atomicAdd(&D.word[6], c);
      __syncthreads();
      return D.word[6];
    };
    unsigned long long lo, hi;
    if (S.mode == ORBFE_COV_CONNECTIONS) {
      uint32_t wlo = 1u, whi = (uint32_t)(best >> 32);
      while (wlo < whi) {
        const uint32_t mid = wlo + ((whi - wlo + 1u) >> 1);
        if (count_rows([&](int r) { return counter[r] >= mid; }) >= cap) wlo = mid; else whi = mid - 1u;
      }
      lo = (unsigned long long)wlo << 32;
      hi = lo | (unsigned long long)(uint32_t)(n_kf - 1);
    } else {
      hi = 0xffffffffull;
      lo = hi - (unsigned long long)(uint32_t)(n_kf - 1);
    }
    while (lo < hi) {
      const unsigned long long mid = lo + ((hi - lo + 1ull) >> 1);
      if (count_rows([&](int r) { return row_key(T, counter, S.mode, r) >= mid; }) >= cap) lo = mid; else hi = mid - 1ull;
    }
    floor_key = lo;
  }
  __syncthreads();

  // 4. gather in arrival order, pad, order by key descending
  int m = 4;
  while (m < n_write) m <<= 1;   // <= cap2
  for (int r = tid; r < n_kf; r += COV_THREADS) {
    const unsigned long long key = row_key(T, counter, S.mode, r);
    if (key < floor_key) continue;
    const int at = atomicAdd(&D.word[4], 1);
    if (at < m) { D.keys[at] = key; D.rows[at] = r; }   // at >= n_write: equal keys, outside the stated domain
  }
  __syncthreads();
  const int gathered = D.word[4] < m ? D.word[4] : m;
  for (int e = gathered + tid; e < m; e += COV_THREADS) { D.keys[e] = 0ull; D.rows[e] = -1; }
  __syncthreads();
  for (int k = 2; k <= m; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = tid; e < m; e += COV_THREADS) {
        const int x = e ^ j;
        if (x > e) {
          const unsigned long long a = D.keys[e], b = D.keys[x];
          const bool descending = (e & k) == 0;
          if (descending ? a < b : a > b) {
            D.keys[e] = b; D.keys[x] = a;
            const int32_t t = D.rows[e]; D.rows[e] = D.rows[x]; D.rows[x] = t;
          }
        }
      }
      __syncthreads();
    }

  // 5. out
  for (int e = tid; e < n_write; e += COV_THREADS) {
    const int32_t r = D.rows[e];
    if (r < 0) continue;
    E[e].kf = r;
    E[e].weight = (int32_t)counter[r];
  }
  if (tid == 0) {
    H->n_counted = n_counted; H->n_ordered = n_ordered; H->kf_max = D.word[5]; H->w_max = (int32_t)(best >> 32);
    H->status = n_counted == 0 ? ORBFE_COV_EMPTY : n_entries > cap ? ORBFE_COV_OVERFLOW : ORBFE_COV_OK;
    H->n_written = n_write;
    H->single = (S.mode == ORBFE_COV_CONNECTIONS && n_ordered == 0 && n_counted > 0) ? 1 : 0;
    H->reserved = 0;
  }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(COV_THREADS) void covis_cull_kernel(const CovCullLaunch L) {
  extern __shared__ __attribute__((aligned(16))) uint8_t cov_smem[];
  uint32_t* culled = reinterpret_cast<uint32_t*>(cov_smem);           // [ORBFE_COV_MAX_KEYFRAMES / 32]
  int* sum = reinterpret_cast<int*>(cov_smem + ORBFE_COV_MAX_KEYFRAMES / 8);   // [0] nMPs [1] nRedundant [2] refused
  const CovTables& T = L.T;
  const int tid = threadIdx.x, lane = tid & 63;
  const orbfe_cov_problem P = L.problems[blockIdx.x];
  if (!cov_problem_ok(P, L.n_local_total)) return;   // uniform
  for (int w = tid; w < (T.n_kf + 31) / 32; w += COV_THREADS) culled[w] = 0u;
  if (tid < 3) sum[tid] = 0;
  __syncthreads();
  for (int j = 0; j < P.n_local; j++) {
    const int32_t k = L.local[P.local_offset + j];
    orbfe_cov_verdict* V = L.verdicts + P.local_offset + j;
    int verdict = ORBFE_COV_ROW_REFUSED;
    orbfe_cov_keyframe K = {};
    bool walk = false;   // everything up to here is uniform
    if (cov_row_ok(k, T.n_kf)) {
      K = T.kfs[k];
      if (K.flags & ORBFE_COV_IS_ID0) verdict = ORBFE_COV_SKIPPED_ID0;
      else walk = cov_keyframe_ok(K, P.monocular);
    }
    if (!walk) {
      if (tid == 0) { V->n_mps = 0; V->n_redundant = 0; V->verdict = verdict; V->reserved = 0; }
      continue;
    }
    int n_mps = 0, n_red = 0, refused = 0;
    for (int i = tid; i < K.n_keys; i += COV_THREADS) {
      const int r = cov_cull_slot(T, culled, k, K, i, P.monocular);
      if (r < 0) refused = 1; else { n_mps += r & 1; n_red += r >> 1; }
    }
    n_mps = wave_sum(n_mps); n_red = wave_sum(n_red); refused = wave_sum(refused);
    if (lane == 0) {
      if (n_mps) atomicAdd(&sum[0], n_mps);
      if (n_red) atomicAdd(&sum[1], n_red);
      if (refused) atomicAdd(&sum[2], refused);
    }
    __syncthreads();
    if (tid == 0) {
      const bool bad = sum[2] != 0;
      n_mps = bad ? 0 : sum[0]; n_red = bad ? 0 : sum[1];
      verdict = bad ? ORBFE_COV_ROW_REFUSED : cov_verdict(n_red, n_mps, K.flags);
      V->n_mps = n_mps; V->n_redundant = n_red; V->verdict = verdict; V->reserved = 0;
      if (verdict == ORBFE_COV_CULLED) culled[k >> 5] |= 1u << (k & 31);
      sum[0] = sum[1] = sum[2] = 0;
    }
    __syncthreads();
  }
}

// hipFuncSetAttribute applies to the device that is current when it is called; one bit per device ordinal, set only once the limit
// has been raised there, so that a failure is reported by every call and not by the first alone
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

hipError_t orbfe_launch_covis_count(const CovCountLaunch& L, hipStream_t s) {
  if (L.S <= 0) return hipSuccess;
  static std::atomic<unsigned long long> raised{0};
  const hipError_t e = raise_dynamic_lds(reinterpret_cast<const void*>(covis_count_kernel),
                                         (int)cov_count_lds_bytes(ORBFE_COV_MAX_KEYFRAMES, ORBFE_COV_MAX_CONN), raised);
  if (e != hipSuccess) return e;   // nothing is launched
  hipLaunchKernelGGL(covis_count_kernel, dim3((unsigned)L.S), dim3(COV_THREADS), cov_count_lds_bytes(L.T.n_kf, L.conn_cap), s, L);
  return hipSuccess;
}

void orbfe_launch_covis_cull(const CovCullLaunch& L, hipStream_t s) {
  if (L.Q <= 0) return;
  hipLaunchKernelGGL(covis_cull_kernel, dim3((unsigned)L.Q), dim3(COV_THREADS), ORBFE_COV_MAX_KEYFRAMES / 8 + 16, s, L);
}
