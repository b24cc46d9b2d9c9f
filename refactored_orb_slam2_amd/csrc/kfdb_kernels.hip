// kfdb_kernels.hip -- KeyFrameDatabase::DetectRelocalizationCandidates / DetectLoopCandidates (L/src/KeyFrameDatabase.cc:72-304) for
// Q queries against every entry of the database.  The reference walks an inverted file with std::lists; here the same sets are
// evaluated per (query, slot), a slot being an entry's add sequence number.  The arithmetic is kfdb_internal.h; this file stages,
// distributes, scans and orders.
//   kfdb_common_kernel<false>  grid (ceil(n_slots / KFDB_STRIP), Q).  The workgroup stages its query's sorted word ids in LDS (at most
//     4096 x 4 B) and walks a strip of KFDB_STRIP slots, KFDB_STRIP / KFDB_WAVES per wave.  A wave's lanes stride over the entry's
//     words, each lane looks its word up in the staged ids by bisection, and the ballot of 64 verdicts gives the count (popcount) and
//     the first common word (entry ids ascend: the lowest set lane of the first non-empty ballot).  Erased slots and, for a loop
//     query, entries whose id is in the query's connected set get 0: they never enter lKFsSharingWords.
//   kfdb_threshold_kernel  one workgroup per query: |S|, maxCommonWords, minCommonWords.
//   kfdb_score_kernel      grid as the common pass.  Wave 0 looks at the strip's 64 counts; a workgroup without a scored slot ends
//     there (most do: only entries above 0.8 x max are scored).  Otherwise it stages ids AND values (48 KiB) and its waves take the
//     scored slots in turn.  The terms of 64 entry words are computed in parallel; they are ADDED one by one in lane order by every
//     lane alike (a wave-uniform loop over the ballot's bits), which is the ascending word order of L1Scoring::score.
//   kfdb_carry_kernel      (relocalisation) one thread per slot walks the batch in query order: carried[q][slot] is the mRelocScore
//     query q finds there (the last scored value of an earlier query of the batch, else the handle's state), and the state moves to
//     the value behind the last query.
//   kfdb_select_kernel     one workgroup per query: lScoreAndMatch, the accumulation over the covisible neighbours, bestAccScore (a
//     maximum: `if (acc > best) best = acc` from a non-negative start over non-negative floats), the 0.75 threshold, the order
//     (first common word, slot) of lKFsSharingWords by counting smaller keys, the first-occurrence rule, the outputs.  Lists are
//     compacted in slot order with ballot scans.
// No atomics, no scratch; nothing read was written by another workgroup of the same launch.  A query's bytes depend on the database,
// on the query and, for relocalisation, on the carried state only -- not on Q or on the position in the batch.
#include "kfdb_internal.h"

static_assert(sizeof(KfdbSlot) == 24 && sizeof(orbfe_kfdb_query_info) == 32, "record layout");
static_assert(KFDB_STRIP == 64 && KFDB_STRIP % KFDB_WAVES == 0, "wave 0 scans a strip with one lane per slot");

__device__ __forceinline__ int kfdb_clamp(int v, int hi) { return min(max(v, 0), hi); }

// index of `id` in the ascending list s[0 .. n), or -1
__device__ __forceinline__ int kfdb_find(const int32_t* s, int n, int id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] < id) lo = mid + 1; else hi = mid;
  }
  return (lo < n && s[lo] == id) ? lo : -1;
}

__device__ __forceinline__ bool kfdb_connected(const int64_t* c, int n, int64_t id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c[mid] < id) lo = mid + 1; else hi = mid;
  }
  return lo < n && c[lo] == id;
}

// FUSED (the measured alternative, orbfe_debug_kfdb_arrangement(1)): the values are staged too and the L1 sum of EVERY pair with a
// common word is formed right here, in the same order as kfdb_pair_sum forms it; the score pass then only copies the dense outputs.
template <bool FUSED>
__global__ __launch_bounds__(KFDB_THREADS) void kfdb_common_kernel(KfdbLaunch L) {
  extern __shared__ double s_dyn[];   // FUSED: [4096] values, then [4096] ids; else the ids alone
  double* s_vals = s_dyn;
  int32_t* s_ids = FUSED ? reinterpret_cast<int32_t*>(s_dyn + ORBFE_KFDB_MAX_WORDS) : reinterpret_cast<int32_t*>(s_dyn);
  const int q = blockIdx.y, n = L.n_slots;
  const int q0 = L.q_off[q], nq = kfdb_clamp(L.q_off[q + 1] - q0, ORBFE_KFDB_MAX_WORDS);
  for (int i = threadIdx.x; i < nq; i += KFDB_THREADS) {
    s_ids[i] = L.q_ids[q0 + i];
    if (FUSED) s_vals[i] = L.q_vals[q0 + i];
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t* conn = nullptr;
  int n_conn = 0;
  if (L.loop) {
    const int c0 = L.c_off[q];
    n_conn = max(L.c_off[q + 1] - c0, 0);
    conn = L.c_ids + c0;
  }
  const int per = KFDB_STRIP / KFDB_WAVES;
  const int s0 = (int)blockIdx.x * KFDB_STRIP + wave * per;
  for (int s = s0; s < min(s0 + per, n); s++) {
    const KfdbSlot sl = L.slots[s];
    int count = 0, first = -1;
    double sum = 0.0;
    if (sl.live && !(n_conn > 0 && kfdb_connected(conn, n_conn, sl.id))) {
      const int len = kfdb_clamp(sl.len, ORBFE_KFDB_MAX_WORDS);
      const int32_t* e = L.ids + sl.off;
      for (int base = 0; base < len; base += 64) {
        const int i = base + lane;
        int id = -1;
        bool hit = false;
        double term = 0.0;
        if (i < len) {
          id = e[i];
          const int p = kfdb_find(s_ids, nq, id);
          hit = p >= 0;
          if (FUSED && hit) term = kfdb_l1_term(s_vals[p], L.vals[sl.off + i]);
        }
        uint64_t b = __ballot(hit);
        if (b) {
          if (first < 0) first = __shfl(id, __ffsll((unsigned long long)b) - 1);
          count += __popcll(b);
          if (FUSED)
            for (; b; b &= b - 1) sum += __shfl(term, __ffsll((unsigned long long)b) - 1);
        }
      }
    }
    if (lane == 0) {
      L.words[(size_t)q * n + s] = count;
      L.first[(size_t)q * n + s] = first;
      if (FUSED) L.score[(size_t)q * n + s] = kfdb_l1_finish(sum);
    }
  }
}

__global__ __launch_bounds__(KFDB_THREADS) void kfdb_threshold_kernel(KfdbLaunch L) {
  __shared__ int s_max[KFDB_WAVES], s_cnt[KFDB_WAVES];
  const int q = blockIdx.x, n = L.n_slots;
  const int32_t* words = L.words + (size_t)q * n;
  int mx = 0, cnt = 0;
  for (int s = threadIdx.x; s < n; s += KFDB_THREADS) {
    const int w = words[s];
    mx = max(mx, w);
    cnt += w > 0;
  }
  for (int d = 32; d > 0; d >>= 1) {
    mx = max(mx, __shfl_xor(mx, d));
    cnt += __shfl_xor(cnt, d);
  }
  if ((threadIdx.x & 63) == 0) {
    s_max[threadIdx.x >> 6] = mx;
    s_cnt[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = 0; cnt = 0;
    for (int k = 0; k < KFDB_WAVES; k++) {
      mx = max(mx, s_max[k]);
      cnt += s_cnt[k];
    }
    L.qstat[3 * q] = cnt;
    L.qstat[3 * q + 1] = mx;
    L.qstat[3 * q + 2] = kfdb_min_common_words(mx);
  }
}

// wave-uniform: the sum of kfdb_l1_term over the common words of the staged query and one entry, added in ascending word order
__device__ __forceinline__ double kfdb_pair_sum(const int32_t* s_ids, const double* s_vals, int nq, const int32_t* e_ids,
                                                const double* e_vals, int len, int lane) {
  double sum = 0.0;
  for (int base = 0; base < len; base += 64) {
    const int i = base + lane;
    double term = 0.0;
    bool hit = false;
    if (i < len) {
      const int p = kfdb_find(s_ids, nq, e_ids[i]);
      if (p >= 0) {
        hit = true;
        term = kfdb_l1_term(s_vals[p], e_vals[i]);
      }
    }
    uint64_t b = __ballot(hit);
    while (b) {   // uniform: every lane adds the same terms in the same order
      sum += __shfl(term, __ffsll((unsigned long long)b) - 1);
      b &= b - 1;
    }
  }
  return sum;
}

// stages query q: values first (8-byte aligned), ids behind them
__device__ __forceinline__ int kfdb_stage_query(const KfdbLaunch& L, int q, double* s_vals, int32_t* s_ids) {
  const int q0 = L.q_off[q], nq = kfdb_clamp(L.q_off[q + 1] - q0, ORBFE_KFDB_MAX_WORDS);
  for (int i = threadIdx.x; i < nq; i += KFDB_THREADS) {
    s_ids[i] = L.q_ids[q0 + i];
    s_vals[i] = L.q_vals[q0 + i];
  }
  return nq;
}

__global__ __launch_bounds__(KFDB_THREADS) void kfdb_score_kernel(KfdbLaunch L) {
  extern __shared__ double s_vals[];   // [4096] values, then [4096] ids
  __shared__ unsigned long long s_mask;
  int32_t* s_ids = reinterpret_cast<int32_t*>(s_vals + ORBFE_KFDB_MAX_WORDS);
  const int q = blockIdx.y, n = L.n_slots;
  const int minc = L.qstat[3 * q + 2];
  const int base = (int)blockIdx.x * KFDB_STRIP;
  if (threadIdx.x < 64) {
    const int s = base + (int)threadIdx.x;
    const uint64_t b = __ballot(s < n && L.words[(size_t)q * n + min(s, n - 1)] > minc);
    if (threadIdx.x == 0) s_mask = b;
  }
  __syncthreads();
  const uint64_t mask = s_mask;
  if (!mask) return;   // uniform
  if (L.fused) {       // the common pass has scored every pair: only the dense outputs are left
    const size_t o = (size_t)q * n + base + threadIdx.x;
    if (threadIdx.x < 64 && ((mask >> threadIdx.x) & 1)) {
      if (L.o_words) L.o_words[o] = L.words[o];
      if (L.o_scores) L.o_scores[o] = L.score[o];
    }
    return;
  }
  const int nq = kfdb_stage_query(L, q, s_vals, s_ids);
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  int k = 0;
  for (uint64_t b = mask; b; b &= b - 1, k++) {
    if ((k & (KFDB_WAVES - 1)) != wave) continue;
    const int s = base + __ffsll((unsigned long long)b) - 1;
    const KfdbSlot sl = L.slots[s];
    const float si = kfdb_l1_finish(kfdb_pair_sum(s_ids, s_vals, nq, L.ids + sl.off, L.vals + sl.off, kfdb_clamp(sl.len, ORBFE_KFDB_MAX_WORDS), lane));
    if (lane == 0) {
      const size_t o = (size_t)q * n + s;
      L.score[o] = si;
      if (L.o_words) L.o_words[o] = L.words[o];
      if (L.o_scores) L.o_scores[o] = si;
    }
  }
}

__global__ __launch_bounds__(KFDB_THREADS) void kfdb_carry_kernel(KfdbLaunch L) {
  const int s = blockIdx.x * KFDB_THREADS + threadIdx.x, n = L.n_slots;
  if (s >= n) return;
  float c = L.state[s];
  for (int q = 0; q < L.Q; q++) {
    const size_t o = (size_t)q * n + s;
    L.carried[o] = c;
    if (L.words[o] > L.qstat[3 * q + 2]) c = L.score[o];
  }
  L.state[s] = c;
}

// position of this thread's flag among the workgroup's set flags, in thread order; total = how many are set.  Called by all threads.
__device__ __forceinline__ int kfdb_scan(bool f, int* s_cnt, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t b = __ballot(f);
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();   // the previous scan's counts have been read
  if (lane == 0) s_cnt[w] = __popcll(b);
  __syncthreads();
  int off = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < KFDB_WAVES; k++) {
    const int c = s_cnt[k];
    if (k < w) off += c;
    total += c;
  }
  return off + before;
}

__global__ __launch_bounds__(KFDB_THREADS) void kfdb_select_kernel(KfdbLaunch L) {
  __shared__ int s_cnt[KFDB_WAVES];
  __shared__ float s_max[KFDB_WAVES];
  const int q = blockIdx.x, n = L.n_slots, tid = threadIdx.x;
  const size_t row = (size_t)q * n;
  const int32_t* words = L.words + row;
  const int32_t* first = L.first + row;
  const float* score = L.score + row;
  const float* carried = L.carried + row;
  int32_t* A = L.sel[0] + row;                                 // lScoreAndMatch: slots, in slot order; later the ordered best slots
  float* ACC = reinterpret_cast<float*>(L.sel[1] + row);       // accScore of A[i]
  int32_t* BEST = L.sel[2] + row;                              // pBestKF of A[i]
  int32_t* RF = L.sel[3] + row;                                // retained: first common word,
  int32_t* RS = L.sel[4] + row;                                //           slot,
  int32_t* RB = L.sel[5] + row;                                //           best slot
  const int n_sharing = L.qstat[3 * q], maxc = L.qstat[3 * q + 1], minc = L.qstat[3 * q + 2];
  const bool loop = L.loop != 0;
  const float min_score = loop ? L.min_score[q] : 0.0f;

  int M = 0, n_scored = 0;
  for (int base = 0; base < n; base += KFDB_THREADS) {
    const int s = base + tid;
    const bool scored = s < n && words[s] > minc;
    const bool match = scored && (!loop || score[s] >= min_score);
    int tot;
    const int pos = kfdb_scan(match, s_cnt, tot);
    if (match) A[M + pos] = s;
    M += tot;
    kfdb_scan(scored, s_cnt, tot);
    n_scored += tot;
  }
  __syncthreads();

  float best_acc = min_score;   // bestAccScore = minScore (:142) or 0 (:255)
  for (int i = tid; i < M; i += KFDB_THREADS) {
    const int s = A[i];
    KfdbAcc a;
    kfdb_acc_start(a, score[s], s);
    for (int k = 0; k < KFDB_NEIGHBOURS; k++) {
      const int s2 = L.neigh[(size_t)s * KFDB_NEIGHBOURS + k];
      if (s2 < 0 || s2 >= n) continue;
      const int w2 = words[s2];
      if (w2 <= 0) continue;   // not in S
      const bool scored2 = w2 > minc;
      if (loop && !scored2) continue;
      kfdb_acc_neighbour(a, scored2 ? score[s2] : carried[s2], s2);
    }
    ACC[i] = a.acc;
    BEST[i] = a.best_slot;
    best_acc = fmaxf(best_acc, a.acc);
  }
  for (int d = 32; d > 0; d >>= 1) best_acc = fmaxf(best_acc, __shfl_xor(best_acc, d));
  if ((tid & 63) == 0) s_max[tid >> 6] = best_acc;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KFDB_WAVES; k++) best_acc = fmaxf(best_acc, s_max[k]);
  const float retain = kfdb_min_score_to_retain(best_acc);

  int R = 0;
  for (int base = 0; base < M; base += KFDB_THREADS) {
    const int i = base + tid;
    const bool keep = i < M && ACC[i] > retain;
    int tot;
    const int pos = kfdb_scan(keep, s_cnt, tot);
    if (keep) {
      const int s = A[i];
      RF[R + pos] = first[s];
      RS[R + pos] = s;
      RB[R + pos] = BEST[i];
    }
    R += tot;
  }
  __syncthreads();   // A is read no more: it takes the ordered list

  for (int i = tid; i < R; i += KFDB_THREADS) {
    const int f = RF[i], s = RS[i];
    int rank = 0;
    for (int j = 0; j < R; j++) {
      const int fj = RF[j];
      rank += fj < f || (fj == f && RS[j] < s);
    }
    A[rank] = RB[i];
  }
  __syncthreads();

  int C = 0;
  for (int base = 0; base < R; base += KFDB_THREADS) {
    const int r = base + tid;
    bool keep = r < R;
    int b = -1;
    if (keep) {
      b = A[r];
      for (int j = 0; j < r; j++)
        if (A[j] == b) {
          keep = false;
          break;
        }
    }
    int tot;
    const int pos = kfdb_scan(keep, s_cnt, tot);
    if (keep && C + pos < L.cand_cap) L.cand[(size_t)q * L.cand_cap + C + pos] = L.slots[b].id;
    C += tot;
  }
  if (tid == 0) {
    L.n_cand[q] = C;
    if (L.info) {
      orbfe_kfdb_query_info r;
      r.n_sharing = n_sharing;
      r.max_common_words = maxc;
      r.min_common_words = minc;
      r.n_scored = n_scored;
      r.n_matches = M;
      r.best_acc_score = M > 0 ? best_acc : 0.0f;            // the early returns (:102, :138, :219) leave the floats at 0
      r.min_score_to_retain = M > 0 ? retain : 0.0f;
      r.n_candidates = C;
      L.info[q] = r;
    }
  }
}

__global__ __launch_bounds__(KFDB_THREADS) void kfdb_score_list_kernel(KfdbLaunch L, const int32_t* list, int m, float* out) {
  extern __shared__ double s_vals[];
  int32_t* s_ids = reinterpret_cast<int32_t*>(s_vals + ORBFE_KFDB_MAX_WORDS);
  const int nq = kfdb_stage_query(L, 0, s_vals, s_ids);
  __syncthreads();
  const int k = (int)blockIdx.x * KFDB_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= m) return;
  const int s = list[k];
  float si = ORBFE_KFDB_SCORE_UNKNOWN;
  if (s >= 0 && s < L.n_slots) {
    const KfdbSlot sl = L.slots[s];
    si = kfdb_l1_finish(kfdb_pair_sum(s_ids, s_vals, nq, L.ids + sl.off, L.vals + sl.off, kfdb_clamp(sl.len, ORBFE_KFDB_MAX_WORDS), lane));
  }
  if (lane == 0) out[k] = si;
}

#define KFDB_QUERY_LDS ((size_t)ORBFE_KFDB_MAX_WORDS * 12)

void orbfe_launch_kfdb_detect(const KfdbLaunch& L, hipStream_t s) {
  if (L.Q < 1) return;
  const int n = L.n_slots;
  const dim3 strips((n + KFDB_STRIP - 1) / KFDB_STRIP, L.Q);
  if (n > 0 && L.fused) hipLaunchKernelGGL(kfdb_common_kernel<true>, strips, dim3(KFDB_THREADS), KFDB_QUERY_LDS, s, L);
  if (n > 0 && !L.fused) hipLaunchKernelGGL(kfdb_common_kernel<false>, strips, dim3(KFDB_THREADS), (size_t)ORBFE_KFDB_MAX_WORDS * 4, s, L);
  hipLaunchKernelGGL(kfdb_threshold_kernel, dim3(L.Q), dim3(KFDB_THREADS), 0, s, L);
  if (n > 0) hipLaunchKernelGGL(kfdb_score_kernel, strips, dim3(KFDB_THREADS), L.fused ? 0 : KFDB_QUERY_LDS, s, L);
  if (n > 0 && !L.loop) hipLaunchKernelGGL(kfdb_carry_kernel, dim3((n + KFDB_THREADS - 1) / KFDB_THREADS), dim3(KFDB_THREADS), 0, s, L);
  hipLaunchKernelGGL(kfdb_select_kernel, dim3(L.Q), dim3(KFDB_THREADS), 0, s, L);
}

void orbfe_launch_kfdb_score_list(const KfdbLaunch& L, const int32_t* d_list, int m, float* d_out, hipStream_t s) {
  if (m < 1) return;
  hipLaunchKernelGGL(kfdb_score_list_kernel, dim3((m + KFDB_WAVES - 1) / KFDB_WAVES), dim3(KFDB_THREADS), KFDB_QUERY_LDS, s, L, d_list, m, d_out);
}
