// vocab_train_kernels.hip -- DBoW2::TemplatedVocabulary::create on gfx950: hierarchical k-medians in Hamming space, one level of the
// tree at a time with every node of the level in flight (D/include/DBoW2/TemplatedVocabulary.h:640-994; the arithmetic is in
// vocab_train_internal.h).  The descriptors stay where they are; a permutation sorted by node makes a node a contiguous segment in
// original order, and a stable segmented partition after each level makes the child segments.
//
// Two forms evaluate the same integers:
//   wide     a segment is walked in chunks of VT_CHUNK positions by a grid of workgroups.  Seeding: a pass that updates min_dists and
//            leaves one sum per chunk, then one workgroup per segment that sums the chunk sums in order, draws the cut, finds the chunk
//            and scans inside it (a two-pass segmented scan).  A round: an association pass that counts set bits per cluster and bit
//            column in LDS and flushes them with integer atomics, then one workgroup per segment that compares, takes the majorities
//            and reports whether the segment still runs.
//   narrow   one workgroup holds a segment of at most VT_CHUNK descriptors in LDS and runs seeding and every round to convergence.
// Bit counters: a workgroup has 256 threads and a descriptor 256 bits, so thread t owns bit column t of every cluster's counters and
// walks the staged members; the member's cluster is uniform over the workgroup, the counter address is the thread's own, and no
// atomic or ballot is needed until the flush.
#include "vocab_train_internal.h"

#define T VT_THREADS

struct Desc { uint32_t w[8]; };

__device__ __forceinline__ Desc load_desc(const uint8_t* base, size_t idx) {
  const uint4* p = reinterpret_cast<const uint4*>(base + idx * 32);
  const uint4 a = p[0], b = p[1];
  Desc d;
  d.w[0] = a.x; d.w[1] = a.y; d.w[2] = a.z; d.w[3] = a.w; d.w[4] = b.x; d.w[5] = b.y; d.w[6] = b.z; d.w[7] = b.w;
  return d;
}
__device__ __forceinline__ Desc lds_desc(const uint32_t* p) {
  Desc d;
#pragma unroll
  for (int i = 0; i < 8; i++) d.w[i] = p[i];
  return d;
}
__device__ __forceinline__ void put_desc(uint32_t* p, const Desc& d) {
#pragma unroll
  for (int i = 0; i < 8; i++) p[i] = d.w[i];
}

// the first cluster at the least distance: strict `<` in cluster order (:732-743)
__device__ __forceinline__ int nearest(const Desc& d, const uint32_t* cen, int nc) {
  int best = 0, bd = vt_hamming(d.w, cen);
  for (int c = 1; c < nc; c++) {
    const int dc = vt_hamming(d.w, cen + c * 8);
    if (dc < bd) { bd = dc; best = c; }
  }
  return best;
}

// exclusive prefix of v over the workgroup in thread order; *total = the sum.  `tmp` holds 4 ints.
__device__ __forceinline__ int block_scan(int v, int* tmp, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int o = __shfl_up(inc, s, 64);
    if (lane >= s) inc += o;
  }
  __syncthreads();
  if (lane == 63) tmp[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; w++) base += tmp[w];
  *total = tmp[0] + tmp[1] + tmp[2] + tmp[3];
  return base + inc - v;
}

// bit column `t` of the staged members [0, m): cl[i] is member i's cluster (uniform), stage[i * 8 ..] its words
__device__ __forceinline__ void count_columns(const uint32_t* stage, const uint8_t* cl, int m, uint32_t* cnt, int t) {
  const int word = t >> 5, bit = t & 31;
  for (int i = 0; i < m; i++) cnt[cl[i] * 256 + t] += (stage[i * 8 + word] >> bit) & 1u;
}

// the mean of cluster c (FORB::meanValue): thread t decides bit t, a wave's ballot is eight bytes of the descriptor
__device__ __forceinline__ void write_mean(uint32_t count_t, int n_c, uint32_t* cen_c) {
  const unsigned long long m = __ballot(count_t >= (uint32_t)vt_majority(n_c));
  if ((threadIdx.x & 63) == 0) {
    cen_c[(threadIdx.x >> 6) * 2] = (uint32_t)m;
    cen_c[(threadIdx.x >> 6) * 2 + 1] = (uint32_t)(m >> 32);
  }
}

__global__ __launch_bounds__(T) void vt_init_kernel(int32_t* perm, int32_t* leaf_slot, int n) {
  const int i = blockIdx.x * T + threadIdx.x;
  if (i < n) { perm[i] = i; leaf_slot[i] = 0; }
}

// [n_frames][cap][32] with counts -> dense; one thread per 16 bytes
__global__ __launch_bounds__(T) void vt_compact_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ start, int cap,
                                                        uint8_t* __restrict__ out) {
  const int f = blockIdx.x, i = blockIdx.y * T + threadIdx.x;   // frames on x: there may be more than 65535
  const int s = start[f], n = start[f + 1] - s;
  if (i >= 2 * n) return;
  reinterpret_cast<uint4*>(out)[(size_t)s * 2 + i] = reinterpret_cast<const uint4*>(in)[(size_t)f * cap * 2 + i];
}

// one workgroup per segment: reset the state; a trivial segment (n <= k) is finished here: one cluster per feature, in order (:658-668)
__global__ __launch_bounds__(T) void vt_level_begin_kernel(VtLevel lv) {
  const int s = blockIdx.x, t = threadIdx.x;
  const VtSegment sg = lv.seg[s];
  VtSegState* st = lv.st + s;
  const bool trivial = sg.kind == VT_SEG_TRIVIAL;
  if (t == 0) {
    st->n_centres = trivial ? sg.n : 0;
    st->state = trivial ? VT_CONVERGED : VT_RUNNING;
    st->rounds = 0; st->draws = 0; st->empty_events = 0; st->short_seeding = 0; st->changed = 0; st->reserved = 0;
    st->dist_sum = 0;
  }
  if (t < VT_MAX_K) st->size[t] = trivial && t < sg.n ? 1 : 0;
  if (trivial) {
    if (t < sg.n) {
      lv.assoc[sg.start + t] = t;
      const Desc d = load_desc(lv.desc, (size_t)lv.perm[sg.start + t]);
      uint32_t* c = reinterpret_cast<uint32_t*>(lv.centre) + ((size_t)sg.centre0 + t) * 8;
      put_desc(c, d);
    }
    return;
  }
  for (int p = t; p < sg.n; p += T) lv.assoc[sg.start + p] = -1;
  if (sg.wide) {
    uint32_t* cnt = lv.count + (size_t)sg.wide_idx * lv.k * 256;
    for (int c = 0; c < lv.k; c++) cnt[c * 256 + t] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- wide form
// centre 0: int(r / (RAND_MAX + 1.0) * n) (:853)
__global__ __launch_bounds__(64) void vt_seed_first_kernel(VtLevel lv) {
  const int s = lv.wide_seg[blockIdx.x], t = threadIdx.x;
  const VtSegment sg = lv.seg[s];
  const int idx = vt_first_index(vt_draw(lv.seed, (uint32_t)lv.level, sg.path, 0), sg.n);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(lv.desc) + (size_t)lv.perm[sg.start + idx] * 8;
  uint32_t* dst = reinterpret_cast<uint32_t*>(lv.centre) + (size_t)sg.centre0 * 8;
  if (t < 8) dst[t] = src[t];
  if (t == 0) { lv.st[s].draws = 1; lv.st[s].n_centres = 1; }
}

// min_dists against centre j - 1 and their sum per chunk (:862-881); four consecutive positions per thread
__global__ __launch_bounds__(T) void vt_seed_update_kernel(VtLevel lv, int j) {
  __shared__ int tmp[4];
  const int ci = lv.wide_chunk[blockIdx.x];
  const VtChunk ch = lv.chunk[ci];
  const VtSegment sg = lv.seg[ch.seg];
  if (lv.st[ch.seg].n_centres != j) return;   // the seeding stopped short
  const Desc cen = load_desc(lv.centre, (size_t)sg.centre0 + j - 1);
  int sum = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int p = threadIdx.x * 4 + q;
    if (p < ch.n) {
      const Desc d = load_desc(lv.desc, (size_t)lv.perm[ch.start + p]);
      int md = vt_hamming(d.w, cen.w);
      if (j > 1) md = min(md, lv.min_dist[ch.start + p]);
      lv.min_dist[ch.start + p] = md;
      sum += md;
    }
  }
  int total;
  block_scan(sum, tmp, &total);
  if (threadIdx.x == 0) lv.chunk_sum[ci] = total;
}

// one workgroup per segment: dist_sum, the cut, the chunk that holds it, the index inside (:881-903)
__global__ __launch_bounds__(T) void vt_seed_pick_kernel(VtLevel lv, int j) {
  __shared__ int tmp[4];
  __shared__ int s_chunk, s_pick, s_go;
  __shared__ long long s_rem;
  const int s = lv.wide_seg[blockIdx.x], t = threadIdx.x;
  const VtSegment sg = lv.seg[s];
  VtSegState* st = lv.st + s;
  if (st->n_centres != j) return;
  const int nch = (sg.n + VT_CHUNK - 1) / VT_CHUNK;
  if (t == 0) {
    long long dist_sum = 0;
    for (int c = 0; c < nch; c++) dist_sum += lv.chunk_sum[sg.chunk0 + c];
    st->dist_sum = dist_sum;
    s_go = dist_sum > 0;
    s_pick = sg.n - 1;   // "if none qualifies, the last index"
    s_chunk = -1;
    if (dist_sum > 0) {
      uint32_t draws = (uint32_t)st->draws;
      const long long target = vt_cut_target(vt_cut_draw(lv.seed, (uint32_t)lv.level, sg.path, &draws, dist_sum));
      st->draws = (int32_t)draws;
      long long up = 0;
      for (int c = 0; c < nch; c++) {
        const long long cs = lv.chunk_sum[sg.chunk0 + c];
        if (up + cs >= target) { s_chunk = c; s_rem = target - up; break; }
        up += cs;
      }
    } else {
      st->short_seeding = 1;
    }
  }
  __syncthreads();
  if (!s_go) return;
  if (s_chunk >= 0) {
    const VtChunk ch = lv.chunk[sg.chunk0 + s_chunk];
    int md[4], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int p = t * 4 + q;
      md[q] = p < ch.n ? lv.min_dist[ch.start + p] : 0;
      sum += md[q];
    }
    int total;
    long long inc = block_scan(sum, tmp, &total);
    const long long rem = s_rem;
    int found = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      inc += md[q];
      if (found == 0x7fffffff && inc >= rem && t * 4 + q < ch.n) found = ch.start - sg.start + t * 4 + q;
    }
    if (found != 0x7fffffff) atomicMin(&s_pick, found);
    __syncthreads();
  }
  const int idx = s_pick;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(lv.desc) + (size_t)lv.perm[sg.start + idx] * 8;
  uint32_t* dst = reinterpret_cast<uint32_t*>(lv.centre) + ((size_t)sg.centre0 + j) * 8;
  if (t < 8) dst[t] = src[t];
  if (t == 0) st->n_centres = j + 1;
}

// the association of one chunk (:722-749) and its share of the bit counters
__global__ __launch_bounds__(T) void vt_assign_kernel(VtLevel lv) {
  __shared__ uint32_t cnt[VT_MAX_K * 256];
  __shared__ uint32_t stage[T * 8];
  __shared__ uint32_t cen[VT_MAX_K * 8];
  __shared__ int sz[VT_MAX_K];
  __shared__ uint8_t cl[T];
  const VtChunk ch = lv.chunk[lv.wide_chunk[blockIdx.x]];
  const VtSegment sg = lv.seg[ch.seg];
  VtSegState* st = lv.st + ch.seg;
  if (st->state != VT_RUNNING) return;
  const int t = threadIdx.x, nc = st->n_centres;
  if (t < nc * 8) cen[t] = reinterpret_cast<const uint32_t*>(lv.centre)[(size_t)sg.centre0 * 8 + t];
  for (int c = 0; c < nc; c++) cnt[c * 256 + t] = 0;
  if (t < VT_MAX_K) sz[t] = 0;
  __syncthreads();
  int changed = 0;
  for (int base = 0; base < ch.n; base += T) {
    const int p = base + t;
    if (p < ch.n) {
      const Desc d = load_desc(lv.desc, (size_t)lv.perm[ch.start + p]);
      const int best = nearest(d, cen, nc);
      changed |= lv.assoc[ch.start + p] != best;
      lv.assoc[ch.start + p] = best;
      put_desc(stage + t * 8, d);
      cl[t] = (uint8_t)best;
      atomicAdd(&sz[best], 1);
    }
    __syncthreads();
    count_columns(stage, cl, min(T, ch.n - base), cnt, t);
    __syncthreads();
  }
  uint32_t* g = lv.count + (size_t)sg.wide_idx * lv.k * 256;
  for (int c = 0; c < nc; c++) {
    const uint32_t v = cnt[c * 256 + t];
    if (v) atomicAdd(&g[c * 256 + t], v);
  }
  if (t < nc && sz[t]) atomicAdd(&st->size[t], sz[t]);
  if (__syncthreads_or(changed) && t == 0) atomicOr(&st->changed, 1);
}

// one workgroup per segment, after an association: converged (:753-770), capped, or the means of the next round (:692-715)
__global__ __launch_bounds__(T) void vt_finish_kernel(VtLevel lv) {
  const int s = lv.wide_seg[blockIdx.x], t = threadIdx.x;
  const VtSegment sg = lv.seg[s];
  VtSegState* st = lv.st + s;
  if (st->state != VT_RUNNING) return;
  const int rounds = st->rounds + 1, changed = st->changed, nc = st->n_centres;
  __syncthreads();
  if (t == 0) st->rounds = rounds;
  if (!changed || rounds >= lv.max_iterations) {
    if (t == 0) st->state = changed ? VT_CAPPED : VT_CONVERGED;
    return;
  }
  uint32_t* g = lv.count + (size_t)sg.wide_idx * lv.k * 256;
  uint32_t* cen = reinterpret_cast<uint32_t*>(lv.centre) + (size_t)sg.centre0 * 8;
  int empty = 0;
  for (int c = 0; c < nc; c++) {
    const int n_c = st->size[c];
    if (n_c == 0) { empty++; continue; }   // an empty cluster keeps the centre it had
    write_mean(g[c * 256 + t], n_c, cen + c * 8);
    g[c * 256 + t] = 0;
  }
  __syncthreads();
  if (t < nc) st->size[t] = 0;
  if (t == 0) {
    st->empty_events += empty;
    st->changed = 0;
    atomicAdd(lv.control, 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------- narrow form
// one workgroup owns a segment of at most VT_CHUNK descriptors: seeding and every round out of LDS
__global__ __launch_bounds__(T) void vt_narrow_kernel(VtLevel lv, const int32_t* __restrict__ seg_list) {
  __shared__ uint32_t sd[VT_CHUNK * 8];
  __shared__ uint32_t cnt[VT_MAX_K * 256];
  __shared__ uint32_t cen[VT_MAX_K * 8];
  __shared__ uint16_t md[VT_CHUNK];
  __shared__ uint8_t as[VT_CHUNK];
  __shared__ int sz[VT_MAX_K];
  __shared__ int tmp[4];
  __shared__ int s_pick;
  __shared__ long long s_target;
  const int s = seg_list[blockIdx.x], t = threadIdx.x;
  const VtSegment sg = lv.seg[s];
  const int n = sg.n, k = lv.k;
  for (int p = t; p < n; p += T) {
    put_desc(sd + p * 8, load_desc(lv.desc, (size_t)lv.perm[sg.start + p]));
    as[p] = 0xff;
  }
  __syncthreads();
  // ---- k-means++ seeding (:847-909)
  uint32_t draws = 0;
  int nc = 1, short_seeding = 0;
  {
    const int idx = vt_first_index(vt_draw(lv.seed, (uint32_t)lv.level, sg.path, draws++), n);
    if (t < 8) cen[t] = sd[idx * 8 + t];
  }
  __syncthreads();
  for (int j = 1; j < k; j++) {
    const Desc c = lds_desc(cen + (j - 1) * 8);
    int m4[4], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int p = t * 4 + q;
      m4[q] = 0;
      if (p < n) {
        const Desc d = lds_desc(sd + p * 8);
        int v = vt_hamming(d.w, c.w);
        if (j > 1) v = min(v, (int)md[p]);
        md[p] = (uint16_t)v;
        m4[q] = v;
      }
      sum += m4[q];
    }
    int dist_sum;
    const int up = block_scan(sum, tmp, &dist_sum);
    if (dist_sum == 0) { short_seeding = 1; break; }   // uniform
    if (t == 0) {
      s_target = vt_cut_target(vt_cut_draw(lv.seed, (uint32_t)lv.level, sg.path, &draws, dist_sum));
      s_pick = n - 1;
    }
    __syncthreads();
    const long long target = s_target;
    int found = 0x7fffffff, inc = up;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      inc += m4[q];
      if (found == 0x7fffffff && inc >= target && t * 4 + q < n) found = t * 4 + q;
    }
    if (found != 0x7fffffff) atomicMin(&s_pick, found);
    __syncthreads();
    if (t < 8) cen[j * 8 + t] = sd[s_pick * 8 + t];
    nc = j + 1;
    __syncthreads();
  }
  // ---- rounds (:679-779)
  int rounds = 0, empty = 0, state = VT_RUNNING;
  for (;;) {
    for (int c = 0; c < nc; c++) cnt[c * 256 + t] = 0;
    if (t < VT_MAX_K) sz[t] = 0;
    __syncthreads();
    int changed = 0;
    for (int p = t; p < n; p += T) {
      const int best = nearest(lds_desc(sd + p * 8), cen, nc);
      changed |= as[p] != best;
      as[p] = (uint8_t)best;
      atomicAdd(&sz[best], 1);
    }
    __syncthreads();
    count_columns(sd, as, n, cnt, t);
    rounds++;
    changed = __syncthreads_or(changed);
    if (!changed) { state = VT_CONVERGED; break; }
    if (rounds >= lv.max_iterations) { state = VT_CAPPED; break; }
    for (int c = 0; c < nc; c++) {
      const int n_c = sz[c];
      if (n_c == 0) { empty++; continue; }
      write_mean(cnt[c * 256 + t], n_c, cen + c * 8);
    }
    __syncthreads();
  }
  // ---- what the level keeps
  VtSegState* st = lv.st + s;
  for (int p = t; p < n; p += T) lv.assoc[sg.start + p] = as[p];
  if (t < nc * 8) reinterpret_cast<uint32_t*>(lv.centre)[(size_t)sg.centre0 * 8 + t] = cen[t];
  if (t < VT_MAX_K) st->size[t] = t < nc ? sz[t] : 0;
  if (t == 0) {
    st->n_centres = nc; st->state = state; st->rounds = rounds; st->empty_events = empty; st->short_seeding = short_seeding;
  }
}

// ---------------------------------------------------------------------------------------------------------------- partition
__global__ __launch_bounds__(T) void vt_hist_kernel(VtLevel lv) {
  __shared__ int h[VT_MAX_K];
  const VtChunk ch = lv.chunk[blockIdx.x];
  const int t = threadIdx.x;
  if (t < VT_MAX_K) h[t] = 0;
  __syncthreads();
  for (int p = t; p < ch.n; p += T) atomicAdd(&h[lv.assoc[ch.start + p]], 1);
  __syncthreads();
  if (t < lv.k) lv.chunk_hist[(size_t)blockIdx.x * lv.k + t] = h[t];
}

// thread c turns the counts of cluster c over the segment's chunks into the first destination of each chunk
__global__ __launch_bounds__(64) void vt_offsets_kernel(VtLevel lv) {
  const int s = blockIdx.x, c = threadIdx.x;
  const VtSegment sg = lv.seg[s];
  const VtSegState* st = lv.st + s;
  if (c >= st->n_centres) return;
  int off = sg.start;
  for (int i = 0; i < c; i++) off += st->size[i];
  const int nch = (sg.n + VT_CHUNK - 1) / VT_CHUNK;
  for (int i = 0; i < nch; i++) {
    int32_t* h = lv.chunk_hist + (size_t)(sg.chunk0 + i) * lv.k + c;
    const int v = *h;
    *h = off;
    off += v;
  }
}

// thread c walks the chunk in order and appends the members of cluster c: stable by construction
__global__ __launch_bounds__(64) void vt_scatter_kernel(VtLevel lv) {
  __shared__ int32_t a[VT_CHUNK], f[VT_CHUNK];
  const VtChunk ch = lv.chunk[blockIdx.x];
  const VtSegment sg = lv.seg[ch.seg];
  const int t = threadIdx.x, nc = lv.st[ch.seg].n_centres;
  for (int p = t; p < ch.n; p += 64) {
    a[p] = lv.assoc[ch.start + p];
    f[p] = lv.perm[ch.start + p];
  }
  __syncthreads();
  if (t >= nc) return;
  int dst = lv.chunk_hist[(size_t)blockIdx.x * lv.k + t];
  const int slot = lv.slot_base + sg.centre0 + t;
  for (int p = 0; p < ch.n; p++)
    if (a[p] == t) {
      lv.perm_next[dst++] = f[p];
      lv.leaf_slot[f[p]] = slot;
    }
}

__global__ __launch_bounds__(T) void vt_leaf_translate_kernel(const int32_t* __restrict__ leaf_slot, const int32_t* __restrict__ slot_node,
                                                               int n, int32_t* __restrict__ leaf_node) {
  const int i = blockIdx.x * T + threadIdx.x;
  if (i < n) leaf_node[i] = slot_node[leaf_slot[i]];
}

// Ni of setNodeWeights (:960-981): a workgroup takes images g, g + gridDim.x, ... and marks their words in a bitmap of its own; the
// thread that sets a bit counts the image for the word.  Every access to the bitmap is an atomic, so all of them meet in L2.
__global__ __launch_bounds__(T) void vt_ni_kernel(const int32_t* __restrict__ word, const int32_t* __restrict__ image_start, int n_images,
                                                   int n_words, uint32_t* bitmaps, int32_t* ni) {
  uint32_t* bm = bitmaps + (size_t)blockIdx.x * ((n_words + 31) / 32);
  for (int img = blockIdx.x; img < n_images; img += gridDim.x) {
    const int b = image_start[img], e = image_start[img + 1];
    for (int i = b + (int)threadIdx.x; i < e; i += T) {
      const int w = word[i];
      const uint32_t bit = 1u << (w & 31);
      if (!(atomicOr(&bm[w >> 5], bit) & bit)) atomicAdd(&ni[w], 1);
    }
    __threadfence();
    __syncthreads();
    for (int i = b + (int)threadIdx.x; i < e; i += T) atomicAnd(&bm[word[i] >> 5], 0u);
    __threadfence();
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- launchers
void vt_launch_init(int32_t* perm, int32_t* leaf_slot, int n, hipStream_t s) {
  hipLaunchKernelGGL(vt_init_kernel, dim3((n + T - 1) / T), dim3(T), 0, s, perm, leaf_slot, n);
}
void vt_launch_compact(const uint8_t* d_desc, const int32_t* d_start, int n_frames, int cap, uint8_t* out, hipStream_t s) {
  hipLaunchKernelGGL(vt_compact_kernel, dim3(n_frames, (2 * cap + T - 1) / T), dim3(T), 0, s, d_desc, d_start, cap, out);
}
void vt_launch_level_begin(const VtLevel& lv, hipStream_t s) {
  hipLaunchKernelGGL(vt_level_begin_kernel, dim3(lv.n_seg), dim3(T), 0, s, lv);
}
void vt_launch_narrow(const VtLevel& lv, const int32_t* seg_list, int n_list, hipStream_t s) {
  if (n_list > 0) hipLaunchKernelGGL(vt_narrow_kernel, dim3(n_list), dim3(T), 0, s, lv, seg_list);
}
void vt_launch_seed_first(const VtLevel& lv, hipStream_t s) {
  hipLaunchKernelGGL(vt_seed_first_kernel, dim3(lv.n_wide), dim3(64), 0, s, lv);
}
void vt_launch_seed_step(const VtLevel& lv, int j, hipStream_t s) {
  hipLaunchKernelGGL(vt_seed_update_kernel, dim3(lv.n_wide_chunks), dim3(T), 0, s, lv, j);
  hipLaunchKernelGGL(vt_seed_pick_kernel, dim3(lv.n_wide), dim3(T), 0, s, lv, j);
}
void vt_launch_round(const VtLevel& lv, hipStream_t s) {
  hipLaunchKernelGGL(vt_assign_kernel, dim3(lv.n_wide_chunks), dim3(T), 0, s, lv);
  hipLaunchKernelGGL(vt_finish_kernel, dim3(lv.n_wide), dim3(T), 0, s, lv);
}
void vt_launch_partition(const VtLevel& lv, hipStream_t s) {
  hipLaunchKernelGGL(vt_hist_kernel, dim3(lv.n_chunks), dim3(T), 0, s, lv);
  hipLaunchKernelGGL(vt_offsets_kernel, dim3(lv.n_seg), dim3(64), 0, s, lv);
  hipLaunchKernelGGL(vt_scatter_kernel, dim3(lv.n_chunks), dim3(64), 0, s, lv);
}
void vt_launch_leaf_translate(const int32_t* leaf_slot, const int32_t* slot_node, int n, int32_t* leaf_node, hipStream_t s) {
  hipLaunchKernelGGL(vt_leaf_translate_kernel, dim3((n + T - 1) / T), dim3(T), 0, s, leaf_slot, slot_node, n, leaf_node);
}
void vt_launch_ni(const int32_t* word, const int32_t* image_start, int n_images, int n_words, int groups, uint32_t* bitmaps, int32_t* ni,
                  hipStream_t s) {
  hipLaunchKernelGGL(vt_ni_kernel, dim3(groups), dim3(T), 0, s, word, image_start, n_images, n_words, bitmaps, ni);
}
