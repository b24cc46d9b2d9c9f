// projection_kernels.hip -- the searches over a query's window of the frame grid, for gfx950 (MI355X, wave64).
// Kernel              replaces (reference file:line, L/ = Source/Libraries/ORB_SLAM2/)
// proj_best           best-distance loops of Fuse, Fuse(Sim3), SearchBySim3   L/src/ORBmatcher.cc:832-887,983-1011,1116-1144,1194-1222
// proj_candidates     Frame::GetFeaturesInArea + DescriptorDistance           L/src/Frame.cc:341-397
// proj_resolve        order-dependent assignment of SearchByProjection        L/src/ORBmatcher.cc:45-128,1247-1383,1385-1504
// init_resolve        SearchForInitialization                                 L/src/ORBmatcher.cc:388-492
// Compiled with -ffp-contract=off: every float expression is evaluated un-fused, as the reference does.
#include "search_device.h"   // WAVE, the wave helpers, hamming256, cell_rec_unpack, enumerate_window, rot_bin, three_maxima

// The reference's strict `dist < bestDist` walk keeps the FIRST minimum in enumeration order: with keys dist << 16 | rank that is
// the wave minimum b = wave_min_u32(key), and its payload sits in the lowest lane that holds b (L/src/ORBmatcher.cc:78-100)
__device__ __forceinline__ int first_min_lane(unsigned key, unsigned b) { return __ffsll((long long)__ballot(key == b)) - 1; }

// One wave per query, independent arg-min (no query blocks another): Fuse, Fuse(Sim3), SearchBySim3.  best = first
// minimum in GetFeaturesInArea order (strict `dist < bestDist`).
template <int GATE>
__global__ __launch_bounds__(256) void proj_best_kernel(FrameBatch F, QueryBatch Q, const float* __restrict__ inv_sigma2,
                                                        int32_t* __restrict__ best_idx, int32_t* __restrict__ best_dist) {
  __shared__ float s_inv[ORBFE_MAX_LEVELS];
  if (threadIdx.x < ORBFE_MAX_LEVELS) s_inv[threadIdx.x] = inv_sigma2 ? inv_sigma2[threadIdx.x] : 0.f;
  __syncthreads();
  const int f = blockIdx.y;
  const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qi >= Q.n[f]) return;
  const orbfe_query* qp = Q.q + (size_t)f * Q.cap + qi;
  const orbfe_query q = *qp;
  unsigned key = 0xFFFFFFFFu;
  int mine = -1;
  if (q.valid) {
    uint4 q0, q1;
    load_desc4(qp->desc, q0, q1);
    enumerate_window<GATE>(F, f, q, q0, q1, [&](int rank, int idx, int dist, int) {
      const unsigned k = ((unsigned)dist << 16) | (unsigned)min(rank, 0xffff);
      if (k < key) { key = k; mine = idx; }
    }, s_inv);
  }
  const unsigned b = wave_min_u32(key);
  int bi = -1;
  if (b != 0xFFFFFFFFu) bi = __builtin_amdgcn_readlane(mine, first_min_lane(key, b));
  if ((threadIdx.x & 63) == 0) {
    best_idx[(size_t)f * Q.cap + qi] = bi;
    best_dist[(size_t)f * Q.cap + qi] = bi >= 0 ? (int)(b >> 16) : 256;
  }
}

// Candidate lists in enumeration order, SIXTEEN LANES PER QUERY (four queries per wave).  A search window holds a handful of
// grid entries (2.8 survivors per query at th = 7), so a whole wave per query left three quarters of the lanes idle and the
// kernel latency-bound on its four dependent round trips (query, cell ranges, cell records, descriptors) at full occupancy;
// with four queries per wave a quarter of the waves make those trips.  Same order as enumerate_window: the window's grid
// columns left to right (lane c of the group fetches column c's CSR range; 16 columns per batch), entries of the concatenated
// ranges 16 at a time, survivors ranked by a ballot inside the group.
#define ORBFE_CAND_LANES 16
__global__ __launch_bounds__(256) void proj_candidates_kernel(FrameBatch F, QueryBatch Q, orbfe_cand* __restrict__ cand,
                                                               int32_t* __restrict__ n_cand, int max_cand) {
  const int f = blockIdx.y;
  constexpr int G = ORBFE_CAND_LANES;   // lanes per query
  constexpr int QPW = WAVE / G;         // queries per wave
  const int lane = threadIdx.x & (WAVE - 1), sl = lane & (G - 1), gbase = lane & ~(G - 1);
  const int qi = (blockIdx.x * 4 + (threadIdx.x >> 6)) * QPW + lane / G;
  const int nq = Q.n[f];
  // the group's query: every lane of the group reads the same record (slot min(qi, cap - 1) is always readable)
  const orbfe_query* qp = Q.q + (size_t)f * Q.cap + min(qi, Q.cap - 1);
  const float x = qp->u, y = qp->v, r = qp->radius, qur = qp->u_r;
  const int min_level = qp->min_level, max_level = qp->max_level;
  const bool live = qi < nq && qi < Q.cap;
  bool act = live && qp->valid;
  uint4 q0, q1;
  load_desc4(qp->desc, q0, q1);
  const int nMinCellX = max(0, (int)floorf((x - F.min_x - r) * F.gw_inv));
  const int nMaxCellX = min(ORBFE_GRID_COLS - 1, (int)ceilf((x - F.min_x + r) * F.gw_inv));
  const int nMinCellY = max(0, (int)floorf((y - F.min_y - r) * F.gh_inv));
  const int nMaxCellY = min(ORBFE_GRID_ROWS - 1, (int)ceilf((y - F.min_y + r) * F.gh_inv));
  if (nMinCellX >= ORBFE_GRID_COLS || nMaxCellX < 0 || nMinCellY >= ORBFE_GRID_ROWS || nMaxCellY < 0) act = false;   // Frame.cc:347-366
  const bool bCheckLevels = (min_level > 0) || (max_level >= 0);
  const uint8_t* desc = F.desc + (size_t)f * F.cap * 32;
  const bool has_ur = F.u_right != nullptr;
  const int32_t* cs = F.cell_start + (size_t)f * (GRID_CELLS + 1);
  const uint4* cr = reinterpret_cast<const uint4*>(F.cell_rec) + (size_t)f * F.cap;
  orbfe_cand* out = cand + ((size_t)f * Q.cap + min(qi, Q.cap - 1)) * max_cand;
  const int ncol = act ? nMaxCellX - nMinCellX + 1 : 0;
  int total = 0;
  for (int cb = 0; __any(cb < ncol); cb += G) {
    int e0c = 0, cntc = 0;
    if (cb + sl < ncol) {
      const int ix = nMinCellX + cb + sl;
      e0c = cs[ix * ORBFE_GRID_ROWS + nMinCellY];
      cntc = cs[ix * ORBFE_GRID_ROWS + nMaxCellY + 1] - e0c;
    }
    static_assert(G == 16, "a group is one DPP row: the row shifts below never read a lane of another query");
    int inclc = cntc;   // inclusive scan inside the group (DPP row shifts; a shift from outside the row adds 0)
    { const int a = __builtin_amdgcn_update_dpp(0, inclc, 0x111, 0xf, 0xf, false); inclc += sl >= 1 ? a : 0; }
    { const int a = __builtin_amdgcn_update_dpp(0, inclc, 0x112, 0xf, 0xf, false); inclc += sl >= 2 ? a : 0; }
    { const int a = __builtin_amdgcn_update_dpp(0, inclc, 0x114, 0xf, 0xf, false); inclc += sl >= 4 ? a : 0; }
    { const int a = __builtin_amdgcn_update_dpp(0, inclc, 0x118, 0xf, 0xf, false); inclc += sl >= 8 ? a : 0; }
    const int exclc = inclc - cntc;
    const int n_entries = __shfl(inclc, gbase | (G - 1), WAVE);
    const int ncb = max(0, min(G, ncol - cb));             // columns of this batch (group-uniform)
    int ncb_max = ncb;                                     // wave-uniform loop bound
    ncb_max = max(ncb_max, __shfl_xor(ncb_max, 16, WAVE));
    ncb_max = max(ncb_max, __shfl_xor(ncb_max, 32, WAVE));
    ncb_max = __builtin_amdgcn_readfirstlane(ncb_max);
    for (int base = 0; __any(base < n_entries); base += G) {
      const int t = base + sl;
      int ent = -1;
      for (int c = 0; c < ncb_max; c++) {
        const int oc = __shfl(exclc, gbase | c, WAVE), nc = __shfl(cntc, gbase | c, WAVE), ec = __shfl(e0c, gbase | c, WAVE);
        if (c < ncb && t >= oc && t < oc + nc) ent = ec + (t - oc);
      }
      bool ok = false;
      int idx = 0, oct = 0;
      if (ent >= 0) {
        const CellRec k = cell_rec_unpack(cr[ent]);
        idx = k.idx;
        oct = k.oct;
        const float kx = k.x, ky = k.y, kur = k.ur;
        ok = true;
        if (bCheckLevels) {
          if (oct < min_level) ok = false;
          if (max_level >= 0 && oct > max_level) ok = false;
        }
        const float distx = kx - x, disty = ky - y;
        if (!(fabsf(distx) < r && fabsf(disty) < r)) ok = false;
        if (ok && has_ur && kur > 0) {           // the matcher's stereo gate
          const float er = fabsf(qur - kur);
          if (er > r) ok = false;
        }
      }
      const unsigned bits = (unsigned)((__ballot(ok) >> gbase) & ((1ull << G) - 1ull));
      if (ok) {
        uint4 d0, d1;
        load_desc(desc + (size_t)idx * 32, d0, d1);
        const int rank = total + __popc(bits & ((1u << sl) - 1u));
        if (rank < max_cand) { out[rank].idx = idx; out[rank].dist = hamming256(q0, q1, d0, d1) | (oct << 16); }
      }
      total += __popc(bits);
    }
  }
  if (sl == 0 && live) n_cand[(size_t)f * Q.cap + qi] = total;
}

// Order-dependent assignment of SearchByProjection.  One 1024-thread workgroup per frame.  Queries are taken
// up to RC_THREADS (1024) at a time, one per thread, and resolved by a fixed-point iteration against the blocked[] state the
// chunks before left: a thread's choice is its best candidate (mode 0: best and second-best) that no EARLIER thread of the chunk
// claims; claims are exchanged once per round, and the rounds converge to exactly the result of walking the queries one by one
// (L/src/ORBmatcher.cc:52-125, 1270-1361).  A query whose candidate list was truncated (> max_cand) ends the chunk and is
// handled alone by wave 0, which re-enumerates its window.
// mode 0: SearchByProjection(Frame&, vector<MapPoint*>&)   -- best/second with the same-level ratio test
// mode 1: SearchByProjection(Frame& cur, const Frame& last) -- best only, th_high = TH_HIGH, rotation histogram;
//         SearchByProjection(Frame&, KeyFrame*, set, th, ORBdist) is the same walk with th_high = ORBdist (:1385-1504)
#ifndef FC_TIMING
#define FC_TIMING 0
#endif
#if FC_TIMING
// -DFC_TIMING=1 (tools/search_latency.py): cycles of proj_resolve_kernel's workgroup 0 per phase (thread 0's clock after each barrier)
__device__ unsigned long long g_rs_prof[16];
extern "C" int orbfe_debug_rs_profile(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rs_prof), sizeof(unsigned long long) * 16) != hipSuccess) return 1;
  if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_rs_prof), z, sizeof(z)) != hipSuccess) return 1; }
  return 0;
}
#define RS_T(i) do { const unsigned long long _t = __builtin_readcyclecounter(); rs_acc##i += (unsigned)(_t - rs_prev); rs_prev = _t; } while (0)
#define RS_COUNT(i) do { rs_acc##i += 1; } while (0)
#define RS_END() do { if (blockIdx.x == 0 && threadIdx.x == 0) { unsigned a[11] = {rs_acc0, rs_acc1, rs_acc2, rs_acc3, rs_acc4, rs_acc5, rs_acc6, \
    rs_acc7, rs_acc8, rs_acc9, rs_acc10}; for (int _i = 0; _i < 11; _i++) g_rs_prof[_i] += a[_i]; } } while (0)
#else
#define RS_T(i)
#define RS_COUNT(i)
#define RS_END()
#endif
// best / second-best entry by distance, first one wins ties (the reference's strict "<"); RC_INVALID loses against everything.
// The pair is read into locals and written back with selects, no branches: with `if (...) e1 = e; else e2 = e;` on references (or a
// by-reference lambda) the compiler kept the pair in scratch memory and selected the ADDRESS to store to -- private-memory round
// trips inside the fixed-point loop (7 k cycles per round).
__device__ __forceinline__ void rc_take(uint32_t e, uint32_t& e1, uint32_t& e2) {
  const uint32_t a = e1, b = e2;
  const bool lt1 = (e >> 20) < (a >> 20), lt2 = (e >> 20) < (b >> 20);
  e2 = lt1 ? a : (lt2 ? e : b);
  e1 = lt1 ? e : a;
}
#define RC_THREADS 1024
#define RC_LIST_CAP 16384  // staged candidate entries per chunk (64 KiB): what does not fit the registers
#define RC_REG 4           // candidates per query kept in registers
#define RC_INVALID 0xFFFFFFFFu
#define RC_TAG_MAX 0x1fffff // claim words: (RC_TAG_MAX - round) << 10 | thread, 0x7fffffff = never claimed
__global__ __launch_bounds__(RC_THREADS) void proj_resolve_kernel(FrameBatch F, QueryBatch Q, const orbfe_cand* __restrict__ cand,
                                                           const int32_t* __restrict__ n_cand, int max_cand, int mode, int th_high,
                                                           float nnratio, int check_ori, uint8_t* __restrict__ blocked_all,
                                                           int32_t* __restrict__ assigned_all, int32_t* __restrict__ n_matches,
                                                           int32_t* __restrict__ push_idx_all, uint8_t* __restrict__ push_bin_all) {
  __shared__ int hist[ORBFE_HISTO_LENGTH];
  __shared__ uint32_t lc[RC_LIST_CAP];  // staged candidate lists: dist<<20 | octave<<16 | idx
  __shared__ int loff[RC_THREADS + 1];
  __shared__ int scan_tmp[RC_THREADS / WAVE];
  __shared__ int sh_len, sh_nm, sh_npush;
  __shared__ int sh_changed[2];
  extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
  const int capA = (F.cap + 15) & ~15;
  uint8_t* blocked = dyn;                                   // F.mvpMapPoints[idx]->Observations() > 0
  int* claim = reinterpret_cast<int*>(dyn + capA);          // smallest chunk thread that blocks idx this round
  int* claimB = claim + F.cap;                              // second claim buffer (the two alternate per iteration)
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid >> 6;
  const int nq = Q.n[f];
  uint8_t* blocked_g = blocked_all + (size_t)f * F.cap;
  int32_t* assigned = assigned_all + (size_t)f * F.cap;
  int32_t* push_idx = push_idx_all + (size_t)f * Q.cap;
  uint8_t* push_bin = push_bin_all + (size_t)f * Q.cap;
  const orbfe_keypoint* keys = F.keys + (size_t)f * F.cap;
  const orbfe_query* qbase = Q.q + (size_t)f * Q.cap;
  const int32_t* ncb = n_cand + (size_t)f * Q.cap;
  for (int i = tid; i < F.cap; i += RC_THREADS) { blocked[i] = blocked_g[i]; claim[i] = 0x7fffffff; claimB[i] = 0x7fffffff; }
  if (tid < ORBFE_HISTO_LENGTH) hist[tid] = 0;
  if (tid == 0) { sh_nm = 0; sh_npush = 0; }
#if FC_TIMING
  unsigned rs_acc0 = 0, rs_acc1 = 0, rs_acc2 = 0, rs_acc3 = 0, rs_acc4 = 0, rs_acc5 = 0, rs_acc6 = 0, rs_acc7 = 0, rs_acc8 = 0, rs_acc9 = 0,
           rs_acc10 = 0;
  unsigned long long rs_prev = __builtin_readcyclecounter();
#endif
  __syncthreads();
  RS_T(0);   // set-up
  const bool use_hist = (mode == 1) && check_ori;
  int q0 = 0;
  int round = 1;   // counts on across chunks: stamps the claims
  while (q0 < nq) {
    RS_COUNT(8);
    const int qi = q0 + tid;
    // one round trip: the query's flags, its candidate count and its first RC_REG candidates (slot rows exist for every qi < nq;
    // entries beyond the count are masked below)
    int tot = 0, qblocks = 0;
    float qangle = 0.f;
    uint2 craw[RC_REG];
#pragma unroll
    for (int u = 0; u < RC_REG; u++) craw[u] = make_uint2(0u, 0u);
    if (qi < nq) {
      const orbfe_query* qp = qbase + qi;
      const int qvalid = qp->valid;
      const int n = ncb[qi];
      qblocks = qp->blocks != 0;
      qangle = qp->angle;
      const uint2* row = reinterpret_cast<const uint2*>(cand + ((size_t)f * Q.cap + qi) * max_cand);
#pragma unroll
      for (int u = 0; u < RC_REG; u++) craw[u] = row[min(u, max_cand - 1)];
      tot = qvalid ? n : 0;
    }
    // chunk = queries q0 .. q0+len-1: stops before the first truncated list and before the staging area is full
    if (tid == 0) { sh_len = min(RC_THREADS, nq - q0); sh_changed[0] = 0; sh_changed[1] = 0; }
    __syncthreads();
    {
      const int v = tot > max_cand ? 0 : max(tot - RC_REG, 0);   // entries beyond the registers go through LDS
      const int w = wave_incl_scan_i(v);
      if (lane == WAVE - 1) scan_tmp[wid] = w;
      __syncthreads();
      int off = 0;
      for (int k = 0; k < wid; k++) off += scan_tmp[k];
      const int incl = off + w;
      loff[tid + 1] = incl;
      if (tid == 0) loff[0] = 0;
      if (tot > max_cand || incl > RC_LIST_CAP) atomicMin(&sh_len, tid);
    }
    __syncthreads();
    RS_T(1);   // query records + chunk scan
    const int len = sh_len;
    if (len == 0) {
      // ---- truncated list at q0: wave 0 re-enumerates this one window, the other waves wait
      if (wid == 0) {
        const orbfe_query* qp = qbase + q0;
        const orbfe_query q = *qp;
        uint4 d0, d1;
        load_desc4(qp->desc, d0, d1);
        unsigned k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;
        int i1 = -1, i2 = -1;
        enumerate_window(F, f, q, d0, d1, [&](int rank, int idx, int dist, int) {
          if (blocked[idx]) return;
          const unsigned key = ((unsigned)dist << 16) | (unsigned)min(rank, 0xffff);
          if (key < k1) { k2 = k1; i2 = i1; k1 = key; i1 = idx; }
          else if (key < k2) { k2 = key; i2 = idx; }
        });
        const unsigned b = wave_min_u32(k1);
        if (b != 0xFFFFFFFFu) {
          const int wl = first_min_lane(k1, b);
          const int bestIdx = __builtin_amdgcn_readlane(i1, wl);
          const int bestDist = (int)(b >> 16);
          bool accept = false;
          if (mode == 0) {
            const unsigned mine = (lane == wl) ? k2 : k1;   // second-best: the winning lane offers its second key
            const int mine_i = (lane == wl) ? i2 : i1;
            const unsigned s2 = wave_min_u32(mine);
            int bestDist2 = 256, bestLevel2 = -1;
            if (s2 != 0xFFFFFFFFu) {
              const int sl = first_min_lane(mine, s2);
              bestDist2 = (int)(s2 >> 16);
              bestLevel2 = keys[__shfl(mine_i, sl, WAVE)].octave;
            }
            const int bestLevel = keys[bestIdx].octave;
            if (bestDist <= th_high && !(bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2))
              accept = true;
          } else {
            accept = bestDist <= th_high;
          }
          if (accept && lane == 0) {
            assigned[bestIdx] = q0;
            blocked[bestIdx] = (uint8_t)(q.blocks != 0);
            sh_nm += 1;
            if (use_hist) {
              const int bin = rot_bin(q.angle, keys[bestIdx].angle);
              push_idx[sh_npush] = bestIdx;
              push_bin[sh_npush] = (uint8_t)bin;
              sh_npush += 1;
              hist[bin]++;
            }
          }
        }
      }
      __syncthreads();
      q0 += 1;
      continue;
    }
    // ---- the chunk's candidates, packed dist<<20 | octave<<16 | idx, COMPACTED in list order: an entry is dropped when its
    // keypoint is blocked (blocked[] only changes when a chunk commits, so that holds for every round below) or when its distance
    // cannot matter -- beyond th_high it is never accepted, and as a second-best (mode 0) it rejects the best one only while
    // nnratio * d < th_high.  What is left is the true match and a near miss or two: the first RC_REG entries stay in registers,
    // a longer list puts the rest in LDS (and its owner re-selects in every round).
    uint32_t creg[RC_REG];
#pragma unroll
    for (int u = 0; u < RC_REG; u++) creg[u] = RC_INVALID;
    int kept = 0, nover = 0;
    auto matters = [&](uint32_t d) {
      return d <= (uint32_t)th_high || (mode == 0 && d < 256u && nnratio * (float)d < (float)th_high);
    };
#pragma unroll
    for (int u = 0; u < RC_REG; u++) {
      const uint32_t idx = craw[u].x & 0xffffu, dd = craw[u].y;
      const uint32_t e = ((dd & 0xffffu) << 20) | (((dd >> 16) & 0xfu) << 16) | idx;
      const bool ok = tid < len && u < tot && matters(dd & 0xffffu) && !blocked[min(idx, (uint32_t)F.cap - 1u)];
#pragma unroll
      for (int j = 0; j <= u; j++) creg[j] = (ok && kept == j) ? e : creg[j];
      kept += ok;
    }
    {
      const int nraw = (tid < len) ? max(tot - RC_REG, 0) : 0;
      const uint2* row = reinterpret_cast<const uint2*>(cand + ((size_t)f * Q.cap + qi) * max_cand) + RC_REG;
      uint32_t* dstl = lc + loff[tid < len ? tid : 0];
      for (int c0 = 0; c0 < nraw; c0 += 4) {
        uint2 r[4];
#pragma unroll
        for (int u = 0; u < 4; u++) r[u] = row[min(c0 + u, nraw - 1)];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const uint32_t idx = r[u].x & 0xffffu, dd = r[u].y;
          if (c0 + u >= nraw || !matters(dd & 0xffffu) || blocked[idx]) continue;
          const uint32_t e = ((dd & 0xffffu) << 20) | (((dd >> 16) & 0xfu) << 16) | idx;
          if (kept < RC_REG) {
#pragma unroll
            for (int j = 0; j < RC_REG; j++) creg[j] = (kept == j) ? e : creg[j];
          } else {
            dstl[nover++] = e;
          }
          kept++;
        }
      }
    }
    __syncthreads();
    RS_T(2);   // staging
    const bool active = kept > 0;
    const uint32_t* mylist = lc + loff[tid < len ? tid : 0];
    // Fixed-point iteration over the chunk.  Thread t's choice = best candidate that is neither blocked nor
    // claimed (blocked-to-be) by an EARLIER thread of the chunk; claims come from the previous round.
    // Thread t's choice is final after at most t+1 rounds (it only depends on earlier threads), so the
    // iteration converges to exactly the sequential result; in practice the dependency chains are 2-5 deep.
    // One barrier per round: a claim is the word (RC_TAG_MAX - round) << 10 | thread, written by atomicMin into the buffer of
    // the round's parity and read back from the other buffer in the next round -- a newer round always wins the min, an older
    // word fails the tag test, so nothing is ever cleared (rounds count on across chunks; 2^21 of them fit).  The "somebody
    // changed" flag carries the round number the same way.  A barrier costs ~0.5 us with sixteen waves, a round hardly more.
    // state = the two best entries; RC_INVALID (distance field 0xfff) = none.  Plain 32-bit values only: bool flags updated
    // through a by-reference lambda ended up in scratch memory, several private-memory round trips per iteration (7 k cycles).
    uint32_t e1 = RC_INVALID, e2 = RC_INVALID;
    uint32_t pmask = ~0u;   // which of the register candidates an earlier query claimed, previous round
    int accept = 0;
    for (int iter = 0;; iter++, round++) {
      const int* cprev = (round & 1) ? claim : claimB;   // written in round - 1
      int* cnew = (round & 1) ? claimB : claim;
      const int want = (RC_TAG_MAX - (round - 1));       // tag of a claim made in the previous round
      bool changed = false;
      if (active) {
        int cl[RC_REG];
        uint32_t m = 0;
        if (iter > 0) {   // (the previous round of the first iteration belongs to the chunk before: no claims yet)
#pragma unroll
          for (int u = 0; u < RC_REG; u++) cl[u] = cprev[creg[u] == RC_INVALID ? 0 : (int)(creg[u] & 0xffffu)];
#pragma unroll
          for (int u = 0; u < RC_REG; u++)
            m |= (creg[u] != RC_INVALID && (cl[u] >> 10) == want && (cl[u] & (RC_THREADS - 1)) < tid) ? (1u << u) : 0u;
        }
        // The choice is a function of the claim pattern alone: same pattern, same choice.
        if (m != pmask || nover > 0) {
          pmask = m;
          const uint32_t pe1 = e1, pe2 = e2;
          e1 = e2 = RC_INVALID;
          accept = 0;
#pragma unroll
          for (int u = 0; u < RC_REG; u++) rc_take(((m >> u) & 1u) ? RC_INVALID : creg[u], e1, e2);
          for (int c0 = 0; c0 < nover; c0 += 4) {  // 4 candidates in flight: independent LDS loads first, then the scan
            uint32_t ev[4];
            int co[4];
#pragma unroll
            for (int u = 0; u < 4; u++) ev[u] = (c0 + u < nover) ? mylist[c0 + u] : RC_INVALID;
#pragma unroll
            for (int u = 0; u < 4; u++) co[u] = cprev[ev[u] == RC_INVALID ? 0 : (int)(ev[u] & 0xffffu)];
#pragma unroll
            for (int u = 0; u < 4; u++) {
              const bool taken = iter > 0 && (co[u] >> 10) == want && (co[u] & (RC_THREADS - 1)) < tid;
              rc_take(taken ? RC_INVALID : ev[u], e1, e2);
            }
          }
          if (e1 != RC_INVALID) {
            const int bestDist = (int)(e1 >> 20);
            if (mode == 0) {
              const int bestDist2 = e2 != RC_INVALID ? (int)(e2 >> 20) : 256;
              const int bestLevel = (int)((e1 >> 16) & 0xf), bestLevel2 = e2 != RC_INVALID ? (int)((e2 >> 16) & 0xf) : -1;
              accept = bestDist <= th_high && !(bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2);
            } else {
              accept = bestDist <= th_high;
            }
          }
          changed = e1 != pe1 || e2 != pe2;
        }
      }
      const int bestIdx = (int)(e1 & 0xffff);
      if (accept && qblocks) atomicMin(&cnew[bestIdx], ((RC_TAG_MAX - round) << 10) | tid);
      if (iter == 0 || changed) sh_changed[round & 1] = round;
      __syncthreads();
      RS_T(3);   // fixed-point rounds
      RS_COUNT(9);
      if (sh_changed[round & 1] == round) continue;
      // converged: commit every accepted query of the chunk.  Several queries may take the same keypoint
      // (only when the earlier ones do not block it): the last one in query order wins, as in the reference.
      round++;
      int* cw = (round & 1) ? claimB : claim;
      const int mine = ((RC_TAG_MAX - round) << 10) | (RC_THREADS - 1 - tid);
      if (active && accept) atomicMin(&cw[bestIdx], mine);
      __syncthreads();
      if (active && accept) {
        if (cw[bestIdx] == mine) {
          assigned[bestIdx] = qi;
          blocked[bestIdx] = (uint8_t)qblocks;
        }
        atomicAdd(&sh_nm, 1);
        if (use_hist) {
          const int bin = rot_bin(qangle, keys[bestIdx].angle);
          const int pos = atomicAdd(&sh_npush, 1);
          push_idx[pos] = bestIdx;
          push_bin[pos] = (uint8_t)bin;
          atomicAdd(&hist[bin], 1);
        }
      }
      round++;   // (no barrier here: the next chunk's first round writes the other buffer, and its set-up has barriers of its own)
      RS_T(4);   // commit
      break;
    }
    q0 += len;
  }
  __syncthreads();
  if (use_hist) {
    // rotation consistency (:1363-1379): every recorded match whose bin is not one of the three maxima is removed
    if (tid == 0) {
      int i1, i2, i3;
      three_maxima(hist, ORBFE_HISTO_LENGTH, i1, i2, i3);
      hist[0] = i1; hist[1] = i2; hist[2] = i3;  // the histogram itself is no longer needed
    }
    __syncthreads();
    const int i1 = hist[0], i2 = hist[1], i3 = hist[2];
    const int np = sh_npush;
    int removed = 0;
    for (int k = tid; k < np; k += RC_THREADS) {
      const int bin = push_bin[k];
      if (bin != i1 && bin != i2 && bin != i3) { assigned[push_idx[k]] = -1; blocked[push_idx[k]] = 0; removed++; }   // the slot is NULL again
    }
    if (removed) atomicSub(&sh_nm, removed);
  }
  __syncthreads();
  for (int i = tid; i < F.cap; i += RC_THREADS) blocked_g[i] = blocked[i];
  if (tid == 0) n_matches[f] = sh_nm;
  RS_T(5);   // rotation check + write-back
  RS_COUNT(10);
  RS_END();
}

// ------------------------------------------------------------------------------------------------ mono init
// ORBmatcher::SearchForInitialization (L/src/ORBmatcher.cc:388-492).  Every F1 keypoint may steal an F2 keypoint
// from an earlier one when it is strictly closer (vMatchedDistance / vnMatches21), so the queries are walked
// strictly in order by ONE wave; the lanes share each query's candidates (stored list, or the re-enumerated
// window when the list was truncated).  Runs a handful of times per session (map initialisation).
__global__ __launch_bounds__(64) void init_resolve_kernel(FrameBatch F, QueryBatch Q, const orbfe_cand* __restrict__ cand,
                                                           const int32_t* __restrict__ n_cand, int max_cand, float nnratio,
                                                           int check_ori, int32_t* __restrict__ matches12,
                                                           float* __restrict__ prev_xy, int32_t* __restrict__ n_matches,
                                                           int32_t* __restrict__ push_idx, uint8_t* __restrict__ push_bin) {
  __shared__ int hist[ORBFE_HISTO_LENGTH];
  extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
  int* matchedDist = reinterpret_cast<int*>(dyn);  // vMatchedDistance
  int* matches21 = matchedDist + F.cap;             // vnMatches21
  const int lane = threadIdx.x;
  const int n1 = Q.n[0], n2 = F.n[0];
  const orbfe_keypoint* keys2 = F.keys;
  for (int i = lane; i < n2; i += WAVE) { matchedDist[i] = 2147483647; matches21[i] = -1; }
  for (int i = lane; i < n1; i += WAVE) matches12[i] = -1;
  if (lane < ORBFE_HISTO_LENGTH) hist[lane] = 0;
  __syncthreads();
  int npush = 0;
  for (int i1 = 0; i1 < n1; i1++) {
    const orbfe_query* qp = Q.q + i1;
    if (!qp->valid) continue;  // level1 > 0
    const int total = n_cand[i1];
    if (total == 0) continue;
    unsigned k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;
    int i1b = -1;
    auto consider = [&](int rank, int idx, int dist, int = 0) {
      if (matchedDist[idx] <= dist) return;
      const unsigned key = ((unsigned)dist << 16) | (unsigned)min(rank, 0xffff);
      if (key < k1) { k2 = k1; k1 = key; i1b = idx; }
      else if (key < k2) { k2 = key; }
    };
    if (total <= max_cand) {
      const orbfe_cand* cl = cand + (size_t)i1 * max_cand;
      for (int c = lane; c < total; c += WAVE) consider(c, cl[c].idx, cl[c].dist & 0xffff, 0);
    } else {
      const orbfe_query q = *qp;
      uint4 d0, d1;
      load_desc4(qp->desc, d0, d1);
      enumerate_window(F, 0, q, d0, d1, consider);
    }
    const unsigned b = wave_min_u32(k1);
    if (b != 0xFFFFFFFFu) {
      const int wl = first_min_lane(k1, b);
      const int bestIdx2 = __builtin_amdgcn_readlane(i1b, wl);
      const int bestDist = (int)(b >> 16);
      const unsigned mine = (lane == wl) ? k2 : k1;   // second-best: the winning lane offers its second key
      const unsigned s2 = wave_min_u32(mine);
      const int bestDist2 = s2 != 0xFFFFFFFFu ? (int)(s2 >> 16) : 2147483647;
      if (bestDist <= ORBFE_TH_LOW && (float)bestDist < (float)bestDist2 * nnratio) {
        if (lane == 0) {
          const int prev = matches21[bestIdx2];
          if (prev >= 0) matches12[prev] = -1;
          matches12[i1] = bestIdx2;
          matches21[bestIdx2] = i1;
          matchedDist[bestIdx2] = bestDist;
          if (check_ori) {
            const int bin = rot_bin(qp->angle, keys2[bestIdx2].angle);
            push_idx[npush] = i1;
            push_bin[npush] = (uint8_t)bin;
            hist[bin]++;
          }
        }
        npush += check_ori ? 1 : 0;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  if (lane == 0) {
    if (check_ori) {
      int a, b2, c;
      three_maxima(hist, ORBFE_HISTO_LENGTH, a, b2, c);
      for (int k = 0; k < npush; k++) {
        const int bin = push_bin[k];
        if (bin != a && bin != b2 && bin != c) {
          const int idx1 = push_idx[k];
          if (matches12[idx1] >= 0) matches12[idx1] = -1;
        }
      }
    }
  }
  __syncthreads();
  int cnt = 0;
  for (int i = lane; i < n1; i += WAVE) {
    const int m = matches12[i];
    if (m >= 0) {
      cnt++;
      prev_xy[2 * i] = keys2[m].x;      // vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt (:487-489)
      prev_xy[2 * i + 1] = keys2[m].y;
    }
  }
  // the reference's nmatches (++ on assignment, -- on steal / rotation reject) == F1 keypoints still holding a match
  cnt = wave_sum_i32(cnt);
  if (lane == 0) n_matches[0] = cnt;
}

// ------------------------------------------------------------------------------------------------ launchers
void orbfe_launch_proj_best(const FrameBatch& f, const QueryBatch& q, int gate, const float* inv_sigma2, int32_t* best_idx,
                            int32_t* best_dist, int n_frames, hipStream_t s) {
  if (q.cap < 1) return;
  dim3 grid((q.cap + 3) / 4, n_frames);
  if (gate == 2) hipLaunchKernelGGL(proj_best_kernel<2>, grid, dim3(256), 0, s, f, q, inv_sigma2, best_idx, best_dist);
  else if (gate == 1) hipLaunchKernelGGL(proj_best_kernel<1>, grid, dim3(256), 0, s, f, q, inv_sigma2, best_idx, best_dist);
  else hipLaunchKernelGGL(proj_best_kernel<0>, grid, dim3(256), 0, s, f, q, inv_sigma2, best_idx, best_dist);
}
void orbfe_launch_proj_candidates(const FrameBatch& f, const QueryBatch& q, orbfe_cand* cand, int32_t* n_cand,
                                  int max_cand, int n_frames, hipStream_t s) {
  if (q.cap < 1) return;
  constexpr int QPB = 4 * (WAVE / ORBFE_CAND_LANES);   // queries per workgroup
  dim3 grid((q.cap + QPB - 1) / QPB, n_frames);
  hipLaunchKernelGGL(proj_candidates_kernel, grid, dim3(256), 0, s, f, q, cand, n_cand, max_cand);
}
void orbfe_launch_proj_resolve(const FrameBatch& f, const QueryBatch& q, const orbfe_cand* cand, const int32_t* n_cand,
                               int max_cand, int mode, int th_high, float nnratio, int check_ori, uint8_t* blocked,
                               int32_t* assigned, int32_t* n_matches, int32_t* push_idx, uint8_t* push_bin, int n_frames,
                               hipStream_t s) {
  const size_t dyn = (size_t)(((f.cap + 15) & ~15) + 8 * (size_t)f.cap);
  // this kernel's static LDS alone is ~69 KiB: the limit is raised once per device, whichever thread launches first
  static std::atomic<unsigned long long> raised{0};
  raise_dynamic_lds(reinterpret_cast<const void*>(proj_resolve_kernel), 88 * 1024, raised);
  hipLaunchKernelGGL(proj_resolve_kernel, dim3(n_frames), dim3(RC_THREADS), dyn, s, f, q, cand, n_cand, max_cand, mode, th_high,
                     nnratio, check_ori, blocked, assigned, n_matches, push_idx, push_bin);
}
void orbfe_launch_init_resolve(const FrameBatch& f, const QueryBatch& q, const orbfe_cand* cand, const int32_t* n_cand,
                               int max_cand, float nnratio, int check_ori, int32_t* matches12, float* prev_xy,
                               int32_t* n_matches, int32_t* push_idx, uint8_t* push_bin, hipStream_t s) {
  hipLaunchKernelGGL(init_resolve_kernel, dim3(1), dim3(64), (size_t)f.cap * 8, s, f, q, cand, n_cand, max_cand, nnratio,
                     check_ori, matches12, prev_xy, n_matches, push_idx, push_bin);
}
