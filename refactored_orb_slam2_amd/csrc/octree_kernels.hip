// octree_kernels.hip -- the keypoint selection stage of the ORB extractor for gfx950 (MI355X, wave64).
//
// octree_select     DistributeOctTree + DivideNode                       L/src/ORBextractor.cc:475-731
// (reference file:line, L/ = Source/Libraries/ORB_SLAM2/)
//
// All arithmetic that decides an output bit is integer, or float evaluated exactly as the x86-64 reference build does
// (no FMA contraction: this file is compiled with -ffp-contract=off; IEEE divide).
#include <string.h>

#include "orbfe_internal.h"
#include "extract_device.h"

// ------------------------------------------------------------------------------------------------ octree
// DistributeOctTree as an array algorithm.  The leaves of the quadtree are kept in an array in std::list
// order (index 0 = list head); because every insertion in the reference is a push_front and the initial
// nodes are push_back'ed, list order == descending creation order, so "sort by (size, node address)" with
// a bump allocator == sort by (size, -position).  One iteration = count keys per (leaf, quadrant), prefix
// sums over leaves, rebuild the array, relabel keys.  Keys never move.
//
// key record (8 bytes): x:int16 | y:int16 | node:uint16 | score:uint8 | quadrant:uint8
__device__ __forceinline__ unsigned long long key_pack(int x, int y, int node, int score, int q) {
  return (unsigned long long)(uint16_t)x | ((unsigned long long)(uint16_t)y << 16) |
         ((unsigned long long)(uint16_t)node << 32) | ((unsigned long long)(uint8_t)score << 48) |
         ((unsigned long long)(uint8_t)q << 56);
}
#define KEY_X(k) ((int)(int16_t)((k) & 0xffff))
#define KEY_Y(k) ((int)(int16_t)(((k) >> 16) & 0xffff))
#define KEY_NODE(k) ((int)(((k) >> 32) & 0xffff))
#define KEY_SCORE(k) ((int)(((k) >> 48) & 0xff))
#define KEY_Q(k) ((int)(((k) >> 56) & 0xff))

struct OctNode {
  int16_t x0, x1, y0, y1;
  int32_t cnt;
};

size_t orbfe_octree_lds_bytes(int M, int lds_keys) {
  // nodeA, nodeB (12 B), cnt4 (16 B), childpos (8 B: 4 x uint16), aux (4 B), aux2 (4 B); the phase-2 sort buffers
  // alias childpos (sort keys) and nodeB (sorted keys), which are dead while the sort runs
  return (size_t)M * (12 + 12 + 16 + 8 + 4 + 4) + (size_t)lds_keys * 8 + 64 * 4 + ORBFE_MAX_INI * 8 + 256;
}

#if FC_TIMING
__device__ unsigned long long g_oct_prof[256];   // [level] cycles, [32 + level] iterations of the subdivision loop, [64 + 8 level + phase] cycles
extern "C" int orbfe_debug_oct_profile(unsigned long long* out, int reset) {   // out: 256 entries
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_oct_prof), sizeof(unsigned long long) * 256) != hipSuccess) return 1;
  if (reset) { unsigned long long z[256]; memset(z, 0, sizeof(z)); if (hipMemcpyToSymbol(HIP_SYMBOL(g_oct_prof), z, sizeof(z)) != hipSuccess) return 1; }
  return 0;
}
// phases (tools/oct_phase_profile.py): 0 cell offsets, 1 key gather, 2 first relabel / histogram, 3 node work of the subdivision
// rounds, 4 their key sweeps, 5 best key + output
#define OCT_TP(i) do { const unsigned long long _t = __builtin_readcyclecounter(); tph[i] += _t - t_prev; t_prev = _t; } while (0)
#else
#define OCT_TP(i)
#endif
#define OCT_T ORBFE_OCT_THREADS   // 256 measured best (64: 0.120, 128: 0.091, 256: 0.069, 512: 0.091 ms per 256 images)
static_assert(ORBFE_MAX_INI <= ORBFE_OCT_THREADS, "one thread per root node in step 3");
__global__ __launch_bounds__(ORBFE_OCT_THREADS) void octree_select_kernel(OctParams P) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x;
  // grid = (images, levels): workgroups start level-major, the long ones (level 0: ~120 k cycles, level 7: ~45 k) first, so the
  // tail of the launch is made of short workgroups (image-major order ran as two rounds of the longest one: 110 -> 80 us)
  const int level = blockIdx.y, img = blockIdx.x;
#if FC_TIMING
  const unsigned long long t_begin = __builtin_readcyclecounter();
  unsigned long long t_prev = t_begin, tph[6] = {0, 0, 0, 0, 0, 0};
  int n_iter = 0;
#endif
  const OctLevel L = P.lv[level];
  const int M = P.max_nodes;

  // carve dynamic LDS
  uint8_t* sp = smem;
  unsigned long long* lkeys = reinterpret_cast<unsigned long long*>(sp);   sp += (size_t)P.lds_keys * 8;
  uint16_t* childpos = reinterpret_cast<uint16_t*>(sp); sp += (size_t)M * 8;
  OctNode* nodeA = reinterpret_cast<OctNode*>(sp); sp += (size_t)M * 12;   // M is a multiple of 64: 8-byte aligned
  OctNode* nodeB = reinterpret_cast<OctNode*>(sp); sp += (size_t)M * 12;
  int* cnt4 = reinterpret_cast<int*>(sp);          sp += (size_t)M * 16;
  int* aux = reinterpret_cast<int*>(sp);           sp += (size_t)M * 4;   // childbase / flags
  int* aux2 = reinterpret_cast<int*>(sp);          sp += (size_t)M * 4;   // staypos
  int* ini_cnt = reinterpret_cast<int*>(sp);       sp += ORBFE_MAX_INI * 4;
  int* ini_map = reinterpret_cast<int*>(sp);       sp += ORBFE_MAX_INI * 4;
  int* scan_tmp = reinterpret_cast<int*>(sp);      sp += 16 * 4;
  int* sh = reinterpret_cast<int*>(sp);            // small shared scalars

  const int32_t* cnt = P.cell_cnt + (size_t)img * P.total_cells + L.cell_begin;
  int32_t* coff = P.cell_off + (size_t)img * P.total_cells + L.cell_begin;
  const CellDesc* cells = P.cells + L.cell_begin;
  const uint32_t* slots = P.slots + (size_t)img * P.slots_per_image;
  uint32_t* out_kp = P.lvl_kp + (size_t)img * P.kp_per_image + L.kp_off;

  // 1. exclusive offsets of the cells' candidate lists (cell raster order == vToDistributeKeys order).  Offset, count and slot
  //    address of every cell go to LDS (the quadrant-count array, idle until step 3) when the level's cells fit: the gather below
  //    then has the candidates themselves as its only memory requests
  const int tab_cap = (M * 4) / 3;
  const bool use_tab = L.n_cells <= tab_cap;
  int* tb_o = cnt4;
  int* tb_n = cnt4 + tab_cap;
  uint32_t* tb_so = reinterpret_cast<uint32_t*>(cnt4 + 2 * tab_cap);
  int running = 0;
  for (int base = 0; base < L.n_cells; base += OCT_T) {
    const int c = base + tid;
    const int v = c < L.n_cells ? cnt[c] : 0;
    const uint32_t so = c < L.n_cells ? cells[c].slot_off : 0u;
    int tot;
    const int incl = block_incl_scan_t<OCT_T>(v, scan_tmp, &tot);
    if (c < L.n_cells) {
      if (use_tab) { tb_o[c] = running + incl - v; tb_n[c] = v; tb_so[c] = so; }
      else coff[c] = running + incl - v;
    }
    running += tot;
  }
  const int C = running;
  OCT_TP(0);
  if (C > L.key_cap || C > 0xFFFFFF) {  // cannot happen: key_cap = sum of slot caps
    if (tid == 0) { atomicOr(P.err, 1); P.lvl_n[(size_t)img * ORBFE_MAX_LEVELS + level] = 0; }
    return;
  }
  unsigned long long* keys = (C <= P.lds_keys) ? lkeys : (P.gkeys + (size_t)img * P.gkeys_per_image + L.key_off);

  for (int i = tid; i < L.n_ini; i += OCT_T) ini_cnt[i] = 0;
  __syncthreads();

  // 2. gather keys, assign to the root nodes: vpIniNodes[kp.pt.x / hX] (L/src/ORBextractor.cc:559)
  auto put_key = [&](uint32_t e, int at) {
    const int x = e & 0xfff, y = (e >> 12) & 0xfff, s = e >> 24;
    int node = (int)((float)x / L.hX);
    if (node >= L.n_ini) node = L.n_ini - 1;
    keys[at] = key_pack(x, y, node, s, 0);
    atomicAdd(&ini_cnt[node], 1);
  };
  if (use_tab) {
    // G lanes per cell, G = the power of two at or above the mean list length (1 .. 64): few candidates per cell -> many cells per
    // pass; dense texture -> a wave per cell, coalesced reads and writes.  Two cells x four candidates per lane are requested
    // together (thread per cell with one request at a time was a chain of round trips: a quarter of the level-0 workgroup's time,
    // a third with dense texture)
    int gs = 0;
    while (gs < 6 && ((L.n_cells << gs) < C)) gs++;
    const int G = 1 << gs, NG = OCT_T >> gs;
    const int g = tid >> gs, jl = tid & (G - 1);
    for (int c0 = g; c0 < L.n_cells; c0 += 2 * NG) {
      const int c1 = c0 + NG;
      const bool h1 = c1 < L.n_cells;
      const int nA = tb_n[c0], oA = tb_o[c0], nB = h1 ? tb_n[c1] : 0, oB = h1 ? tb_o[c1] : 0;
      const uint32_t* sA = slots + tb_so[c0];
      const uint32_t* sB = slots + (h1 ? tb_so[c1] : 0u);
      for (int j0 = jl; j0 < max(nA, nB); j0 += 4 * G) {
        uint32_t eA[4], eB[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          eA[u] = j0 + u * G < nA ? sA[j0 + u * G] : 0u;
          eB[u] = j0 + u * G < nB ? sB[j0 + u * G] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          if (j0 + u * G < nA) put_key(eA[u], oA + j0 + u * G);
          if (j0 + u * G < nB) put_key(eB[u], oB + j0 + u * G);
        }
      }
    }
  } else {
    for (int c = tid; c < L.n_cells; c += OCT_T) {   // more cells than the table holds (very large images): thread per cell
      const int n = cnt[c];
      const int o = coff[c];
      const uint32_t* src = slots + cells[c].slot_off;
      for (int j = 0; j < n; j++) put_key(src[j], o + j);
    }
  }
  __syncthreads();
  OCT_TP(1);

  // 3. root nodes that hold keys, in order (empty ones are erased, :564-572)
  int size;
  {
    const int has = (tid < L.n_ini && ini_cnt[tid] > 0) ? 1 : 0;
    int tot;
    const int incl = block_incl_scan_t<OCT_T>(has, scan_tmp, &tot);
    if (tid < L.n_ini) {
      ini_map[tid] = incl - has;
      if (has) {
        OctNode nd;
        nd.x0 = (int16_t)(int)(L.hX * (float)tid);
        nd.x1 = (int16_t)(int)(L.hX * (float)(tid + 1));
        nd.y0 = 0;
        nd.y1 = (int16_t)L.height;
        nd.cnt = ini_cnt[tid];
        nodeA[incl - 1] = nd;
      }
    }
    size = tot;
  }
  for (int i = tid; i < size * 4; i += OCT_T) cnt4[i] = 0;
  __syncthreads();
  // A key's new leaf and, in the same visit, the quadrant of that leaf it falls into with the leaf's quadrant count (DivideNode
  // :505-517) for the NEXT subdivision round: one read and one write of every key per round instead of two passes (a count
  // pass and a relabel pass).  Four keys per thread are requested together (the spill path reads them from HBM: one round trip
  // per key otherwise).
  auto relabel_and_count = [&](const OctNode* nodes, auto&& new_leaf) {
    for (int k0 = tid; k0 < C; k0 += 4 * OCT_T) {
      unsigned long long kk[4];
#pragma unroll
      for (int j = 0; j < 4; j++) kk[j] = keys[min(k0 + j * OCT_T, C - 1)];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int k = k0 + j * OCT_T;
        if (k >= C) break;
        const int np = new_leaf(kk[j]);
        const OctNode nd = nodes[np];
        int q = 0;
        if (nd.cnt > 1) {
          const int mx = nd.x0 + ((nd.x1 - nd.x0 + 1) >> 1);  // UL.x + ceil(w/2)
          const int my = nd.y0 + ((nd.y1 - nd.y0 + 1) >> 1);
          q = (KEY_X(kk[j]) >= mx ? 1 : 0) + (KEY_Y(kk[j]) >= my ? 2 : 0);  // 0:n1 1:n2 2:n3 3:n4
          atomicAdd(&cnt4[np * 4 + q], 1);
        }
        keys[k] = (kk[j] & 0x00ff0000ffffffffULL) | ((unsigned long long)(uint16_t)np << 32) | ((unsigned long long)q << 56);
      }
    }
  };
  // ---- fast-forward for levels whose keys live in HBM (dense texture).  Where a node is cut depends on the node alone, so a key's
  // path through the first D = L.ff_depth subdivisions is a function of its position: ONE sweep counts the keys per depth-D cell,
  // sums of four give the counts of every shallower node, and the subdivision rounds below take a new leaf's quadrant counts from
  // those tables instead of sweeping the keys (a sweep = 16 bytes per key through the fabric for all workgroups at once: the four
  // rounds of uniform noise were 630 k of the level-0 workgroup's 1.4 M cycles).  Keys keep their ROOT index meanwhile; the first
  // round that creates a multi-key leaf at depth D writes real labels (`materialise`) and the explicit rounds take over.
  // Tables T_1 .. T_D (T_d: n_ini * 4^d counts, index = 4 * parent index + quadrant), the cell -> leaf map and the leaves'
  // (depth, index) words live in the LDS key array, which is idle exactly when the keys are in HBM.
  const int FD = (keys != lkeys) ? L.ff_depth : 0;
  bool ff = FD > 0;
  int* ffT = reinterpret_cast<int*>(lkeys);                         // T_d starts at n_ini * (4^d - 4) / 3
  const int ff_nT = L.n_ini * (((1 << (2 * FD + 2)) - 4) / 3);
  uint16_t* f2l = reinterpret_cast<uint16_t*>(ffT + ff_nT);         // depth-D cell -> leaf
  const int ff_nF = L.n_ini << (2 * FD);
  uint16_t* infoA = f2l + ((ff_nF + 1) & ~1);                       // leaf -> depth << 12 | index at that depth
  uint16_t* infoB = infoA + M;
  auto ff_tab = [&](int d) { return ffT + L.n_ini * (((1 << (2 * d)) - 4) / 3); };
  auto ff_cell = [&](unsigned long long kk) {   // index of the key's depth-D cell (KEY_NODE = root index)
    const int r = KEY_NODE(kk), x = KEY_X(kk), y = KEY_Y(kk);
    int x0 = (int16_t)(int)(L.hX * (float)r), x1 = (int16_t)(int)(L.hX * (float)(r + 1)), y0 = 0, y1 = (int16_t)L.height;
    int idx = r;
    for (int d = 0; d < FD; d++) {
      const int mx = x0 + ((x1 - x0 + 1) >> 1), my = y0 + ((y1 - y0 + 1) >> 1);
      const int qx = x >= mx ? 1 : 0, qy = y >= my ? 1 : 0;
      if (qx) x0 = mx; else x1 = mx;
      if (qy) y0 = my; else y1 = my;
      idx = idx * 4 + qx + 2 * qy;
    }
    return idx;
  };
  auto ff_fill_f2l = [&](const uint16_t* info, int n) {   // every leaf marks the depth-D cells it covers
    for (int p = tid; p < n; p += OCT_T) {
      const int d = info[p] >> 12, sh = 2 * (FD - d);
      const int first = (int)(info[p] & 0xfffu) << sh;
      for (int i = 0; i < (1 << sh); i++) f2l[first + i] = (uint16_t)p;
    }
  };
  auto ff_counts = [&](const OctNode* nodes, const uint16_t* info, int n) {   // quadrant counts of the multi-key leaves from the tables
    for (int i = tid; i < n * 4; i += OCT_T) {
      const int p = i >> 2;
      if (nodes[p].cnt > 1) cnt4[i] = ff_tab((info[p] >> 12) + 1)[4 * (int)(info[p] & 0xfffu) + (i & 3)];
    }
  };
  if (ff) {
    for (int i = tid; i < ff_nT; i += OCT_T) ffT[i] = 0;
    __syncthreads();
    int* TD = ff_tab(FD);
    for (int k0 = tid; k0 < C; k0 += 8 * OCT_T) {
      unsigned long long kk[8];
#pragma unroll
      for (int j = 0; j < 8; j++) kk[j] = keys[min(k0 + j * OCT_T, C - 1)];
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (k0 + j * OCT_T < C) atomicAdd(&TD[ff_cell(kk[j])], 1);
    }
    __syncthreads();
    for (int d = FD - 1; d >= 1; d--) {
      int* Td = ff_tab(d);
      const int* Tc = ff_tab(d + 1);
      for (int i = tid; i < (L.n_ini << (2 * d)); i += OCT_T) Td[i] = Tc[4 * i] + Tc[4 * i + 1] + Tc[4 * i + 2] + Tc[4 * i + 3];
      __syncthreads();
    }
    if (tid < L.n_ini && ini_cnt[tid] > 0) infoA[ini_map[tid]] = (uint16_t)tid;   // depth 0
    __syncthreads();
    ff_counts(nodeA, infoA, size);
  } else {
    relabel_and_count(nodeA, [&](unsigned long long kk) { return ini_map[KEY_NODE(kk)]; });
  }
  __syncthreads();
  OCT_TP(2);

  // 4. subdivision loop (:581-709)
  int phase = 1;
  int scan_slot = 0;
  bool finish = (size == 0);
  const int N = L.N;
  while (!finish) {
#if FC_TIMING
    n_iter++;
#endif
    const int prev = size;   // cnt4 holds the quadrant counts of every multi-key leaf of nodeA (relabel_and_count)

    // which leaves split, and in which order their children are created.  (The rounds are a chain of barriers -- ~10 k of a
    // workgroup's ~20 k cycles per round whatever the level holds -- so phase 1 takes one packed scan for the children's and the
    // staying leaves' positions, counts the next round's expandable leaves while it builds them, and every thread reads only
    // entries it wrote itself until the barrier behind the build.)
    int K = 0;        // number of children created
    int S = 0;        // leaves that stay
    int nsplit = 0;
    if (tid == 0) { sh[2] = 0; sh[3] = 0; }   // multi-key children created this round (nToExpand) / a leaf below the tables; set behind a barrier
    if (phase == 1) {
      // every multi-key leaf splits, in list order (:592-643)
      int run_c = 0, run_s = 0;
      for (int base = 0; base < size; base += OCT_T) {
        const int p = base + tid;
        int c = 0;
        if (p < size && nodeA[p].cnt > 1)
          c = (cnt4[p * 4] > 0) + (cnt4[p * 4 + 1] > 0) + (cnt4[p * 4 + 2] > 0) + (cnt4[p * 4 + 3] > 0);
        const int st = (p < size && c == 0) ? 1 : 0;   // a multi-key leaf has a non-empty quadrant
        int tot;
        const int incl = block_incl_scan_alt<OCT_T>(c | (st << 16), scan_tmp + 8, scan_slot, &tot);
        if (p < size) {
          aux[p] = c > 0 ? run_c + (incl & 0xffff) - c : -1;  // childbase, -1 = stays
          if (st) aux2[p] = run_s + (incl >> 16) - 1;          // rank among the leaves that stay
        }
        run_c += tot & 0xffff;
        run_s += tot >> 16;
      }
      K = run_c;
      S = run_s;
      for (int p = tid; p < size; p += OCT_T)
        if (aux[p] < 0) aux2[p] += K;   // after the K new children, old order preserved
    } else {
      // phase 2 (:651-707): expandable leaves sorted by (size, address) ascending, walked from the back:
      // larger first, among equal sizes the later-created (= smaller list position) first; stop as soon as
      // the list holds >= N nodes.
      unsigned long long* sortkey = reinterpret_cast<unsigned long long*>(childpos);  // dead until the rebuild below
      unsigned long long* sorted = reinterpret_cast<unsigned long long*>(nodeB);      // previous generation: dead
      int nE = 0;
      for (int base = 0; base < size; base += OCT_T) {
        const int p = base + tid;
        const int e = (p < size && nodeA[p].cnt > 1) ? 1 : 0;
        int tot;
        const int incl = block_incl_scan_t<OCT_T>(e, scan_tmp, &tot);
        if (e) sortkey[nE + incl - 1] = ((unsigned long long)(0xFFFFFFFFu - (uint32_t)nodeA[p].cnt) << 32) | (uint32_t)p;
        if (p < size) aux[p] = -1;
        nE += tot;
      }
      __syncthreads();
      // rank sort (keys are unique)
      for (int i = tid; i < nE; i += OCT_T) {
        const unsigned long long mine = sortkey[i];
        int r = 0;
        for (int j = 0; j < nE; j++) r += (sortkey[j] < mine) ? 1 : 0;
        sorted[r] = mine;
      }
      __syncthreads();
      // walk in sorted order: running list size after each split; first rank reaching N ends the walk
      if (tid == 0) sh[0] = nE;  // index of the last split rank + 1
      int run_inc = 0, run_c = 0;
      for (int base = 0; base < nE; base += OCT_T) {
        const int r = base + tid;
        int c = 0, p = 0;
        if (r < nE) {
          p = (int)(sorted[r] & 0xffffffffu);
          c = (cnt4[p * 4] > 0) + (cnt4[p * 4 + 1] > 0) + (cnt4[p * 4 + 2] > 0) + (cnt4[p * 4 + 3] > 0);
        }
        int tot;
        const int packed = ((c > 0 ? c - 1 : 0) << 16) | c;
        const int incl = block_incl_scan_t<OCT_T>(packed, scan_tmp, &tot);
        if (r < nE) {
          const int size_after = prev + run_inc + (incl >> 16);
          aux2[r] = run_c + (incl & 0xffff) - c;  // childbase by rank (temporarily in aux2)
          if (size_after >= N) atomicMin(&sh[0], r + 1);
        }
        run_inc += tot >> 16;
        run_c += tot & 0xffff;
        __syncthreads();
      }
      __syncthreads();
      nsplit = sh[0];
      __syncthreads();
      if (tid == 0) sh[1] = 0;
      __syncthreads();
      for (int r = tid; r < nsplit; r += OCT_T) {
        const int p = (int)(sorted[r] & 0xffffffffu);
        aux[p] = aux2[r];
        if (r == nsplit - 1) {
          const int c = (cnt4[p * 4] > 0) + (cnt4[p * 4 + 1] > 0) + (cnt4[p * 4 + 2] > 0) + (cnt4[p * 4 + 3] > 0);
          sh[1] = aux2[r] + c;
        }
      }
      __syncthreads();
      K = sh[1];
      __syncthreads();
      // positions of the leaves that stay: after the K new children, old order preserved
      for (int base = 0; base < size; base += OCT_T) {
        const int p = base + tid;
        const int st = (p < size && aux[p] < 0) ? 1 : 0;
        int tot;
        const int incl = block_incl_scan_t<OCT_T>(st, scan_tmp, &tot);
        if (st) aux2[p] = K + S + incl - 1;
        S += tot;
      }
    }
    const int newsize = K + S;
    if (newsize > M) {  // cannot happen: M >= max(N + 3, 4 * nIni)
      if (tid == 0) { atomicOr(P.err, 2); P.lvl_n[(size_t)img * ORBFE_MAX_LEVELS + level] = 0; }
      return;
    }
    // build the new leaf array: children pushed to the front in creation order => reversed
    int n_multi = 0;
    for (int p = tid; p < size; p += OCT_T) {
      const OctNode nd = nodeA[p];
      if (aux[p] >= 0) {
        const int mx = nd.x0 + ((nd.x1 - nd.x0 + 1) >> 1);
        const int my = nd.y0 + ((nd.y1 - nd.y0 + 1) >> 1);
        int j = aux[p];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int cq = cnt4[p * 4 + q];
          if (cq > 0) {
            OctNode ch;
            ch.x0 = (q & 1) ? (int16_t)mx : nd.x0;
            ch.x1 = (q & 1) ? nd.x1 : (int16_t)mx;
            ch.y0 = (q & 2) ? (int16_t)my : nd.y0;
            ch.y1 = (q & 2) ? nd.y1 : (int16_t)my;
            ch.cnt = cq;
            const int pos = K - 1 - j;
            nodeB[pos] = ch;
            childpos[p * 4 + q] = (uint16_t)pos;
            if (ff) infoB[pos] = (uint16_t)((((infoA[p] >> 12) + 1) << 12) | ((infoA[p] & 0xfffu) * 4 + q));
            n_multi += cq > 1 ? 1 : 0;
            j++;
          }
        }
      } else {
        nodeB[aux2[p]] = nd;
        if (ff) infoB[aux2[p]] = infoA[p];
      }
    }
    {   // one add per wave: 256 adds to one LDS word are 256 passes through an LDS pipeline that four workgroups share
      const int wsum = wave_incl_scan(n_multi);
      if ((tid & (WAVE - 1)) == WAVE - 1 && wsum) atomicAdd(&sh[2], wsum);
    }
    __syncthreads();
    const int n_expand = sh[2];   // read here: thread 0 clears it again at the top of the next round, two barriers on
    for (int i = tid; i < newsize * 4; i += OCT_T) cnt4[i] = 0;   // the build above was the last reader of this round's counts
    if (ff) {   // a multi-key leaf at depth D: its quadrant counts are not in the tables
      const bool last = newsize >= N || newsize == prev;   // the loop ends below: nobody reads the next round's counts
      // (no __syncthreads_or: it brings 256 bytes of static LDS, and the fourth workgroup no longer fits the compute unit)
      for (int p = tid; p < newsize; p += OCT_T)
        if (nodeB[p].cnt > 1 && (infoB[p] >> 12) >= FD) sh[3] = 1;
      __syncthreads();
      const int deep = sh[3];
      OCT_TP(3);
      if (last) {
      } else if (!deep) {
        ff_counts(nodeB, infoB, newsize);
      } else {
        ff_fill_f2l(infoB, newsize);
        __syncthreads();
        relabel_and_count(nodeB, [&](unsigned long long kk) { return (int)f2l[ff_cell(kk)]; });   // labels from here on
        ff = false;
      }
      { uint16_t* t = infoA; infoA = infoB; infoB = t; }
    } else {
      __syncthreads();
      OCT_TP(3);
      relabel_and_count(nodeB, [&](unsigned long long kk) {
        const int p = KEY_NODE(kk);
        return aux[p] >= 0 ? (int)childpos[p * 4 + KEY_Q(kk)] : aux2[p];
      });
    }
    { OctNode* t = nodeA; nodeA = nodeB; nodeB = t; }
    size = newsize;
    __syncthreads();
    OCT_TP(4);

    // nToExpand = leaves with more than one key: in phase 1 all of them are this round's children (:645-649)
    if (size >= N || size == prev) finish = true;
    else if (phase == 1 && size + 3 * n_expand > N) phase = 2;
  }

  OCT_TP(3);
  // 5. best key of every leaf: max response, first candidate wins ties (:712-728)
  uint32_t* best = reinterpret_cast<uint32_t*>(cnt4);
  for (int p = tid; p < size; p += OCT_T) best[p] = 0;
  __syncthreads();
  if (ff) {   // the tree was finished inside the tables: the keys never got labels, a key's leaf is its cell's
    ff_fill_f2l(infoA, size);
    __syncthreads();
    for (int k0 = tid; k0 < C; k0 += 8 * OCT_T) {
      unsigned long long kk[8];
#pragma unroll
      for (int j = 0; j < 8; j++) kk[j] = keys[min(k0 + j * OCT_T, C - 1)];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int k = k0 + j * OCT_T;
        if (k < C) atomicMax(&best[f2l[ff_cell(kk[j])]], ((uint32_t)KEY_SCORE(kk[j]) << 24) | (0xFFFFFFu - (uint32_t)k));
      }
    }
  } else {
    for (int k = tid; k < C; k += OCT_T) {
      const unsigned long long kk = keys[k];
      atomicMax(&best[KEY_NODE(kk)], ((uint32_t)KEY_SCORE(kk) << 24) | (0xFFFFFFu - (uint32_t)k));
    }
  }
  __syncthreads();
  for (int p = tid; p < size; p += OCT_T) {
    const int k = (int)(0xFFFFFFu - (best[p] & 0xFFFFFFu));
    const unsigned long long kk = keys[k];
    if (p < L.kp_cap)
      out_kp[p] = (uint32_t)KEY_X(kk) | ((uint32_t)KEY_Y(kk) << 12) | ((uint32_t)KEY_SCORE(kk) << 24);
  }
  if (tid == 0) {
    if (size > L.kp_cap) atomicOr(P.err, 4);
    P.lvl_n[(size_t)img * ORBFE_MAX_LEVELS + level] = size < L.kp_cap ? size : L.kp_cap;
#if FC_TIMING
    atomicAdd(&g_oct_prof[level], __builtin_readcyclecounter() - t_begin);
    atomicAdd(&g_oct_prof[32 + level], (unsigned long long)n_iter);
    OCT_TP(5);
    for (int i = 0; i < 6; i++) atomicAdd(&g_oct_prof[64 + 8 * level + i], tph[i]);
#endif
  }
}

// ------------------------------------------------------------------------------------------------ launchers
void orbfe_launch_octree(const OctParams& p, int n_images, size_t lds_bytes, hipStream_t s) {
  dim3 block(ORBFE_OCT_THREADS), grid(n_images, p.n_levels);
  hipLaunchKernelGGL(octree_select_kernel, grid, block, lds_bytes, s, p);
}

int orbfe_set_octree_lds(size_t lds_bytes) {
  return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(octree_select_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}
