// fast_kernels.hip -- the FAST stage of the ORB extractor for gfx950 (MI355X, wave64).
//
// fast_cells        per-cell cv::FAST(th=ini, else th=min) + NMS         L/src/ORBextractor.cc:756-791
// (reference file:line, L/ = Source/Libraries/ORB_SLAM2/)
//
// All arithmetic that decides an output bit is integer.
#include <string.h>

#include "orbfe_internal.h"
#include "extract_device.h"

// ------------------------------------------------------------------------------------------------ FAST
// ring offsets of FAST-9/16 (OpenCV makeOffsets, patternSize 16)
__device__ constexpr int RDX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
__device__ constexpr int RDY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};

// packed (2 x u16) min / max
__device__ __forceinline__ uint32_t pkmin(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t pkmax(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// packed (2 x i16) helpers of the pair-wise corner score below
__device__ __forceinline__ uint32_t pkmin_i(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_min_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t pkmax_i(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t pksub_i(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_sub_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// max over the sixteen 9-arcs of the arc minimum of t[k] = (v - q_k) ^ m, with the ring held as eight (q_2j, q_2j+1) pairs.
// m = 0: the dark score + 1 of cornerScore<16>.  m = ~0: t = q - v - 1 (bitwise NOT reverses the order), so the result is the
// bright score + 1, minus 1.  One network serves either polarity without a divergent branch around it.
__device__ __forceinline__ int arc9_maxmin_pk(const uint32_t (&P)[8], uint32_t VV, uint32_t m) {
  uint32_t D[8], L[8];
#pragma unroll
  for (int j = 0; j < 8; j++) D[j] = pksub_i(VV, P[j]) ^ m;
#pragma unroll
  for (int j = 0; j < 8; j++) L[j] = pkmin_i(D[j], __builtin_amdgcn_alignbit(D[(j + 1) & 7], D[j], 16));   // min d[i .. i+1]
  uint32_t L4[8];
#pragma unroll
  for (int j = 0; j < 8; j++) L4[j] = pkmin_i(L[j], L[(j + 1) & 7]);                                       // min d[i .. i+3]
#pragma unroll
  for (int j = 0; j < 8; j++) L[j] = pkmin_i(pkmin_i(L4[j], L4[(j + 2) & 7]), D[(j + 4) & 7]);             // min d[i .. i+8]
  const uint32_t A = pkmax_i(pkmax_i(pkmax_i(L[0], L[1]), pkmax_i(L[2], L[3])), pkmax_i(pkmax_i(L[4], L[5]), pkmax_i(L[6], L[7])));
  return max((int)(short)(A & 0xffffu), (int)(short)(A >> 16));
}

// ---- FAST, second formulation (default): one WAVE per cell, no workgroup barriers.
//
// The phases of the per-cell pipeline (stage, quick test, exact score, NMS, ordered emission) have very different widths; in a
// workgroup-wide kernel every phase boundary is a barrier at which most waves idle.  Here every wave owns a run of <= 4
// horizontally adjacent cells and walks them one at a time entirely inside its own LDS slice (~5.4 KB: 28 waves per CU): all
// synchronisation is the in-order execution of one wave's LDS operations and a compute unit holds independent waves in
// different phases.  63 VGPRs; 7 waves per SIMD is what the LDS slices allow; holding the NEXT cell's tile in registers while
// the current one is processed costs 15 registers = one wave per SIMD and measured slower (DESIGN lessons 13, 18).
//   stage   cell ROI (<= 66 x 66) as bytes, shifted one column when that makes the tested region start on an even column (the
//           shift happens in registers: v_alignbyte over one extra aligned dword; LDS stores stay 16-byte aligned)
//   A1      SWAR quick test, two pixels per lane in 16-bit fields: the 16-bit pairs are cut out of aligned dwords with
//           v_perm_b32 (selectors per lane: the pair starts at byte 0 or 2), ten dwords per pair in five ds_read2_b32; packed
//           min / max over the four antipodal pairs, one biased subtract / add per polarity (see below).  Lanes = (row in a
//           band of RI rows, pixel pair): rows are 64 bytes apart, so the lanes of a 32-lane LDS group hit distinct banks.
//           Two tiers: the antipodal pairs (0, 8), (4, 12) first, the other two only if some lane of the wave passes.
//           Survivors -> 384-entry list with their polarity, scored (A2) and emptied whenever more than 256 are waiting.
//           The whole pass runs at iniThFAST first and is repeated at minThFAST (from the tile that is still staged) only for a
//           cell that kept nothing: the reference's own order (L/src/ORBextractor.cc:773-780)
//   A2      exact cornerScore of the surviving polarity: ring held as eight packed pairs, one 9-arc max-min network of packed
//           16-bit min / max for either polarity (arc9_maxmin_pk) -> score plane (tested region + 1-pixel zero frame)
//   B       strict 3x3 NMS inside the cell with lane = survivor (the list still holds every scored pixel; nine LDS reads in flight
//           per lane); kept pixels set bits, one 32-bit word per tested row.  Cells whose list was recycled (> 256 survivors)
//           walk the bitmap instead (lane = word)
//   C       row-major emission from the bitmap, one packed wave scan for the output offsets
#ifndef FC_LIST_CAP
#define FC_LIST_CAP 384
#endif
#define FC_Q1_CAP 128    // queue of tier-1 survivors: it holds < 64 entries between tier-2 rounds and an iteration adds <= 64
#if FC_TIMING
// tools/fc_phase_profile.py: wave-cycles per phase (wait for pixels, stage + clear, A1, A2, NMS, scan + emit) by s_memtime,
// accumulated per wave in scalars and added to one of 4096 slots at the end (one slot would serialise 660 k atomics on one
// cache line: the kernel took 6 ms)
__device__ unsigned long long g_fc_prof[4096 * 8];   // 4096 slots (spread the atomics), summed on the host
extern "C" int orbfe_debug_fc_profile(unsigned long long* out, int reset) {
  static unsigned long long h[4096 * 8];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_fc_prof), sizeof(h)) != hipSuccess) return 1;
  for (int i = 0; i < 8; i++) out[i] = 0;
  for (int sl = 0; sl < 4096; sl++)
    for (int i = 0; i < 8; i++) out[i] += h[sl * 8 + i];
  if (reset) { memset(h, 0, sizeof(h)); if (hipMemcpyToSymbol(HIP_SYMBOL(g_fc_prof), h, sizeof(h)) != hipSuccess) return 1; }
  return 0;
}
#endif
#ifndef FC_WAVES_PER_EU
#define FC_WAVES_PER_EU 7
#endif
#ifndef FC_WG_WAVES
#define FC_WG_WAVES 4   // waves (= runs of cells) per workgroup; the waves share nothing, but a workgroup's LDS and wave slots are held until its last wave ends
#endif
// LDS bytes of one wave's slice: byte tile, score plane, bitmap of scored pixels (nbw words), survivor list, tier-1 queue
__host__ __device__ inline int fc_wave_lds(int rows_max, int pb, int sc_bytes, int nbw) {
  return rows_max * pb + sc_bytes + nbw * 4 + FC_LIST_CAP * 2 + FC_Q1_CAP * 2;
}
template <int PB, int NLD>   // PB: bytes per staged row (64 or 96); NLD: load rounds of 64 lanes x 16 bytes per cell
__global__ __launch_bounds__(64 * FC_WG_WAVES, FC_WAVES_PER_EU) void fast_cells_kernel(PyrView pyr, const CellDesc* __restrict__ cells,
                                                          const FastGroup* __restrict__ runs, int n_runs, int total_cells,
                                                          int rows_max, int sc_bytes, int nbw, int32_t* __restrict__ cell_cnt,
                                                          uint32_t* __restrict__ slots, unsigned long long slots_per_image,
                                                          int ini_th, int min_th, int xcd_run_shift) {
  extern __shared__ __attribute__((aligned(16))) uint8_t fc_smem[];
  const int lane = threadIdx.x & (WAVE - 1), wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* tile = fc_smem + wid * fc_wave_lds(rows_max, PB, sc_bytes, nbw);
  uint8_t* sc = tile + rows_max * PB;
  uint32_t* scb = reinterpret_cast<uint32_t*>(sc + sc_bytes);   // bitmap of scored pixels, row-major over the tested region
  uint16_t* list = reinterpret_cast<uint16_t*>(scb + nbw);      // quick-test survivors (tile index | polarity)
  uint16_t* q1 = list + FC_LIST_CAP;                            // queue of tier-1 survivors: LDS address of a lane's pair window | column parity
  int img = blockIdx.y;
  const int nblk = (n_runs + FC_WG_WAVES - 1) / FC_WG_WAVES;
  const int q = blockIdx.x >> 3;
  const int unit = 8 << (xcd_run_shift < 0 ? 0 : xcd_run_shift);
  int bid = (xcd_run_shift < 0 || (int)blockIdx.x >= (nblk / unit) * unit)
                ? (int)blockIdx.x
                : ((q >> xcd_run_shift) << (xcd_run_shift + 3)) + ((blockIdx.x & 7) << xcd_run_shift) +
                      (q & ((1 << xcd_run_shift) - 1));
  if (xcd_run_shift == -2) {
    // whole images per XCD (workgroups go to the XCDs round-robin in linear order): XCD j walks images j, j + 8, ... one after
    // the other, so the halo rows / 128-byte lines that neighbouring cells share are fetched into ONE L2 once
    const unsigned gx = gridDim.x;
    const unsigned lin = blockIdx.y * gx + blockIdx.x;
    const unsigned grp = lin / (8u * gx);
    if (8u * grp + 8u <= gridDim.y) {
      const unsigned within = lin - grp * 8u * gx;
      img = (int)(8u * grp + (within & 7u));
      bid = (int)(within >> 3);
    }
  }
  const int rid = bid * FC_WG_WAVES + wid;
  if (rid >= n_runs) return;   // no barriers below
  const FastGroup g = runs[rid];
  const int level = g.level;
  const int pitch = pyr.pitch[level];
  const uint8_t* plane = pyr.base[level] + (size_t)img * pyr.img_stride[level];
  const uint32_t tile_a = (uint32_t)(uintptr_t)tile;

#if FC_TIMING
  uint32_t tacc0 = 0, tacc1 = 0, tacc2 = 0, tacc3 = 0, tacc4 = 0, tacc5 = 0, tprev = (uint32_t)__builtin_readcyclecounter();
#endif
  // a cell's descriptor through the scalar cache (eight dwords at a wave-uniform address): left to itself the compiler reads the 16-bit
  // fields with vector loads, one memory round trip after the other
  static_assert(sizeof(CellDesc) == 32, "eight dwords");
  auto load_cell = [&](int idx) {
    const __attribute__((address_space(4))) uint32_t* q =
        (const __attribute__((address_space(4))) uint32_t*)(uintptr_t)(cells + __builtin_amdgcn_readfirstlane(idx));
    CellDesc c;
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = q[j];
    __builtin_memcpy(&c, w, sizeof(c));
    return c;
  };
  for (int k = 0; k < g.n_cells; k++) {
    const CellDesc cd = load_cell(g.first_cell + k);
    // ---- the cell's pixels: every lane loads in every round (row and chunk clamped into the cell: a duplicate load and,
    //      below, a duplicate LDS store of the same bytes cost nothing, a divergent branch around them does)
    uint4 pv[NLD];
    uint32_t pe[NLD];
    {
      const int ndq = ((cd.x0 & 15) + (((cd.x0 & 15) + 3) & 1) + cd.cols + 15) >> 4;   // chunks of the SHIFTED row
      const uint8_t* src = plane + (size_t)cd.y0 * pitch + (cd.x0 & ~15);
      // a 16-byte chunk of a TILED level is one tile row; the dword in front of it the last dword of the tile row to its left
      const bool ltiled = (pyr.tiled >> level) & 1u;
      const uint32_t tstep = (uint32_t)(pitch >> 4) << 7;
      auto chunk_ptr = [&](int r, int c) {
        const int y = cd.y0 + r;
        return ltiled ? plane + (uint32_t)(y >> 3) * tstep + ((uint32_t)(((cd.x0 & ~15) >> 4) + c) << 7) + (uint32_t)((y & 7) * 16)
                      : src + (size_t)r * pitch + 16 * c;
      };
      auto front_ptr = [&](int r, int c, const uint8_t* p) {   // x0 >= 16: never before the row
        return ltiled ? p - 128 + 12 : p - 4;
      };
      if constexpr (PB == 64) {
        // four 16-byte chunks per staged row: lane -> (row, chunk) by shift and mask, sixteen rows per round
        // (three-chunk cells -- seven of ten at KITTI -- in TWO rounds, lane -> (i / 3, i % 3): measured 0.4285-0.4318 ms against 0.4229-0.426;
        //  unlike the describe kernel's, this kernel's load instructions are not what its vector-memory path is busy with: round 6)
        const int c = min(lane & 3, ndq - 1);
#pragma unroll
        for (int kk = 0; kk < NLD; kk++) {
          const int r = min((lane >> 2) + 16 * kk, cd.rows - 1);
          const uint8_t* p = chunk_ptr(r, c);          pv[kk] = *reinterpret_cast<const uint4*>(p);
          pe[kk] = ((cd.x0 & 15) + 3) & 1 ? *reinterpret_cast<const uint32_t*>(front_ptr(r, c, p)) : 0u;   // the dword in front: only a shifted tile needs it (wave-uniform, -1 %)
        }
      } else {
        const int items = cd.rows * ndq;
        const float inv = 1.0f / (float)ndq;
#pragma unroll
        for (int kk = 0; kk < NLD; kk++) {
          const int i = min(lane + WAVE * kk, items - 1);
          const int r = (int)((i + 0.5f) * inv), c = i - r * ndq;
          const uint8_t* p = chunk_ptr(r, c);
          pv[kk] = *reinterpret_cast<const uint4*>(p);
          pe[kk] = *reinterpret_cast<const uint32_t*>(front_ptr(r, c, p));
        }
      }
    }
#if FC_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FC_T(0);   // waiting for the cell's pixels
#endif
    const int cols = cd.cols, rows = cd.rows;
    const int xo = cd.x0 & 15, sh = (xo + 3) & 1, xs = xo + sh;
    const int ndq = (xs + cols + 15) >> 4;
    const int th = rows - 6, tw = cols - 6;
    const int c_lo = xs + 3, c_hi = xs + cols - 3;
    const int SCP = tw + 2;
    const int bsh = tw > 32 ? 6 : 5;   // bitmaps: one word (two for wide cells) per tested row, so a bit index splits by shift and mask
    // ---- stage (shifted by `sh` columns), clear the score plane and the bitmaps
    {
      const int items = rows * ndq;
      const float inv = 1.0f / (float)ndq;
#pragma unroll
      for (int kk = 0; kk < NLD; kk++) {
        int r, c;
        if constexpr (PB == 64) { r = min((lane >> 2) + 16 * kk, rows - 1); c = min(lane & 3, ndq - 1); }
        else { const int i = min(lane + WAVE * kk, items - 1); r = (int)((i + 0.5f) * inv); c = i - r * ndq; }
        uint4 d = pv[kk];
        if (sh) {   // pixel j of the chunk moves to column j + 1: the first byte comes from the dword in front
          d.w = __builtin_amdgcn_alignbyte(d.w, d.z, 3);
          d.z = __builtin_amdgcn_alignbyte(d.z, d.y, 3);
          d.y = __builtin_amdgcn_alignbyte(d.y, d.x, 3);
          d.x = __builtin_amdgcn_alignbyte(d.x, pe[kk], 3);
        }
        *reinterpret_cast<uint4*>(tile + r * PB + 16 * c) = d;
      }
      const int nsc = ((th + 2) * SCP + 15) >> 4;
      for (int i = lane; i < nsc; i += WAVE) reinterpret_cast<uint4*>(sc)[i] = make_uint4(0, 0, 0, 0);
      // (the bitmap is cleared where a cell first needs it: when its list is recycled)
    }
    FC_T(1);   // LDS staging + clears

    // ---- A2 (called when the list is nearly full -- `mark`: the list is about to be recycled, so scored pixels are also
    //      recorded in the bitmap -- and at the end): exact score of list[0 .. n), the polarity (or, about once in 10^4, the
    //      two polarities) the quick test left possible
    auto score_list = [&](int n, bool mark, int th_cur) {
      // A pixel whose two polarities both survived the quick test (a blurred edge through the centre: 3-8 % of the survivors
      // on the upper pyramid levels) needs both networks.  Running the second one under a wave-uniform branch cost a whole
      // network whenever ANY of the 64 lanes had such a pixel -- nearly every round.  Instead the pixel is scored as dark here and
      // appended to the list once more as bright-only (at most one of the two scores can reach the threshold: a ring has no room
      // for two 9-arcs); only when the list is full does the second network run in place.
      int n_end = n;
      for (int done = 0; done < n_end;) {
        const int start = done;
        const int lim = min(start + WAVE, n_end);   // this round's entries
        const int i = start + lane;
        done = lim;
        uint32_t en = i < lim ? list[i] : 0u;
        int e = (int)(en & 0x3fffu);
        int y = PB == 64 ? (e >> 6) : (int)((e + 0.5f) * (1.0f / PB));
        int x = e - y * PB;
        bool valid = i < lim && x < c_hi;   // not the pair straddling the right edge of the tested region
        const bool both = valid && (en & 0xC000u) == 0xC000u;
        const unsigned long long mb = __ballot(both);
        bool second_here = false;
        if (mb) {   // wave-uniform
          const int nb = __popcll(mb);
          if (n_end + nb <= FC_LIST_CAP) {
            const int r = __builtin_amdgcn_mbcnt_hi((uint32_t)(mb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mb, (uint32_t)n_end));
            if (both) list[r] = (uint16_t)((uint32_t)e | 0x4000u);
            if (lim == n_end && lim - start + nb <= WAVE) {
              // last round with idle lanes: they take the bright halves right away instead of forming a round of their own
              if (i >= lim && i < lim + nb) {
                en = list[i];
                e = (int)(en & 0x3fffu);
                y = PB == 64 ? (e >> 6) : (int)((e + 0.5f) * (1.0f / PB));
                x = e - y * PB;
                valid = true;
              }
              done = lim + nb;
            }
            n_end += nb;
          } else {
            second_here = true;
          }
        }
        if (!valid) continue;
        // the centre and the sixteen ring bytes, packed in ring order as eight (q_2j, q_2j+1) pairs (d16 byte loads would
        // build the pairs for free, but with SRAM ECC they zero the other half of the register)
        // (addressed from the ring's top-left corner: every offset is then a non-negative immediate of ds_read_u8, where
        // offsets relative to the centre cost eight address additions)
        int eb = e - (3 * PB + 3);
        asm("" : "+v"(eb));   // keep THIS base: the compiler would fold the constant back and re-create the negative offsets
        const uint8_t* c = tile + eb;
        const uint32_t v = c[3 * PB + 3];
        uint32_t P[8];
#pragma unroll
        for (int j = 0; j < 8; j++)
          P[j] = (uint32_t)c[(RDY[2 * j] + 3) * PB + RDX[2 * j] + 3] | ((uint32_t)c[(RDY[2 * j + 1] + 3) * PB + RDX[2 * j + 1] + 3] << 16);
        const uint32_t VV = v | (v << 16);
        const bool bright = (en & 0xC000u) == 0x4000u;   // bright only; dark first where both are possible
        int s = arc9_maxmin_pk(P, VV, bright ? ~0u : 0u) + (bright ? 1 : 0);
        if (second_here) {   // list full (wave-uniform): the bright network of the two-polarity pixels in place
          if (both) s = max(s, arc9_maxmin_pk(P, VV, ~0u) + 1);
        }
        if (s - 1 >= th_cur) {
          const int ty = y - 3, tx = x - c_lo;
          sc[(ty + 1) * SCP + tx + 1] = (uint8_t)(s - 1);
          if (mark) {
            const int p = (ty << bsh) + tx;
            atomicOr(&scb[p >> 5], 1u << (p & 31));
          }
        }
      }
    };

    // The reference's own order (L/src/ORBextractor.cc:773-780): cv::FAST(cell, iniThFAST) first, cv::FAST(cell, minThFAST)
    // only when that returned nothing.  Pass 0 runs quick test, score, NMS at ini_th; a cell whose pass 0 keeps no pixel
    // (wave-uniform) repeats them at min_th from the tile that is still staged.
    uint32_t keep[2] = {0u, 0u};
    int total = 0;
    bool was_flushed = false;
    for (int pass = 0; pass < 2; pass++) {
      const int th_cur = pass ? min_th : ini_th;
      const uint32_t C = (uint32_t)(0x8000 - th_cur - 1) * 0x00010001u;
      bool flushed = false;
      int wcnt = 0;
      // ---- A1
      if (th > 0 && tw > 0) {
        const int ppr = cd.ppr;                        // (tw + 1) >> 1, <= 30
        const int RI = cd.ri;                          // WAVE / ppr: rows per iteration, >= 2
        const int rl = (int)((lane + 0.5f) * cd.inv_ppr), pl = lane - rl * ppr;
        const bool lane_ok = rl < RI;
        const int n_it = cd.n_it;                      // (th + RI - 1) / RI
        const int x = c_lo + 2 * pl;                   // even: the pair (x, x + 1) starts at byte 0 or 2 of its dword
        const bool odd2 = (x & 2) != 0;
        const uint32_t selV = odd2 ? 0x0c030c02u : 0x0c010c00u;    // (x, x+1) and (x, x+1) of rows +-3
        const uint32_t selM = odd2 ? 0x0c040c03u : 0x0c020c01u;    // (x-3, x-2) out of dwords {D(x)-1, D(x)}
        const uint32_t selP = odd2 ? 0x0c020c01u : 0x0c040c03u;    // (x+3, x+4) out of dwords {D(x+2), D(x+2)+1}
        // addresses of row (y - 3): a0 = the dword of x minus one dword (the centre row reads {D-1, D}); a1 = the dword of
        // x - 2, which is also the dword of x + 2 minus one dword (x = 4k: D(x) - 1; x = 4k + 2: D(x))
        uint32_t a0 = tile_a + rl * PB + ((x >> 2) << 2) - 4;
        uint32_t a1 = a0 + (odd2 ? 4u : 0u);
        // Tier 1 runs over all the cell's pixels; the lanes that pass it (a fifth of the 64 on a triggered iteration) used to take the
        // whole wave through tier 2 and the survivor push (35 vector instructions at ~20 % lane use).  Here they only queue their
        // pair (`q1`, first in first out = row-major order: the LDS address of the pair's window | its column parity); tier 2 + push
        // run over 64 QUEUED pairs at a time: whenever the queue holds a wave's worth, and once at the end of the cell (the tile is
        // restaged for the next one).
        // The tier-1 loop itself is one block of assembly: measured on this kernel a scalar instruction costs what a vector
        // instruction costs (eight s_add per iteration: + 3.1 % alone, + 1.1 % on the step; eight v_add: + 3.5 % / + 1.3 %), and the
        // compiler's loop carried ~20 of them per iteration (loop-carried conditions materialised as 64-bit masks, exec save /
        // restore around the queue store, a branch per condition).  Per iteration here: 3 LDS reads, 19 vector, 8 scalar
        // instructions, + 4 / 4 / 1 on the 57 % of the iterations in which a lane passes.
        // The block is the only form of the loop and has two preconditions: v_bitop3_b32 exists on gfx950 alone, and the fixed
        // v64 .. v69 lie inside the wave's register budget only while that is at least 70 (512 / FC_WAVES_PER_EU, in steps of 8).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "fast_cells_kernel: the tier-1 loop is gfx950 assembly (v_bitop3_b32)"
#endif
        static_assert(FC_WAVES_PER_EU <= 7, "the tier-1 assembly names v64 .. v69: eight waves per SIMD leave a wave 64 registers");
        const unsigned long long m_full = __ballot(lane_ok), m_last = __ballot(lane_ok && rl < th - (n_it - 1) * RI);
        const uint32_t oddbit = odd2 ? 1u : 0u;
        const uint32_t q_base = (uint32_t)(uintptr_t)q1, q_limit = q_base + 2u * WAVE;
        uint32_t q_addr = q_base;
        int it = 0;
        for (int phase = 0; phase < 2; phase++) {
          const unsigned long long actm = phase ? m_last : m_full;
          const int nit = __builtin_amdgcn_readfirstlane(phase ? n_it : n_it - 1);   // (uniform values the compiler keeps in vector registers)
          const int step = __builtin_amdgcn_readfirstlane(RI * PB);
          for (;;) {
            if (it < nit) {
              uint32_t tV, tA, tB, tC, tD, tE;
              uint32_t sc_;
              asm volatile(
                  "1:\n\t"
                  "ds_read2_b32 v[64:65], %[a0] offset0:1 offset1:%[K61]\n\t"
                  "ds_read2_b32 v[66:67], %[a0] offset0:%[K30] offset1:%[K31]\n\t"
                  "ds_read2_b32 v[68:69], %[a1] offset0:%[K31] offset1:%[K32]\n\t"
                  "s_add_u32 %[it], %[it], 1\n\t"
                  "s_waitcnt lgkmcnt(0)\n\t"
                  "v_perm_b32 %[tV], 0, v67, %[selV]\n\t"          // V: the centre pair
                  "v_perm_b32 %[tA], 0, v64, %[selV]\n\t"          // Q8 (row y - 3)
                  "v_perm_b32 %[tB], 0, v65, %[selV]\n\t"          // Q0 (row y + 3)
                  "v_perm_b32 %[tC], v67, v66, %[selM]\n\t"        // Q12 (x - 3, x - 2)
                  "v_perm_b32 %[tD], v69, v68, %[selP]\n\t"        // Q4 (x + 3, x + 4)
                  "v_pk_min_u16 %[tE], %[tB], %[tA]\n\t"           // min(Q0, Q8)
                  "v_pk_max_u16 %[tA], %[tB], %[tA]\n\t"           // max(Q0, Q8)
                  "v_pk_min_u16 %[tB], %[tD], %[tC]\n\t"           // min(Q4, Q12)
                  "v_pk_max_u16 %[tC], %[tD], %[tC]\n\t"           // max(Q4, Q12)
                  "v_pk_max_u16 %[tE], %[tE], %[tB]\n\t"           // lo
                  "v_pk_min_u16 %[tA], %[tA], %[tC]\n\t"           // hi
                  "v_add_u32 %[tB], %[C], %[tV]\n\t"               // AD = V + C
                  "v_sub_u32 %[tC], %[C], %[tV]\n\t"               // AB = C - V
                  "v_sub_u32 %[tB], %[tB], %[tE]\n\t"              // AD - lo
                  "v_add_u32 %[tC], %[tA], %[tC]\n\t"              // hi + AB
                  "v_bitop3_b32 %[tB], %[tB], %[M], %[tC] bitop3:0xc8\n\t"   // (dark | bright) & 0x80008000
                  "v_cmp_ne_u32 vcc, 0, %[tB]\n\t"
                  "s_and_b64 vcc, vcc, %[actm]\n\t"
                  "s_cbranch_scc0 2f\n\t"
                  "v_mbcnt_lo_u32_b32 %[tA], vcc_lo, 0\n\t"
                  "v_mbcnt_hi_u32_b32 %[tA], vcc_hi, %[tA]\n\t"
                  "v_or_b32 %[tC], %[a0], %[odd]\n\t"
                  "v_lshl_add_u32 %[tA], %[tA], 1, %[qa]\n\t"
                  "s_mov_b64 exec, vcc\n\t"
                  "ds_write_b16 %[tA], %[tC]\n\t"
                  "s_mov_b64 exec, -1\n\t"
                  "s_bcnt1_i32_b64 %[sc], vcc\n\t"
                  "s_lshl1_add_u32 %[qa], %[sc], %[qa]\n\t"
                  "2:\n\t"
                  "v_add_u32 %[a0], %[step], %[a0]\n\t"
                  "v_add_u32 %[a1], %[step], %[a1]\n\t"
                  "s_cmp_ge_u32 %[qa], %[ql]\n\t"
                  "s_cbranch_scc1 3f\n\t"
                  "s_cmp_lt_i32 %[it], %[nit]\n\t"
                  "s_cbranch_scc1 1b\n\t"
                  "3:"
                  : [a0] "+v"(a0), [a1] "+v"(a1), [it] "+s"(it), [qa] "+s"(q_addr), [tV] "=&v"(tV), [tA] "=&v"(tA), [tB] "=&v"(tB),
                    [tC] "=&v"(tC), [tD] "=&v"(tD), [tE] "=&v"(tE), [sc] "=&s"(sc_)
                  : [selV] "v"(selV), [selM] "v"(selM), [selP] "v"(selP), [odd] "v"(oddbit), [C] "s"(C), [M] "s"(0x80008000u),
                    [actm] "s"(actm), [step] "s"(step), [ql] "s"(q_limit), [nit] "s"(nit),
                    [K61] "n"(6 * PB / 4 + 1), [K30] "n"(3 * PB / 4), [K31] "n"(3 * PB / 4 + 1), [K32] "n"(3 * PB / 4 + 2)
                  : "memory", "vcc", "scc", "v64", "v65", "v66", "v67", "v68", "v69");
            }
            const int qn = (int)(q_addr - q_base) >> 1;
            if (qn < WAVE && !(phase == 1 && it >= nit && qn > 0)) break;   // wave-uniform: no round due
            // ---- a round of tier 2 over the first min(qn, 64) queued pairs: lane = pair
            const bool on = lane < qn;
            uint32_t ev = q1[lane];
            ev = on ? ev : tile_a;            // idle lanes test the tile's first window and push nothing
            if (qn > WAVE) {                    // what is left moves to the front of the queue
              const uint32_t rest = q1[WAVE + min(lane, qn - WAVE - 1)];
              if (lane < qn - WAVE) q1[lane] = (uint16_t)rest;
            }
            q_addr = q_base + 2u * (uint32_t)(qn > WAVE ? qn - WAVE : 0);
            const uint32_t o1 = ev & 1u, b0 = ev - o1, b1 = b0 + 4u * o1, k2 = o1 * 0x00020002u;
            const uint32_t e2 = b0 - tile_a + (uint32_t)(3 * PB + 4) + 2u * o1;   // tile index of the pair's first pixel
            const uint32_t sV = 0x0c010c00u + k2, sX = 0x0c030c02u - k2, sM = 0x0c020c01u + k2, sP = 0x0c040c03u - k2;
            unsigned long long p08, pc, pp, p62, p1014;
            asm volatile(
                "ds_read2_b32 %0, %5 offset0:1 offset1:%7\n\t"
                "ds_read2_b32 %1, %5 offset0:%8 offset1:%9\n\t"
                "ds_read2_b32 %2, %6 offset0:%9 offset1:%10\n\t"
                "ds_read2_b32 %3, %6 offset0:%11 offset1:%12\n\t"
                "ds_read2_b32 %4, %6 offset0:%13 offset1:%14\n\t"
                "s_waitcnt lgkmcnt(0)"
                : "=&v"(p08), "=&v"(pc), "=&v"(pp), "=&v"(p62), "=&v"(p1014)
                : "v"(b0), "v"(b1), "n"(6 * PB / 4 + 1), "n"(3 * PB / 4), "n"(3 * PB / 4 + 1), "n"(3 * PB / 4 + 2),
                  "n"(PB / 4 + 1), "n"(5 * PB / 4 + 1), "n"(PB / 4), "n"(5 * PB / 4)
                : "memory");
            {
              const uint32_t D0 = (uint32_t)(pc >> 32), Dm = (uint32_t)pc;
              const uint32_t V = __builtin_amdgcn_perm(0u, D0, sV);
              const uint32_t Q8 = __builtin_amdgcn_perm(0u, (uint32_t)p08, sV), Q0 = __builtin_amdgcn_perm(0u, (uint32_t)(p08 >> 32), sV);
              const uint32_t Q12 = __builtin_amdgcn_perm(D0, Dm, sM);
              const uint32_t Q4 = __builtin_amdgcn_perm((uint32_t)(pp >> 32), (uint32_t)pp, sP);
              const uint32_t Q6 = __builtin_amdgcn_perm(0u, (uint32_t)p62, sX), Q2 = __builtin_amdgcn_perm(0u, (uint32_t)(p62 >> 32), sX);
              const uint32_t Q10 = __builtin_amdgcn_perm(0u, (uint32_t)p1014, sX), Q14 = __builtin_amdgcn_perm(0u, (uint32_t)(p1014 >> 32), sX);
              const uint32_t AD = V + C, AB = C - V;
              const uint32_t lo = pkmax(pkmax(pkmin(Q0, Q8), pkmin(Q4, Q12)), pkmax(pkmin(Q2, Q10), pkmin(Q6, Q14)));
              const uint32_t hi = pkmin(pkmin(pkmax(Q0, Q8), pkmax(Q4, Q12)), pkmin(pkmax(Q2, Q10), pkmax(Q6, Q14)));
              const uint32_t dark = AD - lo, brt = hi + AB;
              const uint32_t G = on ? ((dark & 0x80008000u) | ((brt >> 1) & 0x40004000u)) : 0u;
              const bool has0 = (G & 0xC000u) != 0, has1 = (G >> 30) != 0;
              // the list stays in row-major order (the queue is first in, first out; a lane's two pixels are neighbours): the NMS
              // below emits straight from it
              const unsigned long long m0 = __ballot(has0), m1 = __ballot(has1);
              const int c0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, (uint32_t)wcnt));
              const int i0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, (uint32_t)c0));
              const int i1 = i0 + (has0 ? 1 : 0);
              if (has0) list[i0] = (uint16_t)((G & 0xC000u) | e2);
              if (has1) list[i1] = (uint16_t)(((G >> 16) & 0xC000u) | (e2 + 1));
              wcnt += __popcll(m0) + __popcll(m1);
            }
            if (wcnt > FC_LIST_CAP - 2 * WAVE) {   // wave-uniform
              FC_T(2);
              if (!flushed)
                for (int i = lane; i < nbw; i += WAVE) scb[i] = 0;
              flushed = true;
              score_list(wcnt, true, th_cur);
              FC_T(3);
              wcnt = 0;
            }
          }
        }
        FC_T(2);
        score_list(wcnt, flushed, th_cur);
        FC_T(3);
      }

      // ---- B: strict 3x3 NMS inside the cell.
      if (!flushed) {
        // lane = survivor: the list still holds every scored pixel of the cell, in row-major order -- the order the reference's
        // keypoints of a cell come in -- so a kept pixel goes straight to its output slot: rank = kept pixels in front of it.
        // Nine reads in flight together.  (Pass 0 of a cell that keeps nothing writes nothing.)
        uint32_t* slot = slots + (size_t)img * slots_per_image + cd.slot_off;
        int emitted = 0;
        for (int base = 0; base < wcnt; base += WAVE) {
          const int i = min(base + lane, wcnt - 1);
          const uint32_t en = list[i];
          const int e = (int)(en & 0x3fffu);
          const int y = PB == 64 ? (e >> 6) : (int)((e + 0.5f) * (1.0f / PB));
          const int x = e - y * PB;
          const int ty = y - 3, tx = x - c_lo;
          const uint8_t* s = sc + (ty + 1) * SCP + min(tx, tw - 1) + 1;
          const int v = s[0];
          const int n0 = s[-SCP - 1], n1 = s[-SCP], n2 = s[-SCP + 1], n3 = s[-1], n4 = s[1], n5 = s[SCP - 1], n6 = s[SCP], n7 = s[SCP + 1];
          const bool kp = (base + lane < wcnt) & (x < c_hi) & (v > n0) & (v > n1) & (v > n2) & (v > n3) & (v > n4) & (v > n5) & (v > n6) & (v > n7);   // v = 0: not scored
          const unsigned long long mk = __ballot(kp);
          const int off = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, (uint32_t)emitted));
          const uint32_t rx = (uint32_t)(tx + 3 + cd.x0 - ORBFE_EDGE), ry = (uint32_t)(ty + 3 + cd.y0 - ORBFE_EDGE);
          if (kp && off < cd.slot_cap) slot[off] = rx | (ry << 12) | ((uint32_t)v << 24);
          emitted += __popcll(mk);
        }
        total = emitted;
      } else {
        // the list was recycled (more than 256 quick-test survivors in one cell): lane l walks the bits of words l and l + 64
        // of the bitmap of scored pixels
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const int w = lane + WAVE * h;
          uint32_t m = w < nbw ? scb[w] : 0u;
          keep[h] = 0;
          while (m) {
            const int b = __ffs((int)m) - 1;
            m &= m - 1;
            const int p = w * 32 + b;
            const int ty = p >> bsh, tx = p & ((1 << bsh) - 1);
            const uint8_t* s = sc + (ty + 1) * SCP + tx + 1;
            // all nine reads in flight together: with `&&` every comparison waited for its own LDS round trip
            const int v = s[0];
            const int n0 = s[-SCP - 1], n1 = s[-SCP], n2 = s[-SCP + 1], n3 = s[-1], n4 = s[1], n5 = s[SCP - 1], n6 = s[SCP], n7 = s[SCP + 1];
            const bool kp = (v > n0) & (v > n1) & (v > n2) & (v > n3) & (v > n4) & (v > n5) & (v > n6) & (v > n7);
            if (kp) keep[h] |= 1u << b;
          }
        }
        total = __popcll(__ballot(keep[0] != 0u || keep[1] != 0u));   // > 0 <=> the cell keeps a pixel
      }
      was_flushed = flushed;
      FC_T(4);   // NMS (and, for a cell whose list was never recycled, emission)
      if (total != 0 || pass == 1) break;
      // nothing at ini_th: start over at min_th (the score plane may hold pass 0's plateau pixels; a recycled list's bitmap is
      // cleared again when pass 1 recycles)
      {
        const int nsc = ((th + 2) * SCP + 15) >> 4;
        for (int i = lane; i < nsc; i += WAVE) reinterpret_cast<uint4*>(sc)[i] = make_uint4(0, 0, 0, 0);
      }
    }

    // ---- C: (recycled lists only) row-major emission from registers (one wave scan per bitmap half gives the output offsets)
    if (!was_flushed) {
      if (lane == 0) cell_cnt[(size_t)img * total_cells + g.first_cell + k] = total < cd.slot_cap ? total : cd.slot_cap;
      FC_T(5);
    } else {
      const int pk = __popc(keep[0]) | (__popc(keep[1]) << 16);   // both halves in one packed wave scan
      const int in = wave_incl_scan(pk);
      const int tot = __builtin_amdgcn_readlane(in, WAVE - 1);
      const int tot0 = tot & 0xffff, n_out = tot0 + (tot >> 16);
      const int ex = in - pk;
      uint32_t* slot = slots + (size_t)img * slots_per_image + cd.slot_off;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        int off = h ? tot0 + (ex >> 16) : (ex & 0xffff);
        uint32_t mask = keep[h];
        const int w = lane + WAVE * h;
        while (mask) {
          const int b = __ffs((int)mask) - 1;
          mask &= mask - 1;
          const int p = w * 32 + b;
          const int ty = p >> bsh, tx = p & ((1 << bsh) - 1);
          const uint32_t sv = sc[(ty + 1) * SCP + tx + 1];
          const uint32_t rx = (uint32_t)(tx + 3 + cd.x0 - ORBFE_EDGE), ry = (uint32_t)(ty + 3 + cd.y0 - ORBFE_EDGE);
          if (off < cd.slot_cap) slot[off] = rx | (ry << 12) | (sv << 24);
          off++;
        }
      }
      if (lane == 0) cell_cnt[(size_t)img * total_cells + g.first_cell + k] = n_out < cd.slot_cap ? n_out : cd.slot_cap;
      FC_T(5);   // scans + emission
    }
  }
#if FC_TIMING
  if (lane == 0) {
    unsigned long long* pr = g_fc_prof + (size_t)((rid * 2654435761u) >> 20) * 8;   // 4096 slots
    atomicAdd(&pr[0], (unsigned long long)tacc0); atomicAdd(&pr[1], (unsigned long long)tacc1);
    atomicAdd(&pr[2], (unsigned long long)tacc2); atomicAdd(&pr[3], (unsigned long long)tacc3);
    atomicAdd(&pr[4], (unsigned long long)tacc4); atomicAdd(&pr[5], (unsigned long long)tacc5);
    atomicAdd(&pr[6], 1ull);
    atomicAdd(&pr[7], (unsigned long long)g.n_cells);
  }
#endif
}

// ------------------------------------------------------------------------------------------------ launchers
void orbfe_launch_fast_cells(const PyrView& pyr, const CellDesc* cells, const FastGroup* groups, int n_groups, int total_cells,
                             int cell_rows, int cell_span, int sc_max, int bits_max, int32_t* cell_cnt, uint32_t* slots,
                             unsigned long long slots_per_image, int ini_th, int min_th, int n_images, hipStream_t s) {
  if (n_groups == 0) return;
  const int run_shift = -2;   // whole images per XCD (-1: plain blockIdx order, k >= 0: runs of 2^k workgroups per XCD)
  // wave per run of cells: per-wave LDS slice = byte tile + score plane + bitmap + list
  const int pb = cell_span <= 64 ? 64 : 96;
  const int sc_bytes = (sc_max + 15) & ~15;
  const int nbw = bits_max <= 64 * 32 ? 64 : 128;   // bitmap words (lane l owns words l and l + 64)
  const size_t lds = (size_t)FC_WG_WAVES * fc_wave_lds(cell_rows, pb, sc_bytes, nbw);
  const bool small = cell_rows <= 48;   // a cell loads in three rounds of sixteen rows
  dim3 grid4((n_groups + FC_WG_WAVES - 1) / FC_WG_WAVES, n_images);
#define FC_LAUNCH(PBV, NLDV)                                                                                                   \
  hipLaunchKernelGGL((fast_cells_kernel<PBV, NLDV>), grid4, dim3(64 * FC_WG_WAVES), lds, s, pyr, cells, groups, n_groups, total_cells,       \
                     cell_rows, sc_bytes, nbw, cell_cnt, slots, slots_per_image, ini_th, min_th, run_shift)
  if (lds > 48 * 1024) {   // never for the configured datasets (22 KB at KITTI); the largest cell (66 x 66) needs 46 KB
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fast_cells_kernel<96, 7>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fast_cells_kernel<64, 7>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  if (pb == 64 && small) FC_LAUNCH(64, 3);
  else if (pb == 64) FC_LAUNCH(64, 7);
  else FC_LAUNCH(96, 7);
#undef FC_LAUNCH
}
