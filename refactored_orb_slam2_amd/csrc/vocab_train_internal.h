// vocab_train_internal.h -- the arithmetic of DBoW2::TemplatedVocabulary::create, once, for the kernels (vocab_train_kernels.hip), for
// vocab_train.cpp and for host code that wants the same bits, plus the records the two units share.  __host__ __device__ inline
// functions; every value is an integer or a double that is exact, so the order of evaluation does not matter.
//
// Reference (D/ = Source/ThirdParty/DBoW2/DBoW2-local/):
//   HKmeansStep, initiateClustersKMpp, createWords, setNodeWeights   D/include/DBoW2/TemplatedVocabulary.h:640-994
//   FORB::meanValue, FORB::distance                                  D/src/FORB.cpp:24-100
//   RandomInt, RandomValue                                           D/../DUtils/Random.h
// Stated here and nowhere else:
//   the draw            vt_draw(seed, level, path, j): a splitmix64 chain over the key, reduced to 31 bits (0 .. RAND_MAX = 2^31 - 1)
//   the first centre    int(r / (RAND_MAX + 1.0) * n)                                   vt_first_index
//   the cut             (double)r / RAND_MAX * dist_sum, drawn again while it is 0.0    vt_cut, vt_cut_draw
//   the pick            the first index whose running sum of min_dists is >= cut, else the last index; the sums are integers, so
//                       `sum >= cut` is `sum >= ceil(cut)`: vt_cut_target, vt_pick
//   the majority        a bit of the mean is set when its count >= N / 2 + N % 2        vt_majority
//   the distance        popcount over eight 32-bit words                                 vt_hamming
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/orbfe.h"

#define VT_HD __host__ __device__ __forceinline__
#define VT_THREADS 256          // threads of a workgroup of every kernel: one per bit column of a descriptor
#define VT_CHUNK 1024           // positions of a segment one workgroup of the wide form walks; the most the narrow form holds in LDS
#define VT_MAX_K 20
#define VT_MAX_L 10
#define VT_NI_GROUPS 128        // workgroups (one word bitmap each) of the Ni pass, at most: fewer when the tree has more words than the
                                // training set has descriptors (empty clusters stay nodes), see vt_ni_groups
#define VT_RAND_MAX 2147483647.0

VT_HD uint64_t vt_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// draw j of the node at `level` (1 = the root's clustering) whose child indices from the root read `path` in base k
VT_HD uint32_t vt_draw(uint64_t seed, uint32_t level, uint64_t path, uint32_t j) {
  return (uint32_t)(vt_splitmix64(vt_splitmix64(vt_splitmix64(vt_splitmix64(seed) ^ (uint64_t)level) ^ path) ^ (uint64_t)j) >> 33);
}

VT_HD int vt_first_index(uint32_t r, int n) {
  const int i = (int)((double)r / (VT_RAND_MAX + 1.0) * (double)n);
  return i < n ? i : n - 1;
}
VT_HD double vt_cut(uint32_t r, int64_t dist_sum) { return (double)r / VT_RAND_MAX * (double)dist_sum; }
// the retry rule over any source of draws (`uint32_t draw()`): a cut of 0.0 is drawn again; dist_sum > 0
template <class Draw>
VT_HD double vt_cut_retry(Draw& draw, int64_t dist_sum) {
  double cut;
  do {
    cut = vt_cut(draw(), dist_sum);
  } while (cut == 0.0);
  return cut;
}
// the node's draws from counter *j on
struct VtKeyedDraws {
  uint64_t seed;
  uint32_t level;
  uint64_t path;
  uint32_t* j;
  VT_HD uint32_t operator()() { return vt_draw(seed, level, path, (*j)++); }
};
VT_HD double vt_cut_draw(uint64_t seed, uint32_t level, uint64_t path, uint32_t* j, int64_t dist_sum) {
  VtKeyedDraws draws{seed, level, path, j};
  return vt_cut_retry(draws, dist_sum);
}
VT_HD int64_t vt_cut_target(double cut) { return (int64_t)ceil(cut); }
// sequential form of the pick over n integer distances
VT_HD int vt_pick(const int32_t* min_dists, int n, double cut) {
  const int64_t target = vt_cut_target(cut);
  int64_t up = 0;
  for (int i = 0; i < n; i++) {
    up += min_dists[i];
    if (up >= target) return i;
  }
  return n - 1;
}
// Words are leaves, and a level creates at most n nodes (the sum of min(n_s, k) over its segments), so n_words <= L * n.  The bitmap
// region holds VT_NI_GROUPS bitmaps of n bits; a tree with more words gets fewer groups, never fewer than VT_NI_GROUPS / L >= 12.
VT_HD size_t vt_ni_bitmap_words(size_t n) { return (size_t)VT_NI_GROUPS * ((n + 31) / 32); }
VT_HD int vt_ni_groups(size_t n, size_t n_words) {
  const size_t g = vt_ni_bitmap_words(n) / ((n_words + 31) / 32);
  return (int)(g < (size_t)VT_NI_GROUPS ? g : (size_t)VT_NI_GROUPS);
}
VT_HD int vt_majority(int n) { return n / 2 + n % 2; }

#if defined(__HIP_DEVICE_COMPILE__)
#define VT_POPC(x) __popc(x)
#else
#define VT_POPC(x) __builtin_popcount(x)
#endif
VT_HD int vt_hamming(const uint32_t* a, const uint32_t* b) {
  int d = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d += VT_POPC(a[i] ^ b[i]);
  return d;
}

// ---- records shared by vocab_train.cpp and vocab_train_kernels.hip
enum { VT_SEG_KMEANS = 0, VT_SEG_TRIVIAL = 1 };
enum { VT_RUNNING = 0, VT_CONVERGED = 1, VT_CAPPED = 2 };
struct VtSegment {        // one node of the level in flight: a contiguous run of the permutation
  int32_t start, n;
  uint64_t path;
  int32_t kind;           // VT_SEG_*
  int32_t wide;           // 1: the wide form walks it; its chunks are [chunk0, chunk0 + ceil(n / VT_CHUNK)) in either form
  int32_t chunk0;
  int32_t wide_idx;       // ordinal among the level's wide segments: its block of bit counters
  int32_t centre0;        // first centre of the segment in the level's centre array = sum of min(n, k) over the segments before it;
  int32_t reserved;       // slot_base + centre0 + c names child c in leaf_slot
};
struct VtSegState {       // what the device keeps and reports per segment
  int32_t n_centres, state, rounds, draws;
  int32_t empty_events, short_seeding, changed, reserved;
  int64_t dist_sum;
  int32_t size[VT_MAX_K]; // members per cluster of the last association
};
struct VtChunk { int32_t seg, start, n, reserved; };   // start: position in the permutation
struct VtLevel {
  const uint8_t* desc;    // [N][32]
  int32_t* perm;          // [N] feature index by position
  int32_t* perm_next;     // [N]
  int32_t* assoc;         // [N] by position, -1 before the first association
  int32_t* min_dist;      // [N] by position
  int32_t* leaf_slot;     // [N] by FEATURE: slot of the deepest group so far
  const VtSegment* seg;
  VtSegState* st;
  uint8_t* centre;        // [sum of min(n_s, k)][32], a segment's at VtSegment::centre0
  uint32_t* count;        // [n_wide][k][256] bit counters of the wide form, a segment's at VtSegment::wide_idx
  const VtChunk* chunk;
  int64_t* chunk_sum;     // [n_chunks]
  int32_t* chunk_hist;    // [n_chunks][k], then the offsets of the partition
  int32_t* control;       // [0]: segments of the wide form still running
  const int32_t* wide_seg;    // [n_wide] the segments the wide form walks, and
  const int32_t* wide_chunk;  // [n_wide_chunks] their chunks: the grids of its kernels, so that a level of mostly narrow segments pays nothing
  int32_t n_seg, n_chunks, n_wide, n_wide_chunks, k, level, max_iterations, slot_base;
  uint64_t seed;
};

void vt_launch_init(int32_t* perm, int32_t* leaf_slot, int n, hipStream_t s);
void vt_launch_compact(const uint8_t* d_desc, const int32_t* d_start, int n_frames, int cap, uint8_t* out, hipStream_t s);
void vt_launch_level_begin(const VtLevel& lv, hipStream_t s);                 // states, assoc = -1, trivial segments
void vt_launch_narrow(const VtLevel& lv, const int32_t* seg_list, int n_list, hipStream_t s);
void vt_launch_seed_first(const VtLevel& lv, hipStream_t s);
void vt_launch_seed_step(const VtLevel& lv, int j, hipStream_t s);           // centre j of every wide segment
void vt_launch_round(const VtLevel& lv, hipStream_t s);                       // one association and its means, wide segments
void vt_launch_partition(const VtLevel& lv, hipStream_t s);
void vt_launch_leaf_translate(const int32_t* leaf_slot, const int32_t* slot_node, int n, int32_t* leaf_node, hipStream_t s);
void vt_launch_ni(const int32_t* word, const int32_t* image_start, int n_images, int n_words, int groups, uint32_t* bitmaps, int32_t* ni,
                  hipStream_t s);
