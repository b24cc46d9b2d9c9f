// kfdb_internal.h -- the arithmetic of KeyFrameDatabase's two detection functions, once, for the kernels (kfdb_kernels.hip) and for
// host code that wants the same bits, plus the launch record kfdb.cpp and the kernels share.  __host__ __device__ inline functions,
// compiled with -ffp-contract=off on both sides.
//
// Reference (L/ = Source/Libraries/ORB_SLAM2/, D/ = Source/ThirdParty/DBoW2/DBoW2-local/):
//   DetectLoopCandidates / DetectRelocalizationCandidates   L/src/KeyFrameDatabase.cc:72-193, :195-304
//   L1Scoring::score                                        D/src/ScoringObject.cpp:23-68
// Three things are stated here and nowhere else:
//   the ordered sum     score += fabs(vi - wi) - fabs(vi) - fabs(wi) over the common words in ASCENDING word order, in double, then
//                       (float)(-score / 2.0): kfdb_l1_term, kfdb_l1_finish, kfdb_score_ordered.  A strided or tree sum of the same
//                       terms rounds to another double and now and then to another float.
//   minCommonWords      int minCommonWords = maxCommonWords * 0.8f (:116, :231): a float product, truncated: kfdb_min_common_words
//   the accumulation    accScore / bestScore / pBestKF over the neighbours in their given order, in float (:151-166, :264-279), and
//                       0.75f * bestAccScore (:174, :286): KfdbAcc, kfdb_acc_start, kfdb_acc_neighbour, kfdb_min_score_to_retain
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/orbfe.h"

#define KFDB_HD __host__ __device__ __forceinline__
#define KFDB_WAVES 4    // waves of a workgroup of every kernel of kfdb_kernels.hip
#define KFDB_STRIP 64   // slots one workgroup of the common and the score pass walks: one lane of a wave each when the strip is scanned
#define KFDB_THREADS (KFDB_WAVES * 64)
#define KFDB_NEIGHBOURS ORBFE_KFDB_NEIGHBOURS
#define KFDB_WORK_ARRAYS 10   // [Q][n_slots] arrays of 4 bytes a call needs: words, first, score, carried and six of the selection

KFDB_HD int kfdb_min_common_words(int max_common_words) { return (int)((float)max_common_words * 0.8f); }

// vi is the query's value, wi the entry's (score(F->mBowVec, pKFi->mBowVec)); evaluated left to right as the reference's expression
KFDB_HD double kfdb_l1_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }
KFDB_HD float kfdb_l1_finish(double sum) { return (float)(-sum / 2.0); }

// the whole score of one pair, sequentially: both id lists ascend strictly.  The kernels find the same common words a wave at a
// time and add the same terms in the same order.
KFDB_HD float kfdb_score_ordered(const int32_t* q_ids, const double* q_vals, int nq, const int32_t* e_ids, const double* e_vals, int ne) {
  double sum = 0.0;
  int i = 0, j = 0;
  while (i < nq && j < ne) {
    if (q_ids[i] == e_ids[j]) {
      sum += kfdb_l1_term(q_vals[i], e_vals[j]);
      i++; j++;
    } else if (q_ids[i] < e_ids[j]) {
      i++;
    } else {
      j++;
    }
  }
  return kfdb_l1_finish(sum);
}

struct KfdbAcc {
  float acc, best;   // accScore, bestScore
  int best_slot;     // pBestKF
};
KFDB_HD void kfdb_acc_start(KfdbAcc& a, float si, int slot) { a.acc = si; a.best = si; a.best_slot = slot; }
KFDB_HD void kfdb_acc_neighbour(KfdbAcc& a, float s2, int slot2) {
  a.acc += s2;
  if (s2 > a.best) {
    a.best = s2;
    a.best_slot = slot2;
  }
}
KFDB_HD float kfdb_min_score_to_retain(float best_acc_score) { return 0.75f * best_acc_score; }

// one slot of the database: handed out in add order, never reused before clear
struct KfdbSlot {
  int64_t off;    // first word of the entry in the pooled CSR
  int64_t id;     // the keyframe id; -1 once erased
  int32_t len;    // words
  int32_t live;
};

struct KfdbLaunch {
  // the database
  const int32_t* ids; const double* vals;   // pooled CSR
  const KfdbSlot* slots;
  const int32_t* neigh;                     // [n_slots][KFDB_NEIGHBOURS] slot indices, -1: none / not live
  float* state;                             // [n_slots] the carried relocalisation score
  int n_slots;
  // the queries
  int Q, loop;
  int fused;                                // orbfe_debug_kfdb_arrangement: 1 = the common pass scores every pair (measured alternative)
  const int32_t* q_off; const int32_t* q_ids; const double* q_vals;   // CSR, [Q + 1]
  const float* min_score;                                               // [Q]         (loop)
  const int32_t* c_off; const int64_t* c_ids;                           // CSR, [Q + 1] (loop): connected ids, ascending
  // work space
  int32_t* words; int32_t* first; float* score; float* carried;         // [Q][n_slots]
  int32_t* sel[6];                                                      // [Q][n_slots] each: the selection's lists
  int32_t* qstat;                                                       // [Q][3]: n_sharing, maxCommonWords, minCommonWords
  // outputs
  int64_t* cand; int cand_cap; int32_t* n_cand; orbfe_kfdb_query_info* info;
  int32_t* o_words; float* o_scores;                                    // optional dense outputs, [Q][n_slots]
};

void orbfe_launch_kfdb_detect(const KfdbLaunch& L, hipStream_t s);
// score of one query against m listed slots (-1: unknown id, out = ORBFE_KFDB_SCORE_UNKNOWN)
void orbfe_launch_kfdb_score_list(const KfdbLaunch& L, const int32_t* d_list, int m, float* d_out, hipStream_t s);
