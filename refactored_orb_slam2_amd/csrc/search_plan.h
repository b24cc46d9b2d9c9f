// search_plan.h -- the host half of the searches over common vocabulary nodes in front of the upload: the merge-join of the two
// FeatureVectors on NodeId, the checks that keep a malformed one from indexing past the arrays on the device, the choice between one
// wave per node and the sequential replay, and the capacity of the rotation scratch.  Plain C++ on include/orbfe.h alone, so that
// tests/cpp_nodesearch compiles it for the host without a device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/orbfe.h"

#define ORBFE_NODE_MAX_B 60000   // entries of one node's second-side list (bow_match_kernel keeps a byte of LDS per entry)

struct BowPair { int32_t startA, countA, startB, countB; };

struct TriSearchPlan {
  std::vector<BowPair> pairs;   // the common vocabulary nodes
  int totA = 0, totB = 0;       // entries of the two index arrays
  int sequential = 0;           // the nodes are not independent: one wave walks every pair in NodeId order
  int maxB = 0;                 // the longest second-side list among the pairs
  int push_cap = 0;             // entries of the rotation scratch: max(nA, totA, visits), a visit being one entry of a pair's first-side list
};
typedef TriSearchPlan BowSearchPlan;

// dup_a / dup_b: whether a feature listed twice on that side couples the nodes (replay in order)
inline int orbfe_node_search_plan(int nA, const orbfe_featvec_node* nodesA, int n_nodesA, const int32_t* idxA, int nB,
                                  const orbfe_featvec_node* nodesB, int n_nodesB, const int32_t* idxB, bool dup_a, bool dup_b,
                                  TriSearchPlan& plan) {
  plan.pairs.clear();
  plan.totA = plan.totB = plan.sequential = plan.maxB = 0;
  plan.push_cap = nA;
  int ia = 0, ib = 0;
  // merge-join on NodeId (L/src/ORBmatcher.cc:183-253; lower_bound jumps == plain two-pointer walk on sorted ids)
  while (ia < n_nodesA && ib < n_nodesB) {
    if (nodesA[ia].node_id == nodesB[ib].node_id) {
      plan.pairs.push_back(BowPair{nodesA[ia].start, nodesA[ia].count, nodesB[ib].start, nodesB[ib].count});
      plan.maxB = std::max(plan.maxB, nodesB[ib].count);
      ia++; ib++;
    } else if (nodesA[ia].node_id < nodesB[ib].node_id) ia++;
    else ib++;
  }
  if (plan.maxB > ORBFE_NODE_MAX_B) return ORBFE_ERR_INVALID;
  for (int i = 0; i < n_nodesA; i++) plan.totA = std::max(plan.totA, nodesA[i].start + nodesA[i].count);
  for (int i = 0; i < n_nodesB; i++) plan.totB = std::max(plan.totB, nodesB[i].start + nodesB[i].count);
  plan.push_cap = std::max(plan.totA, nA);
  if (plan.pairs.empty()) return ORBFE_OK;
  // The reference visits a first-side feature once per entry of a common node's list, and every visit can push a rotation entry.
  // The visits are counted as well, not only read off the index array's length: nothing keeps two nodes from naming overlapping
  // ranges of it, and then there are more visits than entries.
  long long visits = 0;
  std::vector<uint8_t> seenA((size_t)nA, 0), seenB((size_t)nB, 0);
  for (const BowPair& pr : plan.pairs) {
    if (pr.startA < 0 || pr.countA < 0 || pr.startB < 0 || pr.countB < 0 || pr.startA > INT32_MAX - pr.countA ||
        pr.startB > INT32_MAX - pr.countB)
      return ORBFE_ERR_INVALID;
    visits += pr.countA;
    if (visits > INT32_MAX) return ORBFE_ERR_INVALID;
    plan.push_cap = std::max(plan.push_cap, (int)visits);
    for (int t = 0; t < pr.countA; t++) {
      const int j = idxA[pr.startA + t];
      if (j < 0 || j >= nA) return ORBFE_ERR_INVALID;
      if (seenA[j] && dup_a) plan.sequential = 1;
      seenA[j] = 1;
    }
    for (int t = 0; t < pr.countB; t++) {
      const int j = idxB[pr.startB + t];
      if (j < 0 || j >= nB) return ORBFE_ERR_INVALID;
      if (seenB[j] && dup_b) plan.sequential = 1;
      seenB[j] = 1;
    }
  }
  return ORBFE_OK;
}

// SearchForTriangulation: nothing couples two second-side features (vbMatched2 is never set), but a pKF1 feature listed under two
// nodes (never produced by DBoW2) is visited twice by the reference and the later visit overwrites vMatches12: replay in order.
inline int orbfe_tri_search_plan(int nA, const orbfe_featvec_node* nodesA, int n_nodesA, const int32_t* idxA, int nB,
                                 const orbfe_featvec_node* nodesB, int n_nodesB, const int32_t* idxB, TriSearchPlan& plan) {
  return orbfe_node_search_plan(nA, nodesA, n_nodesA, idxA, nB, nodesB, n_nodesB, idxB, true, false, plan);
}

// The two SearchByBoW forms.  A second-side feature listed twice couples its nodes through the match table in both forms.  In the
// KF-KF form a first-side feature listed under two common nodes has vpMatches12[idx1] written once per node, the later node winning,
// so the nodes must be walked in order as well; in the KF-Frame form the result is indexed by the frame feature and a repeated
// keyframe feature couples nothing.
inline int orbfe_bow_search_plan(int nA, const orbfe_featvec_node* nodesA, int n_nodesA, const int32_t* idxA, int nB,
                                 const orbfe_featvec_node* nodesB, int n_nodesB, const int32_t* idxB, int kf_mode, BowSearchPlan& plan) {
  return orbfe_node_search_plan(nA, nodesA, n_nodesA, idxA, nB, nodesB, n_nodesB, idxB, kf_mode != 0, true, plan);
}
