// plan_check.cpp -- csrc/search_plan.h compiled for the host as a stand-alone program (address and undefined-behaviour sanitizers, no
// device): reads FeatureVector pairs from the file named on the command line and prints, per case, what the plan functions decide.
// tests/test_nodesearch_cpu.py writes the cases (the FeatureVectors of the scenes of tests/np_nodesearch.py and malformed ones) and
// compares the lines with what the instrumented walks need.
//
// input, whitespace separated, per case:
//   name  mode(0 SearchByBoW KF-Frame, 1 SearchByBoW KF-KF, 2 SearchForTriangulation)  nA nB  n_nodesA n_nodesB  len_idxA len_idxB
//   n_nodesA x (node_id start count)   len_idxA x index   n_nodesB x (node_id start count)   len_idxB x index
// output per case:
//   name rc=<code> pairs=<n> sequential=<0|1> push_cap=<n> maxB=<n> totA=<n> totB=<n> : startA,countA,startB,countB; ...
#include <cstdio>
#include <string>
#include <vector>

#include "search_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: plan_check <cases file>\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  char name[256];
  int n_cases = 0;
  while (fscanf(f, "%255s", name) == 1) {
    int mode, nA, nB, nnA, nnB, lA, lB;
    if (fscanf(f, "%d %d %d %d %d %d %d", &mode, &nA, &nB, &nnA, &nnB, &lA, &lB) != 7 || nnA < 0 || nnB < 0 || lA < 0 || lB < 0) {
      fprintf(stderr, "bad header of case %s\n", name);
      return 2;
    }
    std::vector<orbfe_featvec_node> nodesA((size_t)nnA), nodesB((size_t)nnB);
    std::vector<int32_t> idxA((size_t)lA), idxB((size_t)lB);   // exactly as long as stated: a read past the end is an ASan report
    bool ok = true;
    for (auto& n : nodesA) ok = ok && fscanf(f, "%d %d %d", &n.node_id, &n.start, &n.count) == 3;
    for (auto& v : idxA) ok = ok && fscanf(f, "%d", &v) == 1;
    for (auto& n : nodesB) ok = ok && fscanf(f, "%d %d %d", &n.node_id, &n.start, &n.count) == 3;
    for (auto& v : idxB) ok = ok && fscanf(f, "%d", &v) == 1;
    if (!ok) { fprintf(stderr, "truncated case %s\n", name); return 2; }
    TriSearchPlan plan;
    const int rc = mode == 2 ? orbfe_tri_search_plan(nA, nodesA.data(), nnA, idxA.data(), nB, nodesB.data(), nnB, idxB.data(), plan)
                             : orbfe_bow_search_plan(nA, nodesA.data(), nnA, idxA.data(), nB, nodesB.data(), nnB, idxB.data(), mode, plan);
    printf("%s rc=%d pairs=%zu sequential=%d push_cap=%d maxB=%d totA=%d totB=%d :", name, rc, plan.pairs.size(), plan.sequential,
           plan.push_cap, plan.maxB, plan.totA, plan.totB);
    for (const BowPair& p : plan.pairs) printf(" %d,%d,%d,%d;", p.startA, p.countA, p.startB, p.countB);
    printf("\n");
    n_cases++;
  }
  fclose(f);
  printf("cases=%d\n", n_cases);
  return 0;
}
