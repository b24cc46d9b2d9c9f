// host_arith.cpp -- csrc/localmap_internal.h compiled for the host, as a stand-alone program: the sequential reading of the local map
// (lm_local_map_sequential) over problems that tests/test_localmap_cpu.py writes to a file, built with the address and
// undefined-behaviour sanitizers.  Every table is a heap block of exactly its size, so an index the rules fail to check is a report.
//   host_arith <problems> <answers>
// Both files are streams of little-endian int32.  problems: count, then per problem S, conn_cap, kf_cap, p_cap, n_kf, n_points,
// n_children, n_frame_slots, n_seen, with_records and the tables in the order read below.  answers: per problem headers [S][8],
// local_kf [S][kf_cap], local_points [S][p_cap], n_points [S] and, with records, map_points [S][p_cap][18]; what the rules do not
// write holds the canary 0x5C5C5C5C.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/localmap_internal.h"

namespace {

const int32_t CANARY = 0x5C5C5C5C;

struct Reader {
  FILE* f;
  bool ok = true;
  int32_t one() {
    int32_t v = 0;
    if (fread(&v, 4, 1, f) != 1) ok = false;
    return v;
  }
  // a heap block of exactly n values (nullptr for none): the sanitizer sees one step beyond it
  std::unique_ptr<int32_t[]> block(size_t n) {
    std::unique_ptr<int32_t[]> p(n ? new int32_t[n] : nullptr);
    if (n && fread(p.get(), 4, n, f) != n) ok = false;
    return p;
  }
  std::unique_ptr<uint8_t[]> bytes(size_t n) {   // stored as int32 each
    std::unique_ptr<uint8_t[]> p(n ? new uint8_t[n] : nullptr);
    for (size_t i = 0; i < n; i++) p[i] = (uint8_t)one();
    return p;
  }
};

void put(FILE* f, const void* p, size_t n_words) {
  if (n_words) fwrite(p, 4, n_words, f);
}

}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(orbfe_lm_graph) == 56 && sizeof(orbfe_lm_frame) == 8 && sizeof(orbfe_lm_header) == 32, "record sizes");
  static_assert(sizeof(orbfe_map_point) == 4 * LM_RECORD_DWORDS && offsetof(orbfe_map_point, skip) == 4 * LM_SKIP_DWORD, "map point");
  if (argc != 3) return 2;
  Reader in{fopen(argv[1], "rb")};
  FILE* out = fopen(argv[2], "wb");
  if (!in.f || !out) return 2;
  const int n_problems = in.one();
  for (int q = 0; q < n_problems && in.ok; q++) {
    const int S = in.one(), conn_cap = in.one(), kf_cap = in.one(), p_cap = in.one(), n_kf = in.one(), n_points = in.one(),
              n_children = in.one(), n_frame_slots = in.one(), n_seen = in.one(), with_records = in.one();
    auto votes = in.block((size_t)S * 8), entries = in.block((size_t)S * conn_cap * 2), graph = in.block((size_t)n_kf * 14),
         children = in.block((size_t)n_children);
    auto kf_bad = in.bytes((size_t)n_kf), point_bad = in.bytes((size_t)n_points);
    auto n_keys = in.block((size_t)n_kf), state = in.block((size_t)n_kf);
    std::vector<std::unique_ptr<int32_t[]>> kf_slots;
    std::unique_ptr<orbfe_cov_keyframe[]> table(n_kf ? new orbfe_cov_keyframe[n_kf] : nullptr);
    for (int k = 0; k < n_kf && in.ok; k++) {
      const int len = in.one();
      kf_slots.push_back(in.block((size_t)len));
      memset(&table[k], 0, sizeof(table[k]));
      table[k].n_keys = n_keys[k];
      const uint64_t at = (uint64_t)(uintptr_t)kf_slots.back().get();
      table[k].slots = state[k] == 1 ? 0 : state[k] == 2 ? at + 2 : at;
    }
    auto frame_slots = in.block((size_t)n_frame_slots), subjects = in.block((size_t)S * 4), seen = in.block((size_t)n_seen),
         frames = in.block((size_t)S * 2), records = in.block(with_records ? (size_t)n_points * LM_RECORD_DWORDS : 0);
    if (!in.ok) break;

    LmTables T;
    T.graph = (const orbfe_lm_graph*)graph.get(); T.children = children.get(); T.n_children_total = n_children;
    T.kfs = table.get(); T.kf_bad = kf_bad.get(); T.n_kf = n_kf; T.point_bad = point_bad.get(); T.n_points = n_points;
    T.slots = frame_slots.get(); T.n_slots_total = n_frame_slots; T.seen = seen.get(); T.n_seen_total = n_seen;
    std::vector<int32_t> headers((size_t)S * 8, CANARY), local_kf((size_t)S * kf_cap, CANARY), local_points((size_t)S * p_cap, CANARY),
        n_out((size_t)S, CANARY), map_points(with_records ? (size_t)S * p_cap * LM_RECORD_DWORDS : 0, CANARY);
    std::vector<int32_t> list(LM_LIST_MAX);
    std::vector<uint32_t> kf_marked((size_t)(n_kf + 31) / 32), p_marked((size_t)(n_points + 31) / 32);
    for (int s = 0; s < S; s++) {
      std::fill(kf_marked.begin(), kf_marked.end(), 0u);
      std::fill(p_marked.begin(), p_marked.end(), 0u);
      lm_local_map_sequential(T, ((const orbfe_cov_header*)votes.get())[s], (const orbfe_cov_entry*)entries.get() + (size_t)s * conn_cap,
                              conn_cap, ((const orbfe_cov_subject*)subjects.get())[s], (const orbfe_lm_frame*)frames.get() + s,
                              (const orbfe_map_point*)records.get(), kf_cap, p_cap, list.data(), kf_marked.data(), p_marked.data(),
                              ((orbfe_lm_header*)headers.data())[s], local_kf.data() + (size_t)s * kf_cap,
                              local_points.data() + (size_t)s * p_cap, n_out.data() + s,
                              with_records ? (orbfe_map_point*)map_points.data() + (size_t)s * p_cap : nullptr);
    }
    put(out, headers.data(), headers.size());
    put(out, local_kf.data(), local_kf.size());
    put(out, local_points.data(), local_points.size());
    put(out, n_out.data(), n_out.size());
    put(out, map_points.data(), map_points.size());
  }
  fclose(in.f);
  if (fclose(out) != 0 || !in.ok) return 1;
  printf("local map host arithmetic: %d problems\n", n_problems);
  return 0;
}
