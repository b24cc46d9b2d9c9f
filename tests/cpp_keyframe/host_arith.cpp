// host_arith.cpp -- csrc/keyframe_internal.h compiled for the host, as a stand-alone program: the sequential reading of the keyframe
// decision and the close stereo points (kf_frame_sequential) over the calls that tests/np_keyframe.export_calls writes to a file,
// built with the address and undefined-behaviour sanitizers.  Every array is a heap block of exactly its size, so an index the rules
// fail to check is a report.
//   host_arith <calls> <answers>
// calls: see export_calls.  answers: per call headers [S], new_points [S][new_cap], new_index [S][new_cap], n_new [S], depth_selected
// [S][cap] and, with assigned, assigned [S][cap]; what the rules do not write holds the canary byte 0xA5.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/keyframe_internal.h"

namespace {

struct Reader {
  FILE* f;
  bool ok = true;
  int32_t one() {
    int32_t v = 0;
    if (fread(&v, 4, 1, f) != 1) ok = false;
    return v;
  }
  // a heap block of exactly n bytes (nullptr for none), 8-byte aligned as operator new gives it: the sanitizer sees one step beyond it
  std::unique_ptr<uint8_t[]> block(size_t n) {
    std::unique_ptr<uint8_t[]> p(n ? new uint8_t[n] : nullptr);
    if (n && fread(p.get(), 1, n, f) != n) ok = false;
    return p;
  }
};

std::unique_ptr<uint8_t[]> canary(size_t n) {
  std::unique_ptr<uint8_t[]> p(n ? new uint8_t[n] : nullptr);
  if (n) memset(p.get(), 0xA5, n);
  return p;
}

}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(orbfe_kf_header) == 64 && sizeof(orbfe_kf_decision_in) == 56 && sizeof(orbfe_kf_scales) == 72, "record sizes");
  static_assert(sizeof(orbfe_map_point) == 4 * KF_RECORD_DWORDS && sizeof(orbfe_kf_call) == 208, "record sizes");
  if (argc != 3) return 2;
  Reader in{fopen(argv[1], "rb")};
  FILE* out = fopen(argv[2], "wb");
  if (!in.f || !out) return 2;
  const int n_calls = in.one();
  for (int q = 0; q < n_calls && in.ok; q++) {
    const int S = in.one(), cap = in.one(), new_cap = in.one(), p_cap = in.one(), n_kf = in.one(), n_map_points = in.one(), mode = in.one(),
              flags = in.one(), with_outlier = in.one(), with_assigned = in.one(), observed_offset = in.one();
    in.one();
    KfLaunch L;
    memset(&L, 0, sizeof(L));
    if (fread(&L.cam, sizeof(L.cam), 1, in.f) != 1) break;
    const size_t rows = (size_t)S * cap;
    auto keys = in.block(rows * sizeof(orbfe_keypoint)), desc = in.block(rows * 32), depth = in.block(rows * 4), n = in.block((size_t)S * 4),
         cam = in.block((size_t)S * sizeof(orbfe_unproject_cam)), assigned = in.block(rows * 4),
         points = in.block((size_t)S * p_cap * sizeof(orbfe_map_point)), n_points = in.block((size_t)S * 4), outlier = in.block(rows),
         decision = in.block((size_t)S * sizeof(orbfe_kf_decision_in)), ref_kf = in.block((size_t)S * 4), base = in.block((size_t)S * 4),
         n_keys = in.block((size_t)n_kf * 4), state = in.block((size_t)n_kf * 4);
    std::vector<std::unique_ptr<uint8_t[]>> kf_slots;
    std::unique_ptr<orbfe_cov_keyframe[]> table(n_kf ? new orbfe_cov_keyframe[n_kf] : nullptr);
    for (int k = 0; k < n_kf && in.ok; k++) {
      const int len = in.one();
      kf_slots.push_back(in.block((size_t)len * 4));
      memset(&table[k], 0, sizeof(table[k]));
      table[k].n_keys = ((const int32_t*)n_keys.get())[k];
      const uint64_t at = (uint64_t)(uintptr_t)kf_slots.back().get();
      const int st = ((const int32_t*)state.get())[k];
      table[k].slots = (st == 1 || !len) ? 0 : st == 2 ? at + 2 : at;
    }
    auto point_bad = in.block((size_t)n_map_points), point_obs = in.block((size_t)n_map_points * 4);
    if (!in.ok) break;
    const size_t news = (size_t)S * new_cap;
    auto headers = canary((size_t)S * sizeof(orbfe_kf_header)), new_points = canary(news * sizeof(orbfe_map_point)), new_index = canary(news * 4),
         n_new = canary((size_t)S * 4), depth_selected = canary(rows * 4);
    orbfe_kf_call& C = L.C;
    C.keys_un = (const orbfe_keypoint*)keys.get(); C.desc = desc.get(); C.depth = (const float*)depth.get(); C.n = (const int32_t*)n.get();
    C.cam = (const orbfe_unproject_cam*)cam.get(); C.assigned = with_assigned ? (int32_t*)assigned.get() : nullptr; C.points = points.get();
    C.n_points = (const int32_t*)n_points.get(); C.outlier = with_outlier ? outlier.get() : nullptr;
    C.decision = (const orbfe_kf_decision_in*)decision.get(); C.ref_kf = ref_kf.get(); C.keyframes = table.get(); C.point_bad = point_bad.get();
    C.point_observations = (const int32_t*)point_obs.get(); C.n_points_base = (const int32_t*)base.get();
    C.headers = (orbfe_kf_header*)headers.get(); C.new_points = (orbfe_map_point*)new_points.get(); C.new_index = (int32_t*)new_index.get();
    C.n_new = (int32_t*)n_new.get(); C.depth_selected = (float*)depth_selected.get();
    C.S = S; C.cap = cap; C.new_cap = new_cap; C.p_cap = p_cap; C.frame_shift = 0; C.point_stride = (int32_t)sizeof(orbfe_map_point);
    C.observed_offset = observed_offset; C.ref_kf_stride = 4; C.n_kf = n_kf; C.n_map_points = n_map_points; C.mode = mode; C.flags = flags;
    std::unique_ptr<uint64_t[]> sort_keys(new uint64_t[cap]);
    std::unique_ptr<uint32_t[]> mark(new uint32_t[(cap + 31) / 32]);
    for (int f = 0; f < S; f++) kf_frame_sequential(L, f, sort_keys.get(), mark.get());
    fwrite(headers.get(), 1, (size_t)S * sizeof(orbfe_kf_header), out);
    fwrite(new_points.get(), 1, news * sizeof(orbfe_map_point), out);
    fwrite(new_index.get(), 1, news * 4, out);
    fwrite(n_new.get(), 1, (size_t)S * 4, out);
    fwrite(depth_selected.get(), 1, rows * 4, out);
    if (with_assigned) fwrite(assigned.get(), 1, rows * 4, out);
  }
  fclose(in.f);
  if (fclose(out) != 0 || !in.ok) return 1;
  printf("keyframe host arithmetic: %d calls\n", n_calls);
  return 0;
}
