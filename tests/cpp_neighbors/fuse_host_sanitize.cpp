// fuse_host_sanitize.cpp -- the host-side validation and staging code of csrc/fuse.cpp under AddressSanitizer and UBSan, as a stand-alone
// program for a machine WITHOUT a device: `make sanitize` compiles fuse.cpp itself with -fsanitize=address,undefined, links it with
// this main (which stands in for the error channel and the kernel launchers), and runs it.  Every orbfe_fuse_batch_* entry point is
// driven through each refusal and, with good arguments, up to the missing device; the staging arithmetic is run on real buffers.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../refactored_orb_slam2_amd/csrc/fuse_internal.h"

static char g_err[512];
void orbfe_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
void orbfe_launch_grid_build(const FrameBatch&, int, hipStream_t) { abort(); }   // never reached without a device
void orbfe_launch_fuse_rows(const FuseRows&, hipStream_t) { abort(); }
void orbfe_launch_fuse_scatter(orbfe_kf_point*, int, const orbfe_kf_point*, const int32_t*, int, hipStream_t) { abort(); }

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, g_err); return 1; } } while (0)

int main() {
  const int K = 3, n = 5;
  std::vector<orbfe_keypoint> keys(4);
  std::vector<uint8_t> desc(4 * 32);
  std::vector<orbfe_frame_view> tv(K);
  std::vector<orbfe_kf_camera> cams(K);
  std::vector<float> inv(K * ORBFE_MAX_LEVELS, 1.f);
  memset(cams.data(), 0, sizeof(orbfe_kf_camera) * K);
  for (int k = 0; k < K; k++) {
    tv[k] = orbfe_frame_view{k == 1 ? 0 : 4, k == 1 ? nullptr : keys.data(), k == 1 ? nullptr : desc.data(), nullptr, 0.f, 640.f, 0.f, 480.f};
    cams[k].n_levels = k == 2 ? ORBFE_MAX_LEVELS : 1;
  }
  int cap = 0;
  CHECK(orbfe_fuse_validate_targets(K, tv.data(), cams.data(), inv.data(), ORBFE_KF_FUSE, &cap) == ORBFE_OK && cap == 4);
  orbfe_fuse_batch* h = nullptr;
  // good arguments end at the missing device; nothing was allocated
  CHECK(orbfe_fuse_batch_create(K, tv.data(), cams.data(), inv.data(), ORBFE_KF_FUSE, &h) == ORBFE_ERR_NO_DEVICE && !h);
  CHECK(orbfe_fuse_batch_create(0, nullptr, nullptr, nullptr, ORBFE_KF_FUSE_SIM3, &h) == ORBFE_ERR_NO_DEVICE && !h);
  // refusals
  CHECK(orbfe_fuse_batch_create(-1, tv.data(), cams.data(), inv.data(), ORBFE_KF_FUSE, &h) == ORBFE_ERR_INVALID);
  CHECK(orbfe_fuse_batch_create(K, tv.data(), cams.data(), nullptr, ORBFE_KF_FUSE, &h) == ORBFE_ERR_INVALID);
  CHECK(orbfe_fuse_batch_create(K, tv.data(), cams.data(), inv.data(), ORBFE_KF_SIM3, &h) == ORBFE_ERR_INVALID);
  CHECK(orbfe_fuse_batch_create(K, tv.data(), cams.data(), inv.data(), ORBFE_KF_FUSE, nullptr) == ORBFE_ERR_INVALID);
  cams[0].n_levels = ORBFE_MAX_LEVELS + 1;
  CHECK(orbfe_fuse_batch_create(K, tv.data(), cams.data(), inv.data(), ORBFE_KF_FUSE, &h) == ORBFE_ERR_INVALID);
  cams[0].n_levels = 0;
  CHECK(orbfe_fuse_batch_create(K, tv.data(), cams.data(), inv.data(), ORBFE_KF_FUSE, &h) == ORBFE_ERR_INVALID);
  cams[0].n_levels = 8;
  tv[2].n = 65536;
  CHECK(orbfe_fuse_batch_create(K, tv.data(), cams.data(), inv.data(), ORBFE_KF_FUSE, &h) == ORBFE_ERR_INVALID);   // before the arrays are read
  tv[2].n = 4;
  tv[2].max_x = 641.f;
  CHECK(orbfe_fuse_batch_create(K, tv.data(), cams.data(), inv.data(), ORBFE_KF_FUSE, &h) == ORBFE_ERR_NO_DEVICE);   // bounds of its own
  tv[2].max_x = 640.f;
  tv[2].max_x = 0.f;
  CHECK(orbfe_fuse_batch_create(K, tv.data(), cams.data(), inv.data(), ORBFE_KF_FUSE, &h) == ORBFE_ERR_INVALID);      // empty bounds
  tv[2].max_x = 640.f;
  // K x n_points within int32_t: the last accepted and the first refused values
  CHECK(orbfe_fuse_validate_rows(1, INT32_MAX) == ORBFE_OK && orbfe_fuse_validate_rows(2, 1073741823) == ORBFE_OK);
  CHECK(orbfe_fuse_validate_rows(2, 1073741824) == ORBFE_ERR_INVALID && orbfe_fuse_validate_rows(3, 715827883) == ORBFE_ERR_INVALID);
  CHECK(orbfe_fuse_validate_rows(3, 715827882) == ORBFE_OK && orbfe_fuse_validate_rows(0, INT32_MAX) == ORBFE_OK);
  CHECK(orbfe_fuse_batch_create_device(1, keys.data(), desc.data(), nullptr, nullptr, 4, 0, 640, 0, 480, cams.data(), inv.data(), ORBFE_KF_FUSE,
                                       nullptr, &h) == ORBFE_ERR_INVALID);
  CHECK(orbfe_fuse_batch_create_device(1, keys.data(), desc.data(), nullptr, (const int32_t*)keys.data(), 65536, 0, 640, 0, 480, cams.data(),
                                       inv.data(), ORBFE_KF_FUSE, nullptr, &h) == ORBFE_ERR_INVALID);
  CHECK(orbfe_fuse_batch_search(nullptr, nullptr, 0, nullptr, 0, 0, nullptr, nullptr) == ORBFE_ERR_INVALID);
  CHECK(orbfe_fuse_batch_search_device(nullptr, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nullptr) == ORBFE_ERR_INVALID);
  CHECK(orbfe_fuse_batch_destroy(nullptr) == ORBFE_OK);
  // the index list: last accepted and first refused values
  const int32_t good[3] = {0, 2, n - 1}, dup[2] = {2, 2}, down[2] = {3, 2}, high[1] = {n}, neg[1] = {-1};
  CHECK(orbfe_fuse_validate_index(good, 3, n) == ORBFE_OK && orbfe_fuse_validate_index(good, 0, n) == ORBFE_OK);
  CHECK(orbfe_fuse_validate_index(dup, 2, n) == ORBFE_ERR_INVALID && orbfe_fuse_validate_index(down, 2, n) == ORBFE_ERR_INVALID);
  CHECK(orbfe_fuse_validate_index(high, 1, n) == ORBFE_ERR_INVALID && orbfe_fuse_validate_index(neg, 1, n) == ORBFE_ERR_INVALID);
  // the staging block and the scatter of its rows into the caller's array, full and partial, every first_target
  for (int partial = 0; partial < 2; partial++)
    for (int first = 0; first <= K; first++) {
      const int n_rec = partial ? 3 : n;
      const FuseStage st = orbfe_fuse_stage_layout(K, n, n_rec, partial != 0, true, first);
      CHECK(st.o_pts == 0 && st.o_idx >= sizeof(orbfe_kf_point) * n_rec && st.o_skip >= st.o_idx && st.o_res >= st.o_skip + (size_t)K * n);
      CHECK(st.total >= st.o_res + sizeof(orbfe_kf_result) * (size_t)(K - first) * n_rec && st.total % 256 == 0);
      std::vector<uint8_t> block(st.total, 0);
      orbfe_kf_result* staged = (orbfe_kf_result*)(block.data() + st.o_res);
      for (int r = 0; r < (K - first) * n_rec; r++) staged[r].best_idx = 1000 + r;
      std::vector<orbfe_kf_result> results((size_t)K * n);
      memset(results.data(), 0xAB, sizeof(orbfe_kf_result) * results.size());
      orbfe_fuse_unstage_results(staged, K, n, partial ? good : nullptr, n_rec, first, results.data());
      int written = 0;
      for (int k = 0; k < K; k++)
        for (int i = 0; i < n; i++) {
          const bool sel = k >= first && (!partial || i == good[0] || i == good[1] || i == good[2]);
          const orbfe_kf_result& r = results[(size_t)k * n + i];
          if (sel) {
            written++;
            CHECK(r.best_idx >= 1000 && r.best_idx < 1000 + (K - first) * n_rec);
          } else {
            CHECK((uint32_t)r.best_idx == 0xABABABABu && (uint32_t)r.level == 0xABABABABu);
          }
        }
      CHECK(written == (K - first) * n_rec);
    }
  printf("fuse host code: clean\n");
  return 0;
}
