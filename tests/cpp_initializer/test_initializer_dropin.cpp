// test_initializer_dropin.cpp -- orbfe_host::Initializer (csrc/host/Initializer_hip.h) on the mock Frame: reads a problem, calls
// Initialize() `calls` times on one object and writes, per call, what it returned and the sets it drew, for
// tests/test_initializer_dropin_cpp.py to compare with the Python mirror.
//   in : fx fy cx cy sigma (f32), iterations calls n1 n2 (i32), keys1[n1][2], keys2[n2][2] (f32), matches12[n1] (i32)
//   out: per call: ok (i32), result record, sets[iterations][8] (i32), R21[9] t21[3] (f32), P3D[n1][3] (f32), triangulated[n1] (u8)
#include <stdio.h>

#include <vector>

#include "mock/Frame.h"
#include "../../refactored_orb_slam2_amd/csrc/host/Initializer_hip.h"

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T> static void wr(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  float cam[5];
  int32_t dims[4];
  if (!rd(f, cam, 5) || !rd(f, dims, 4)) return 2;
  const int iterations = dims[0], calls = dims[1], n1 = dims[2], n2 = dims[3];
  std::vector<float> k1((size_t)n1 * 2), k2((size_t)n2 * 2);
  std::vector<int32_t> m((size_t)n1);
  if (!rd(f, k1.data(), k1.size()) || !rd(f, k2.data(), k2.size()) || !rd(f, m.data(), m.size())) return 2;
  fclose(f);
  ORB_SLAM2::Frame ref, cur;
  ref.mK = cv::Mat::eye(3, 3, CV_32F);
  ref.mK.at<float>(0, 0) = cam[0]; ref.mK.at<float>(1, 1) = cam[1]; ref.mK.at<float>(0, 2) = cam[2]; ref.mK.at<float>(1, 2) = cam[3];
  cur.mK = ref.mK.clone();
  for (int i = 0; i < n1; i++) ref.mvKeysUn.push_back(cv::KeyPoint(k1[2 * i], k1[2 * i + 1], 31.f));
  for (int i = 0; i < n2; i++) cur.mvKeysUn.push_back(cv::KeyPoint(k2[2 * i], k2[2 * i + 1], 31.f));
  ORB_SLAM2::orbfe_host::Initializer<ORB_SLAM2::Frame> init(ref, cam[4], iterations);
  const std::vector<int> matches(m.begin(), m.end());
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  bool any_error = false;
  for (int c = 0; c < calls; c++) {
    cv::Mat R21, t21;
    std::vector<cv::Point3f> vP3D;
    std::vector<bool> vbTriangulated;
    const bool ok = init.Initialize(cur, matches, R21, t21, vP3D, vbTriangulated);
    const int32_t ok32 = ok;
    wr(o, &ok32, 1);
    wr(o, &init.Result(), 1);
    if (init.Sets().size() != (size_t)iterations * 8) { any_error = true; break; }
    wr(o, init.Sets().data(), init.Sets().size());
    float Rt[12] = {0};
    std::vector<float> p3d((size_t)n1 * 3, 0.f);
    std::vector<uint8_t> tri((size_t)n1, 0);
    if (ok) {
      for (int r = 0; r < 3; r++) {
        for (int cc = 0; cc < 3; cc++) Rt[3 * r + cc] = R21.at<float>(r, cc);
        Rt[9 + r] = t21.at<float>(r);
      }
      if ((int)vP3D.size() != n1 || (int)vbTriangulated.size() != n1) return 3;
      for (int i = 0; i < n1; i++) {
        p3d[3 * i] = vP3D[i].x; p3d[3 * i + 1] = vP3D[i].y; p3d[3 * i + 2] = vP3D[i].z;
        tri[i] = vbTriangulated[i];
      }
    } else if (!R21.empty() || !vP3D.empty()) {
      return 3;   // a failed call leaves the outputs alone
    }
    wr(o, Rt, 12);
    wr(o, p3d.data(), p3d.size());
    wr(o, tri.data(), tri.size());
  }
  fclose(o);
  return any_error ? 4 : 0;
}
