// host_internal.h -- what the host side of the device back ends shares: the error channel and the device check (every .cpp with a
// C ABI), and HostCall, the staging of a one-problem host call on the calling thread's matcher handle (pose.cpp, mapping.cpp,
// sim3.cpp, optsim3.cpp, lba.cpp, mappoint.cpp, covis.cpp, matcher.cpp; its body is in matcher.cpp, where that handle lives).
// With HOST_LAYOUT_ONLY defined only the region arithmetic is declared, which needs no HIP header or runtime.
#pragma once
#include <assert.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

// offsets at 256-byte boundaries of one block
struct Layout {
  size_t off = 0;
  size_t add(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
};

// The regions of a one-problem host call, declared in three groups in this order: input (uploaded), scratch (device only), output
// (downloaded).  Every declaration returns the region's offset, the same in the device block and in its pinned host mirror.
struct HostLayout {
  size_t in(size_t bytes) { return add(0, bytes); }
  size_t scratch(size_t bytes) { return add(1, bytes); }
  size_t out(size_t bytes) { return add(2, bytes); }
  size_t in_end() const { return end[0]; }
  size_t out_begin() const { return end[1]; }
  size_t total() const { return L.off; }
  size_t out_bytes() const { return L.off - end[1]; }   // the whole output group

 private:
  size_t add(int g, size_t bytes) {
    assert(g >= group && "regions are declared input, then scratch, then output");
    group = g;
    const size_t o = L.add(bytes);
    for (int i = g; i < 2; i++) end[i] = L.off;
    return o;
  }
  Layout L;
  size_t end[2] = {0, 0};   // of the input group, of the scratch group
  int group = 0;
};

// The iteration count of SetRansacParameters (Sim3Solver.cc:112-136, PnPsolver.cc:119-151), for minimal sets of three or four alike
// (both files raise epsilon to the third power): 1 when every correspondence must be an inlier, else
// ceil(log(1 - probability) / log(1 - epsilon^3)), clamped to 1 .. max_iterations.  pow(float, int) is double.  epsilon == 0 gives
// log(1) == 0 and a quotient of -inf, epsilon >= 1 gives log(<= 0): the int conversion of the reference without its overflow -- below 1
// (or NaN) the max() underneath decides, above max_iterations the min().
inline int ransac_iterations(bool all_inliers, double probability, float epsilon, int max_iterations) {
  int n_iterations = 1;
  if (!all_inliers) {
    const double v = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
    n_iterations = !(v >= 1.0) ? 1 : (v >= (double)max_iterations ? max_iterations : (int)v);
  }
  return std::max(1, std::min(n_iterations, max_iterations));
}

#ifndef HOST_LAYOUT_ONLY
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/orbfe.h"

void orbfe_set_error(const char* fmt, ...);   // extractor.cpp

inline bool have_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    orbfe_set_error("no HIP device available (liborbfe has no CPU fallback)");
    return false;
  }
  return true;
}

// the one place a HIP status becomes the library's: ORBFE_OK, or the error text keyed by `where` and ORBFE_ERR_HIP
inline int hip_status(const char* where, hipError_t e) {
  if (e == hipSuccess) return ORBFE_OK;
  orbfe_set_error("%s: %s", where, hipGetErrorString(e));
  return ORBFE_ERR_HIP;
}

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      orbfe_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return ORBFE_ERR_HIP;                                                                       \
    }                                                                                             \
  } while (0)

struct orbfe_matcher;
enum HostDownload { HOST_DMA, HOST_COPY_KERNEL };   // hipMemcpyAsync, or the four-workgroup copy kernel of pipeline_kernels.hip

// The whole life of a one-problem host call: declare the regions, open(), fill host(off) of the input group, upload(), launch on
// `stream` with dev(off) pointers, finish(), read host(off) of the output group.  Between upload() and the end of finish() the
// stream works on the pinned block; the destructor waits for it on every other way out, before the handle's lock is released.
class HostCall : public HostLayout {
 public:
  explicit HostCall(const char* where) : where(where) {}
  ~HostCall();
  HostCall(const HostCall&) = delete;
  HostCall& operator=(const HostCall&) = delete;

  int open();                                  // the calling thread's handle, locked, its device selected, both blocks >= total()
  int upload(bool through_output = false);     // ONE copy of the input group; of the whole block where output regions are read too
  int finish(size_t bytes, HostDownload how = HOST_DMA);       // launch check, ONE copy of the output group's head, wait
  int status(hipError_t e) const { return hip_status(where, e); }
  template <class T = uint8_t> T* dev(size_t off) const { return reinterpret_cast<T*>(d + off); }
  template <class T = uint8_t> T* host(size_t off) const { return reinterpret_cast<T*>(h + off); }

  hipStream_t stream = nullptr;
  orbfe_matcher* m = nullptr;   // the handle, for its device scratch (matcher.cpp)

 private:
  const char* where;
  std::unique_lock<std::mutex> lk;
  uint8_t *d = nullptr, *h = nullptr;
  bool in_flight = false;
};
#endif
