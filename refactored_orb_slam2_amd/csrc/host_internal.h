// host_internal.h -- what the host side of the device back ends (pose.cpp, mapping.cpp, sim3.cpp, optsim3.cpp, matcher.cpp) shares:
// the error channel, the device check, and the staging of a one-problem host call.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>

#include "../../include/orbfe.h"

void orbfe_set_error(const char* fmt, ...);   // extractor.cpp
// the calling thread's matcher handle (matcher.cpp): its stream and a device block with a pinned mirror
int orbfe_internal_thread_block(size_t bytes, std::unique_lock<std::mutex>& lk, hipStream_t* s, uint8_t** dev, uint8_t** pinned);

inline bool have_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    orbfe_set_error("no HIP device available (liborbfe has no CPU fallback)");
    return false;
  }
  return true;
}

inline int hip_fail(const char* where, hipError_t e) {
  orbfe_set_error("%s: %s", where, hipGetErrorString(e));
  return ORBFE_ERR_HIP;
}

// offsets at 256-byte boundaries of one block
struct Layout {
  size_t off = 0;
  size_t add(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
};
