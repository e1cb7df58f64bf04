// tests/checklib/device_pool.h -- TEST-ONLY: device copies of host arrays for the
// *check_device exports, freed together.  The first HIP error sticks in `e` and turns
// every later call into a no-op, so a caller checks it once after its uploads and once
// after its downloads.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace checklib {

struct Pool {
  std::vector<void *> p;
  hipError_t e = hipSuccess;
  // a device buffer of `bytes` (and some slack), filled from `host` unless that is null
  void *put(const void *host, size_t bytes) {
    void *q = nullptr;
    if (e == hipSuccess) e = hipMalloc(&q, bytes + 16);
    if (e == hipSuccess && bytes && host) e = hipMemcpy(q, host, bytes, hipMemcpyHostToDevice);
    p.push_back(q);
    return q;
  }
  // skipped for a null host pointer (an optional output)
  void get(void *host, const void *dev, size_t bytes) {
    if (e == hipSuccess && bytes && host) e = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
  }
  ~Pool() {
    for (void *q : p) (void)hipFree(q);
  }
};

}  // namespace checklib
