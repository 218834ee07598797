// Host-side helpers shared by the launchers.  Nothing here reads the environment or keeps per-kernel state: each launcher keeps
// its own first-call flag and derives its own grid from the CU count.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

namespace m355 {

// Opt a kernel in to `lds_bytes` of dynamic LDS (more than the 64 KiB default).  0, or the HIP error code.
inline int prepare_kernel(const void* fn, int lds_bytes) {
  return (int)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
}

// Compute units of the device, queried once per process.  <= 0: the query failed (the launchers return -2).
inline int num_cus() {
  static int cus = 0;
  if (cus <= 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
  }
  return cus;
}

// Device buffer of a kernel's diagnostic stamps and its way to a file (the M355_*_STAMPS switches).
struct StampSink {
  unsigned long long* d = nullptr;
  bool alloc(size_t bytes) {   // zeroed, once; false: the allocation failed
    if (d) return true;
    if (hipMalloc((void**)&d, bytes) != hipSuccess) return false;
    (void)hipMemset(d, 0, bytes);
    return true;
  }
  void write(const char* path, size_t nbytes) const {   // the first nbytes to `path`; the stream is synchronised already
    if (!path) return;
    std::vector<char> h(nbytes);
    (void)hipMemcpy(h.data(), d, nbytes, hipMemcpyDeviceToHost);
    FILE* f = fopen(path, "wb");
    if (f) { fwrite(h.data(), 1, nbytes, f); fclose(f); }
  }
  int dump(hipStream_t s, const char* path, size_t nbytes) const {   // after a launch: wait for it, then write().  0, or -2
    if (!path) return 0;
    if (hipStreamSynchronize(s) != hipSuccess) return -2;
    write(path, nbytes);
    return 0;
  }
};

}  // namespace m355
