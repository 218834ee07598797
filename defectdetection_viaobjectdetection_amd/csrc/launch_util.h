// Host-side helpers shared by the launchers.  Nothing here reads the environment, and the only per-kernel state is the stamp buffer
// of launch_stamped: each launcher keeps its own first-call flag and derives its own grid from the CU count.
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

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }   // nullptr counts as aligned

// lanes of a wave that share a row of `units` loads: the power of two >= units, 64 at the most
inline int lanes_per_row(int units) {
  int L = 1;
  while (L < units && L < 64) L <<= 1;
  return L;
}

// Device buffer of a probe instance's stamps and its way to a file (the M355_*_STAMPS switches).
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

// The launch of a kernel whose stamps go to a file named by a process-lifetime switch (M355_C2F_STAMPS and its like).  `launch(st)`
// starts the kernel with the stamp buffer st (nullptr: none, the production instance unless an ablation asks for the probe one).
// With `path` set the buffer (cap bytes, one per call site: the lambda's type is the key) is allocated and zeroed on first use, the
// stream is waited for and the first n bytes go to `path`.  0, a HIP error code, or -2.
template <class Launch>
int launch_stamped(const char* path, size_t cap, size_t n, hipStream_t s, Launch launch) {
  static StampSink sink;
  if (path && !sink.alloc(cap)) return -2;
  launch(path ? sink.d : nullptr);
  if (sink.dump(s, path, n)) return -2;
  return (int)hipGetLastError();
}

}  // namespace m355
