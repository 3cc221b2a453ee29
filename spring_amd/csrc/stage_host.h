// spring_amd/csrc/stage_host.h -- the host-side frame that every stage context shares: the HIP
// error check, pooled device buffers, launch grids, event holders and the device / stream set-up of a context.  Host
// code only; a stage writes its kernels, its context struct, its drop_result / destroy and its entry points itself.
// Internal to the library.
#ifndef SPRING_STAGE_HOST_H_
#define SPRING_STAGE_HOST_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "reorder_internal.h"

// A macro, so that the file and the line are the caller's.  Needs `fail` in scope (using sr::fail, or namespace sr).
#define HIPCHK(x)                                                                              \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess)                                                                      \
      return fail(SPRING_REORDER_E_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

namespace sr {

// A device buffer from the library's pool (dev_alloc hands out at least 16 bytes, so a size of 0 is fine).
struct DBuf {
  int dev = 0;
  void *p = nullptr;
  DBuf() = default;
  DBuf(const DBuf &) = delete;
  DBuf &operator=(const DBuf &) = delete;
  ~DBuf() { release(); }
  void release() { if (p) { dev_free(dev, p); p = nullptr; } }
  hipError_t alloc(int d, size_t bytes) { release(); dev = d; return dev_alloc(d, bytes, &p); }
  template <class T> T *as() const { return (T *)p; }
};
// Needs `dev` in scope.
#define DALLOC(buf, bytes) HIPCHK((buf).alloc(dev, (bytes)))

// Blocks for n items; never zero, so a launch over nothing is still a valid launch.
inline dim3 grid(uint64_t n, uint32_t per_block = 256) {
  const uint64_t b = (n + per_block - 1) / per_block;
  return dim3((unsigned)(b ? b : 1));
}

// Device to host, done when it returns.
inline hipError_t rd(hipStream_t st, void *dst, const void *src, size_t n) {
  hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// Up to eight events, destroyed with the holder; a and b name the first two for a function that times one span.
struct Events {
  hipEvent_t e[8] = {};
  hipEvent_t &a = e[0], &b = e[1];
  ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

// What one run of a driver allocates on the host side: any number of events, each with its own creation flags, and pinned
// buffers.  All of it goes with the holder.
struct RunOwned {
  std::vector<hipEvent_t> events;
  std::vector<void *> pinned;
  RunOwned() = default;
  RunOwned(const RunOwned &) = delete;
  RunOwned &operator=(const RunOwned &) = delete;
  ~RunOwned() {
    for (auto e : events) (void)hipEventDestroy(e);
    for (auto p : pinned) (void)hipHostFree(p);
  }
  hipError_t event(hipEvent_t *e, unsigned flags = hipEventDefault) {
    const hipError_t r = hipEventCreateWithFlags(e, flags);
    if (r == hipSuccess) events.push_back(*e);
    return r;
  }
  template <class T> hipError_t pin(T **p, size_t bytes) {
    const hipError_t r = hipHostMalloc((void **)p, bytes, hipHostMallocDefault);
    if (r == hipSuccess) pinned.push_back(*p);
    return r;
  }
};

// Timed spans on one stream, each counted towards a pass of the stage's info.  The events live as long as the holder:
// declare it in front of the function's SyncOnExit, so that no span is in flight when they are destroyed.
struct Lap {
  hipEvent_t a = nullptr, b = nullptr;
  int pass = 0;
};
struct Laps {
  hipStream_t st;
  RunOwned own;
  std::vector<Lap> laps;
  explicit Laps(hipStream_t s) : st(s) {}
  hipError_t begin(int pass) {
    Lap L;
    L.pass = pass;
    hipError_t e = own.event(&L.a);
    if (e == hipSuccess) e = own.event(&L.b);
    if (e == hipSuccess) e = hipEventRecord(L.a, st);
    laps.push_back(L);
    return e;
  }
  hipError_t end() { return hipEventRecord(laps.back().b, st); }
  // After a synchronisation of the stream: every span's time is added to ms_pass[its pass] and to *ms_device.  A HIP
  // failure is reported with this header's file and line, not the stage's (HIPCHK sits here).
  int collect(double *ms_pass, double *ms_device) const {
    for (const Lap &L : laps) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, L.a, L.b));
      ms_pass[L.pass] += ms;
      *ms_device += ms;
    }
    return 0;
  }
};

// The workspace a stage may take: what the caller set on the context (ctx_bytes != 0), else eight tenths of the free
// device memory beyond hold_back (0 when less than that is free).  A failure of hipMemGetInfo is reported with this
// header's file and line.
inline int workspace_budget(uint64_t ctx_bytes, uint64_t hold_back, uint64_t *budget) {
  *budget = ctx_bytes;
  if (ctx_bytes) return 0;
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  *budget = free_b > hold_back ? (uint64_t)((free_b - hold_back) / 10 * 8) : 0;
  return 0;
}

// Declare it behind the buffers of a function: whatever is in flight ends before they go back to the pool.
struct SyncOnExit {
  hipStream_t st;
  ~SyncOnExit() { (void)hipStreamSynchronize(st); }
};

// The same for a run over up to three streams that ends with a synchronisation of its own: declare it behind the run's
// owners and set `ok` in front of the successful return.  On every other exit nothing of the run is in flight any more
// when the events, the pinned buffers and -- in the caller -- the context's device buffers are released.
struct SyncOnError {
  hipStream_t st[3] = {};
  bool ok = false;
  ~SyncOnError() { if (!ok) for (auto s : st) if (s) (void)hipStreamSynchronize(s); }
};

// The device of a new context: *device < 0 picks the current one.  `what` names the stage in the message.
inline int stage_device(int *device, const char *what) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(SPRING_REORDER_E_HIP, "no HIP device available (%s has no CPU fallback)", what);
  if (*device < 0 && hipGetDevice(device) != hipSuccess) *device = 0;
  if (*device >= ndev) return fail(SPRING_REORDER_E_ARG, "device %d out of range", *device);
  return 0;
}

// What every entry point that touches the device starts with: the context's device, and its stream on first use.
inline int stream_begin(int dev, hipStream_t *st) {
  HIPCHK(hipSetDevice(dev));
  if (!*st) HIPCHK(hipStreamCreate(st));
  return 0;
}

}  // namespace sr
#endif
