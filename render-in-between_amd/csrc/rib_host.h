// rib_host.h — what the two host objects of librib.so share: rib.o (rib.hip: the generator runtime) and frame.o (frame.hip: the
// folder driver's frame utilities).  Error plumbing, two one-line helpers and the part of the handle the utilities use; no
// planner type appears here.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/rib.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace rib {

inline std::string fmt(const char* f, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// XCD-aware tile order (RIB_NO_XCD=1 disables): needs the tile count to be a multiple of 8
inline int xcd_chunk_of(int tiles) {
  static const bool off = getenv("RIB_NO_XCD") != nullptr;
  return (!off && tiles >= 64 && tiles % 8 == 0) ? tiles / 8 : 0;
}

// Page-locked staging for the host tables of rib_rasterise and rib_human_mask: two slots, so that a call only enqueues and the
// caller's pageable arrays are free again on return.  A slot is reused once the work that read it has completed, which its
// event says; the CALLER records `done` after that work (rib_rasterise: after the copy out of `host`; rib_human_mask, which
// takes no workspace and keeps the device copy of its table in `dev`: after the kernel that reads `dev`).
struct StageRing {
  struct Slot { char* host = nullptr; char* dev = nullptr; size_t bytes = 0; hipEvent_t done = nullptr; };
  Slot slot[2];
  int next = 0;

  // the next slot, idle, with at least `bytes` of page-locked memory (and of device memory when asked for)
  hipError_t acquire(size_t bytes, bool with_device, Slot** out) {
    Slot& s = slot[next];
    next ^= 1;
    hipError_t e = s.done ? hipEventSynchronize(s.done) : hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    if (s.bytes < bytes || (with_device && !s.dev)) {
      free_buffers(s);
      const size_t cap = align256(bytes);
      if ((e = hipHostMalloc(reinterpret_cast<void**>(&s.host), cap, hipHostMallocDefault)) != hipSuccess) return e;
      s.bytes = cap;
      if (with_device && (e = hipMalloc(reinterpret_cast<void**>(&s.dev), cap)) != hipSuccess) { free_buffers(s); return e; }
    }
    *out = &s;
    return hipSuccess;
  }
  // waits for each slot's event, then frees everything
  void release() {
    for (Slot& s : slot) {
      if (s.done) { (void)hipEventSynchronize(s.done); (void)hipEventDestroy(s.done); s.done = nullptr; }
      free_buffers(s);
    }
  }

 private:
  static void free_buffers(Slot& s) {
    if (s.host) (void)hipHostFree(s.host);
    if (s.dev) (void)hipFree(s.dev);
    s.host = s.dev = nullptr; s.bytes = 0;
  }
};

// rib_png's code tables as the handle keeps them: the bytes they were built from (uploaded again only when these change) and
// the device copy (png.hip.h: PngDeviceTables).  A change of tables takes a new buffer on both sides, and the old ones live as
// long as the handle: work already enqueued, on any stream, may still read them.
struct PngTableState {
  void* dev = nullptr;         // the current device copy
  std::string key;             // the K * 286 code lengths it was built from
  std::vector<void*> dev_all;
  std::vector<void*> host_all; // what the uploads were staged from
  bool lds_ready = false;      // k_png_strips' dynamic-LDS limit has been raised on this handle's device
  void release() {
    for (void* d : dev_all) (void)hipFree(d);
    for (void* h : host_all) free(h);
    dev_all.clear(); host_all.clear(); dev = nullptr; key.clear();
  }
};

// the part of a rib_handle the frame utilities use (rib.hip: struct rib_handle : rib::FrameState)
struct FrameState {
  int device = 0;              // < 0: host-only handle
  std::string err;             // rib_last_error
  int label_nc = 0;            // rib_config::label_nc (rib_rasterise checks its channel count against it)
  bool warp_lds_ready = false; // rib_warp has raised k_warp's dynamic-LDS limit on this handle's device
  StageRing stage;
  PngTableState png;
};

// frame.hip's one way to the state of a handle; defined in rib.hip, where rib_handle is complete
FrameState* frame_state(rib_handle* h);

inline int fail(FrameState* h, int code, const std::string& msg) {
  h->err = msg;
  return code;
}

#define HIP_TRY(h, expr)                                                                   \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      (h)->err = fmt("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return RIB_ERR_HIP;                                                                  \
    }                                                                                      \
  } while (0)

}  // namespace rib
