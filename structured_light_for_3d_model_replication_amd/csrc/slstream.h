// libslgpu.so -- how a file's body leaves device memory in chunks, included by slgpu.hip (which owns the ring in
// sl_ctx and writes the host PLY files with put_all) and slmerge.hip (slmeshwrite.inl, which holds every mesh writer): two
// translation units of one library, hence a named namespace and inline functions.
//
// The body of a file never exists on the host as a whole.  A context owns one Ring of kRing slots, each a device
// buffer and a pinned host buffer of one chunk, allocated on first use and kept (they only grow); chunk k is packed
// into device slot k mod kRing, copied to pinned slot k mod kRing and written from there in stream_chunks' order
// (below).  Staging is kRing (slot + slot) bytes whatever the file's size.
//
// Part 1 (put_all, stream_chunks and the status codes they return) needs no HIP: a plain host compiler compiles
// it alone (tests/host/stream_chunks_check.cpp).  Part 2 is compiled by hipcc only.
#pragma once

#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <unistd.h>

#include "slgpu.h"

namespace slstream {

// ---- part 1: no HIP ---------------------------------------------------------------------------------------------

// write(2) until all of p[0 .. len) is out (short writes, EINTR)
inline bool put_all(int fd, const char* p, size_t len) {
  while (len) {
    const ssize_t w = write(fd, p, len);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return false;
    p += w;
    len -= static_cast<size_t>(w);
  }
  return true;
}

// The ring's order.  enqueue(k, slot): chunk k's work and the slot's event onto the stream; landed(slot): wait
// for that event; sink(k, slot): consume the pinned slot.  Chunk k + ring is queued only after chunk k was
// consumed; after a failure nothing more is queued, and everything queued is still waited for.
template <class Enqueue, class Landed, class Sink>
int stream_chunks(int64_t n_chunks, int ring, Enqueue enqueue, Landed landed, Sink sink) {
  int64_t queued = 0;
  bool dev_ok = true, io_ok = true;
  for (int64_t k = 0; k < n_chunks; ++k) {
    while (dev_ok && io_ok && queued < n_chunks && queued < k + ring) {
      dev_ok = enqueue(queued, static_cast<int>(queued % ring));
      if (dev_ok) ++queued;
    }
    if (k >= queued) break;
    dev_ok = landed(static_cast<int>(k % ring)) && dev_ok;
    if (dev_ok && io_ok) io_ok = sink(k, static_cast<int>(k % ring));
  }
  return !dev_ok ? SL_EHIP : !io_ok ? SL_EIO : SL_OK;
}

}  // namespace slstream

// ---- part 2: the ring and the file around the loop --------------------------------------------------------------
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>

// slgpu.hip: the context's error text, and open(path) for writing from byte 0 (the reaper's one instance)
int slgpu_fail(sl_ctx* c, int code, const char* msg);
int slgpu_open_replacing(const char* path);

namespace slstream {

constexpr int kRing = 2;

struct Ring {
  char* dev[kRing] = {};
  char* pin[kRing] = {};
  hipEvent_t ev[kRing] = {};
  int64_t cap = 0;  // bytes of every slot
};

inline void ring_drop_slots(Ring* r) {
  for (int i = 0; i < kRing; ++i) {
    if (r->dev[i]) (void)hipFree(r->dev[i]);
    if (r->pin[i]) (void)hipHostFree(r->pin[i]);
    r->dev[i] = r->pin[i] = nullptr;
  }
  r->cap = 0;
}

// with the context (the device current)
inline void ring_release(Ring* r) {
  ring_drop_slots(r);
  for (hipEvent_t e : r->ev)
    if (e) (void)hipEventDestroy(e);
}

// Slots of at least `bytes` (idle between calls: a writer waits for all it queued).
inline hipError_t ring_reserve(Ring* r, int64_t bytes) {
  hipError_t e = hipSuccess;
  for (int i = 0; i < kRing && e == hipSuccess; ++i)
    if (!r->ev[i]) e = hipEventCreateWithFlags(&r->ev[i], hipEventDisableTiming);
  if (e != hipSuccess || r->cap >= bytes) return e;
  ring_drop_slots(r);
  for (int i = 0; i < kRing && e == hipSuccess; ++i) {
    e = hipMalloc(reinterpret_cast<void**>(&r->dev[i]), static_cast<size_t>(bytes));
    if (e == hipSuccess)
      e = hipHostMalloc(reinterpret_cast<void**>(&r->pin[i]), static_cast<size_t>(bytes), hipHostMallocDefault);
  }
  if (e == hipSuccess) r->cap = bytes;
  return e;
}

inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The file (path NULL: no file, everything else the same -- a measurement aid): `head`, then the chunks through
// `ring`.  pack(k, dev): chunk k's kernels onto `s`; bytes(k): its size; `what` heads the error texts.  ms[3]: +=
// waiting for chunks to land, += writing them, = the whole call.
template <class Pack, class Bytes>
int write_chunks(sl_ctx* c, const char* what, const char* path, const char* head, size_t head_len, Ring* ring,
                 int64_t n_chunks, Pack pack, Bytes bytes, hipStream_t s, double* ms) {
  const auto t_all = std::chrono::steady_clock::now();
  const int fd = path ? slgpu_open_replacing(path) : -1;
  if (path && fd < 0) return slgpu_fail(c, SL_EIO, (std::string(what) + ": cannot open the file").c_str());
  bool io_ok = !path || put_all(fd, head, head_len);
  const int r = stream_chunks(
      io_ok ? n_chunks : 0, kRing,
      [&](int64_t k, int slot) {
        pack(k, ring->dev[slot]);
        return hipGetLastError() == hipSuccess &&
               hipMemcpyAsync(ring->pin[slot], ring->dev[slot], static_cast<size_t>(bytes(k)), hipMemcpyDeviceToHost,
                              s) == hipSuccess &&
               hipEventRecord(ring->ev[slot], s) == hipSuccess;
      },
      [&](int slot) {
        const auto t0 = std::chrono::steady_clock::now();
        const bool ok = hipEventSynchronize(ring->ev[slot]) == hipSuccess;
        ms[0] += ms_since(t0);
        return ok;
      },
      [&](int64_t k, int slot) {
        if (!path) return true;
        const auto t0 = std::chrono::steady_clock::now();
        const bool ok = put_all(fd, ring->pin[slot], static_cast<size_t>(bytes(k)));
        ms[1] += ms_since(t0);
        return ok;
      });
  if (r == SL_EHIP) (void)hipStreamSynchronize(s);  // a half-queued chunk may still be writing its slot
  if (fd >= 0) io_ok = (close(fd) == 0) && io_ok;
  ms[2] = ms_since(t_all);
  if (r == SL_EHIP) return slgpu_fail(c, SL_EHIP, (std::string(what) + ": packing or copying failed").c_str());
  if (r == SL_EIO || !io_ok) return slgpu_fail(c, SL_EIO, (std::string(what) + ": writing the file failed").c_str());
  return SL_OK;
}

}  // namespace slstream

slstream::Ring* slgpu_file_ring(sl_ctx* c);  // slgpu.hip: the context's ring
#endif  // __HIPCC__
