// hostsim (developer tool, never shipped): the HIP runtime entry points the
// host sources call, on plain host memory, so the unchanged session code
// (csrc/kbg_session.cpp and its .ipp) runs without a device.
//
// "Device" memory is malloc'ed host memory and a mapped pointer is its own
// device pointer. A stream is a queue of operations, run in order under one
// of two schedules (KBG_HOSTSIM_SCHEDULE, read once); both are legal
// executions of the HIP stream model:
//   eager — every operation runs at enqueue; hipEventQuery answers hipSuccess.
//   lazy  — operations queue and run at the last moment HIP allows:
//           hipEventSynchronize(e) and a successful hipEventQuery(e) run the
//           stream up to e's record and no further; hipStreamSynchronize, a
//           synchronous hipMemcpy / hipMemset, hipFree and hipHostFree drain
//           it; hipEventQuery of a pending event answers hipErrorNotReady
//           kQueryNotReady times, then runs up to it. An asynchronous copy
//           touches a pageable host side at enqueue (HIP stages pageable
//           memory before it returns; a device -> pageable copy waits for the
//           stream), pinned and mapped memory only when the copy runs.
// Fresh allocations are filled with a pattern (hipMalloc and hipHostMalloc
// return uninitialised memory). One mutex guards all of it: the session's
// Predictor thread allocates pinned memory beside the committer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <vector>

#include "hostsim.hpp"

namespace {

constexpr int kQueryNotReady = 3;
constexpr int kFillDevice = 0xCB, kFillPinned = 0xCD;

struct Stream {
  std::deque<std::function<void()>> q;
  uint64_t enqueued = 0, done = 0;  // operations ever enqueued / run
};

struct Event {
  Stream* stream = nullptr;  // where it was last recorded
  uint64_t seq = 0;          // complete once stream->done >= seq
  bool recorded = false;
  int polls = 0;
};

struct Sim {
  std::mutex mu;
  bool lazy = false;
  Stream null_stream;
  std::map<const char*, size_t> pinned, device;  // base -> bytes
  std::vector<Stream*> streams;
  Sim() {
    const char* e = getenv("KBG_HOSTSIM_SCHEDULE");
    lazy = e && strcmp(e, "lazy") == 0;
    streams.push_back(&null_stream);
  }
};
Sim& sim() {
  static Sim* s = new Sim();  // (never destroyed: buffers are returned during process exit)
  return *s;
}

Stream* stream_of(hipStream_t s) { return s ? reinterpret_cast<Stream*>(s) : &sim().null_stream; }

// (all below: sim().mu held)
void run_to(Stream* s, uint64_t seq) {
  while (s->done < seq && !s->q.empty()) {
    std::function<void()> fn = std::move(s->q.front());
    s->q.pop_front();
    fn();
    s->done++;
  }
}
void drain(Stream* s) { run_to(s, s->enqueued); }
void drain_all() {
  for (Stream* s : sim().streams) drain(s);
}
void push(Stream* s, std::function<void()> fn) {
  s->enqueued++;
  if (sim().lazy) {
    s->q.push_back(std::move(fn));
  } else {
    fn();
    s->done++;
  }
}
bool in_map(const std::map<const char*, size_t>& m, const void* p) {
  auto it = m.upper_bound((const char*)p);
  if (it == m.begin()) return false;
  --it;
  return (const char*)p < it->first + it->second;
}
bool complete(const Event* e) { return !e->recorded || e->stream->done >= e->seq; }

}  // namespace

void hostsim::enqueue(hipStream_t stream, std::function<void()> fn) {
  std::lock_guard<std::mutex> lk(sim().mu);
  push(stream_of(stream), std::move(fn));
}

extern "C" {

hipError_t hipGetDeviceCount(int* n) {
  *n = 1;
  return hipSuccess;
}
hipError_t hipGetDevice(int* d) {
  *d = 0;
  return hipSuccess;
}
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) {
  switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorInvalidDevice: return "invalid device ordinal";
    case hipErrorNotReady: return "device not ready";
    case hipErrorNotSupported: return "operation not supported (hostsim)";
    case hipErrorInvalidHandle: return "invalid resource handle";
    default: return "hostsim: HIP error";
  }
}

hipError_t hipMalloc(void** p, size_t bytes) {
  void* m = nullptr;  // exactly `bytes`: a sanitizer build sees the first byte past it
  if (posix_memalign(&m, 256, std::max<size_t>(bytes, 1)) != 0) return hipErrorOutOfMemory;
  memset(m, kFillDevice, bytes);
  std::lock_guard<std::mutex> lk(sim().mu);
  sim().device[(const char*)m] = bytes;
  *p = m;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  if (!p) return hipSuccess;
  std::lock_guard<std::mutex> lk(sim().mu);
  drain_all();
  if (!sim().device.erase((const char*)p)) return hipErrorInvalidValue;
  free(p);
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) {
  void* m = nullptr;
  if (posix_memalign(&m, 4096, std::max<size_t>(bytes, 1)) != 0) return hipErrorOutOfMemory;
  memset(m, kFillPinned, bytes);
  std::lock_guard<std::mutex> lk(sim().mu);
  sim().pinned[(const char*)m] = bytes;
  *p = m;
  return hipSuccess;
}
hipError_t hipHostFree(void* p) {
  if (!p) return hipSuccess;
  std::lock_guard<std::mutex> lk(sim().mu);
  drain_all();
  if (!sim().pinned.erase((const char*)p)) return hipErrorInvalidValue;
  free(p);
  return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned int) {
  std::lock_guard<std::mutex> lk(sim().mu);
  if (!in_map(sim().pinned, h)) return hipErrorInvalidValue;
  *d = h;
  return hipSuccess;
}

hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  std::lock_guard<std::mutex> lk(sim().mu);
  drain_all();
  if (bytes) memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipMemset(void* dst, int v, size_t bytes) {
  std::lock_guard<std::mutex> lk(sim().mu);
  drain_all();
  if (bytes) memset(dst, v, bytes);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t stream) {
  std::lock_guard<std::mutex> lk(sim().mu);
  Sim& S = sim();
  Stream* s = stream_of(stream);
  const bool src_pageable = !in_map(S.device, src) && !in_map(S.pinned, src);
  const bool dst_pageable = !in_map(S.device, dst) && !in_map(S.pinned, dst);
  if (dst_pageable) {  // the call returns with the pageable destination written
    drain(s);
    if (bytes) memcpy(dst, src, bytes);
    return hipSuccess;
  }
  if (src_pageable) {  // staged before the call returns
    std::vector<char> staged((const char*)src, (const char*)src + bytes);
    push(s, [dst, staged = std::move(staged)] {
      if (!staged.empty()) memcpy(dst, staged.data(), staged.size());
    });
    return hipSuccess;
  }
  push(s, [dst, src, bytes] {
    if (bytes) memmove(dst, src, bytes);
  });
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int v, size_t bytes, hipStream_t stream) {
  std::lock_guard<std::mutex> lk(sim().mu);
  push(stream_of(stream), [dst, v, bytes] {
    if (bytes) memset(dst, v, bytes);
  });
  return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* out, unsigned int) {
  Stream* s = new Stream();
  std::lock_guard<std::mutex> lk(sim().mu);
  sim().streams.push_back(s);
  *out = reinterpret_cast<hipStream_t>(s);
  return hipSuccess;
}
hipError_t hipStreamCreate(hipStream_t* out) { return hipStreamCreateWithFlags(out, 0); }
hipError_t hipStreamSynchronize(hipStream_t stream) {
  std::lock_guard<std::mutex> lk(sim().mu);
  drain(stream_of(stream));
  return hipSuccess;
}
// (hipStreamDestroy lets the pending work finish; the session destroys its
// events before its stream, so nothing refers to the stream afterwards)
hipError_t hipStreamDestroy(hipStream_t stream) {
  if (!stream) return hipErrorInvalidHandle;
  std::lock_guard<std::mutex> lk(sim().mu);
  Stream* s = stream_of(stream);
  drain(s);
  auto& v = sim().streams;
  v.erase(std::remove(v.begin(), v.end(), s), v.end());
  delete s;
  return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t* out, unsigned int) {
  *out = reinterpret_cast<hipEvent_t>(new Event());
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* out) { return hipEventCreateWithFlags(out, 0); }
hipError_t hipEventDestroy(hipEvent_t ev) {
  if (!ev) return hipErrorInvalidHandle;
  std::lock_guard<std::mutex> lk(sim().mu);
  delete reinterpret_cast<Event*>(ev);
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t stream) {
  if (!ev) return hipErrorInvalidHandle;
  std::lock_guard<std::mutex> lk(sim().mu);
  Event* e = reinterpret_cast<Event*>(ev);
  e->stream = stream_of(stream);
  e->seq = e->stream->enqueued;  // everything enqueued so far, nothing after
  e->recorded = true;
  e->polls = 0;
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t ev) {
  if (!ev) return hipErrorInvalidHandle;
  std::lock_guard<std::mutex> lk(sim().mu);
  Event* e = reinterpret_cast<Event*>(ev);
  if (e->recorded) run_to(e->stream, e->seq);
  return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t ev) {
  if (!ev) return hipErrorInvalidHandle;
  std::lock_guard<std::mutex> lk(sim().mu);
  Event* e = reinterpret_cast<Event*>(ev);
  if (complete(e)) return hipSuccess;
  if (++e->polls <= kQueryNotReady) return hipErrorNotReady;
  run_to(e->stream, e->seq);
  return hipSuccess;
}
// Both events recorded and complete, as HIP demands; the time itself is a
// fixed 1 µs per operation between them (nothing here has a duration).
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  if (!a || !b) return hipErrorInvalidHandle;
  std::lock_guard<std::mutex> lk(sim().mu);
  const Event *x = reinterpret_cast<Event*>(a), *y = reinterpret_cast<Event*>(b);
  if (!x->recorded || !y->recorded) return hipErrorInvalidHandle;
  if (!complete(x) || !complete(y)) return hipErrorNotReady;
  *ms = 0.001f * (float)(y->seq >= x->seq ? y->seq - x->seq : 0);
  return hipSuccess;
}

}  // extern "C"
