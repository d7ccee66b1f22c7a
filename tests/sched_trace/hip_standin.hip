// A recording stand-in for the part of the HIP runtime that the handle-level host code (api_gp.hip, gp_sched.hip) calls.
// No device: hipMalloc hands out disjoint fake address ranges that nobody may dereference, hipHostMalloc returns real memory,
// streams and events are counters, stream-memory operations are "supported", and everything that would be enqueued is
// written down instead (trace_rec.h).
#include "trace_rec.h"
#include <cstdlib>
#include <cstring>
#include <vector>

namespace trace {

bool recording = false;

struct Range {
  uintptr_t base;
  size_t bytes;
  std::string name;
  size_t elem;
  bool host;
  bool live;
};
static std::vector<Range> ranges;
static std::string out_buf;

static Range* find_range(const void* p) {
  const uintptr_t a = (uintptr_t)p;
  for (Range& r : ranges)
    if (r.live && a >= r.base && a < r.base + (r.bytes ? r.bytes : 1)) return &r;
  return nullptr;
}

void name_range(const void* base, const char* name, size_t elem_bytes) {
  if (Range* r = find_range(base)) {
    r->name = name;
    r->elem = elem_bytes;
  }
}

std::string ptr_json(const void* p) {
  if (!p) return "null";
  char b[96];
  if (const Range* r = find_range(p)) {
    const uintptr_t off = (uintptr_t)p - r->base;
    snprintf(b, sizeof(b), "[\"%s\",%llu]", r->name.c_str(), (unsigned long long)(off / r->elem));
  } else {
    snprintf(b, sizeof(b), "[\"?\",%llu]", (unsigned long long)(uintptr_t)p);
  }
  return b;
}

void emit_line(const std::string& json) {
  out_buf += json;
  out_buf += '\n';
  if (out_buf.size() > (1u << 20)) flush();
}

void flush() {
  fwrite(out_buf.data(), 1, out_buf.size(), stdout);
  fflush(stdout);
  out_buf.clear();
}

Rec::Rec(const char* kind, hipStream_t st) {
  char b[64];
  snprintf(b, sizeof(b), "{\"k\":\"%s\",\"s\":%d", kind, st ? st->id : -1);
  s_ = b;
}
Rec::~Rec() {
  if (!recording) return;
  s_ += '}';
  emit_line(s_);
}
Rec& Rec::fn(const char* name) { s_ += ",\"fn\":\""; s_ += name; s_ += '"'; return *this; }
Rec& Rec::i(const char* key, long long v) {
  char b[64];
  snprintf(b, sizeof(b), ",\"%s\":%lld", key, v);
  s_ += b;
  return *this;
}
Rec& Rec::u(const char* key, unsigned long long v) {
  char b[64];
  snprintf(b, sizeof(b), ",\"%s\":%llu", key, v);
  s_ += b;
  return *this;
}
Rec& Rec::d(const char* key, double v) {
  char b[64];
  snprintf(b, sizeof(b), ",\"%s\":%.17g", key, v);
  s_ += b;
  return *this;
}
Rec& Rec::p(const char* key, const void* ptr) { return raw(key, ptr_json(ptr)); }
Rec& Rec::raw(const char* key, const std::string& json) { s_ += ",\""; s_ += key; s_ += "\":"; s_ += json; return *this; }

// fake device addresses: 4 TiB apart (the largest matrix of the sweep, 2048 tile columns, is 0.5 TiB), far from anything mapped
static uintptr_t next_fake = (uintptr_t)1 << 44;
static int n_dev = 0, n_host = 0, n_stream = 0, n_event = 0;

}  // namespace trace

using namespace trace;

extern "C" {

const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "error (stand-in)"; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }

hipError_t hipDeviceGetAttribute(int* pi, hipDeviceAttribute_t attr, int) {
  *pi = attr == hipDeviceAttributeCanUseStreamWaitValue ? 1 : 0;
  return hipSuccess;
}
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) {
  *lo = 0;
  *hi = -1;
  return hipSuccess;
}

hipError_t hipMalloc(void** ptr, size_t size) {
  char nm[32];
  snprintf(nm, sizeof(nm), "dev%d", n_dev++);
  const uintptr_t base = next_fake;
  next_fake += (uintptr_t)1 << 42;
  ranges.push_back({base, size, nm, 1, false, true});
  *ptr = (void*)base;
  return hipSuccess;
}
hipError_t hipFree(void* ptr) {
  if (!ptr) return hipSuccess;
  for (Range& r : ranges)
    if (r.live && !r.host && r.base == (uintptr_t)ptr) { ranges.erase(ranges.begin() + (&r - ranges.data())); return hipSuccess; }
  return hipErrorInvalidValue;
}
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) {
  char nm[32];
  snprintf(nm, sizeof(nm), "host%d", n_host++);
  void* m = calloc(size ? size : 1, 1);
  if (!m) return hipErrorOutOfMemory;
  ranges.push_back({(uintptr_t)m, size, nm, 1, true, true});
  *ptr = m;
  return hipSuccess;
}
hipError_t hipHostFree(void* ptr) {
  if (!ptr) return hipSuccess;
  for (Range& r : ranges)
    if (r.live && r.host && r.base == (uintptr_t)ptr) { ranges.erase(ranges.begin() + (&r - ranges.data())); free(ptr); return hipSuccess; }
  return hipErrorInvalidValue;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) {
  *s = new ihipStream_t{n_stream++};
  return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int) {
  *s = new ihipStream_t{n_stream++};
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  delete s;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  Rec("sync", s);
  return hipSuccess;
}

hipError_t hipEventCreate(hipEvent_t* e) {
  *e = new ihipEvent_t{n_event++};
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) {
  delete e;
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  Rec("ev_record", s).i("ev", e->id);
  return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int) {
  Rec("ev_wait", s).i("ev", e->id);
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
  *ms = 0.0f;
  return hipSuccess;
}

hipError_t hipStreamWriteValue32(hipStream_t s, void* ptr, uint32_t value, unsigned int flags) {
  Rec("write32", s).p("ptr", ptr).u("val", value).u("flags", flags);
  return hipSuccess;
}
hipError_t hipStreamWaitValue32(hipStream_t s, void* ptr, uint32_t value, unsigned int flags, uint32_t mask) {
  Rec("wait32", s).p("ptr", ptr).u("val", value).u("flags", flags).u("mask", mask);
  return hipSuccess;
}

// device memory is fake: a memset of it is only written down; host memory is real
static bool is_host(const void* p) {
  const Range* r = find_range(p);
  return r && r->host;
}
hipError_t hipMemset(void* dst, int value, size_t bytes) {
  Rec("memset", nullptr).p("ptr", dst).i("value", value).u("bytes", bytes);
  if (is_host(dst)) memset(dst, value, bytes);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s) {
  Rec("memset", s).p("ptr", dst).i("value", value).u("bytes", bytes);
  if (is_host(dst)) memset(dst, value, bytes);
  return hipSuccess;
}
hipError_t hipMemsetD32Async(hipDeviceptr_t dst, int value, size_t count, hipStream_t s) {
  Rec("memset", s).p("ptr", dst).i("value", value).u("bytes", 4 * count);
  return hipSuccess;
}
// A download from fake memory: every byte 0x7f -- a bad-pivot word then reads "no bad pivot" (INFO_OK), which is also how the
// dispatch probe of mi_gp_create hears "concurrent" (its poll did not time out).
static void fake_copy(void* dst, const void* src, size_t bytes) {
  if (find_range(dst) && !is_host(dst)) return;  // (an upload: nothing to keep)
  if (!find_range(src) || is_host(src)) memmove(dst, src, bytes);
  else memset(dst, 0x7f, bytes);
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  Rec("memcpy", nullptr).p("dst", find_range(dst) ? dst : nullptr).p("src", find_range(src) ? src : nullptr).u("bytes", bytes);
  fake_copy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t s) {
  Rec("memcpy", s).p("dst", find_range(dst) ? dst : nullptr).p("src", find_range(src) ? src : nullptr).u("bytes", bytes);
  fake_copy(dst, src, bytes);
  return hipSuccess;
}

}  // extern "C"
