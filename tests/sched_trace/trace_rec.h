// Recording side of the schedule-trace program: one JSON record per enqueued operation, in enqueue order.
// Shared by the stand-ins for the HIP runtime (hip_standin.hip), for the kernel launchers (kernel_standin.hip) and by the
// program's main (trace_main.hip).  Nothing here knows what a launch reads or writes: tests/sched_check.py does.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <string>

// the runtime's opaque types, as the stand-in fills them
struct ihipStream_t { int id; };
struct ihipEvent_t { int id; };

namespace trace {

// names the range that holds `base`: fake device memory (never dereferenced) or real host memory; hipMalloc / hipHostMalloc
// call their ranges "dev<i>" / "host<i>" until then
void name_range(const void* base, const char* name, size_t elem_bytes);
std::string ptr_json(const void* p);  // ["name", element offset], null, or ["?", address]

// builds one record; written by its destructor
class Rec {
 public:
  Rec(const char* kind, hipStream_t st);
  ~Rec();
  Rec& fn(const char* name);
  Rec& i(const char* key, long long v);
  Rec& u(const char* key, unsigned long long v);
  Rec& d(const char* key, double v);
  Rec& p(const char* key, const void* ptr);
  Rec& raw(const char* key, const std::string& json);
 private:
  std::string s_;
};

void emit_line(const std::string& json);  // a line of its own (the main's config / begin / end records)
void flush();
extern bool recording;  // records are written while true (the main switches it on once the handle exists)

}  // namespace trace
