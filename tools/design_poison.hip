// Test infrastructure only (tests/test_gpu_design.py): fills ALL of a handle's design scratch (option 56, csrc/api_design.hip) with
// NaN -- every byte 0xff -- on the handle's stream, so that a test can show that a design call reads no element of it that the same
// call has not written.  Returns the number of doubles filled (0: the handle has no such scratch yet), -1 on an error.
#include "../andvaranaut_amd/csrc/gp_handle.h"

extern "C" __attribute__((visibility("default"))) long design_poison(mi_gp_handle* h) {
  if (!h) return -1;
  const CapBlock& b = h->blocks[BLK_DESIGN];
  if (!b.p) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return -1;
  if (hipMemsetAsync(b.p, 0xff, sizeof(double) * b.len, h->stream) != hipSuccess) return -1;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return -1;
  return (long)b.len;
}
