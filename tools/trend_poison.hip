// Test infrastructure only (tests/test_gpu_trend.py): fills ALL of a handle's trend scratch (option 50, csrc/api_trend.hip) with
// NaN -- every byte 0xff -- on the handle's stream, so that a test can show that an evaluation reads no element of it that the
// same call has not written.  Returns the number of doubles filled (0: the handle has no such scratch yet), -1 on an error.
#include "../andvaranaut_amd/csrc/gp_handle.h"

extern "C" __attribute__((visibility("default"))) long trend_poison(mi_gp_handle* h) {
  if (!h) return -1;
  const CapBlock& b = h->blocks[BLK_TREND];
  if (!b.p) return 0;
  const size_t len = b.len;
  if (hipSetDevice(h->device) != hipSuccess) return -1;
  if (hipMemsetAsync(b.p, 0xff, sizeof(double) * len, h->stream) != hipSuccess) return -1;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return -1;
  return (long)len;
}
