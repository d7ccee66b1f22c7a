// The data-side gradients of the sparse inducing-point bound, the one entry point libmi_gp_sparse_data.so has beyond
// libmi_gp_sparse.so's (include/mi_gp_sparse_data.h has the algebra and the contract): binding the outputs, and the step pass 2 of
// api_sparse.hip takes per chunk once they are bound -- the kernels of sparse_xgrad_f64.hip.
#include <cstdio>
#include "sparse_object.h"
#include "../../include/mi_gp_sparse_data.h"

using namespace migp;

// the slab scratch of the X kernel: what the longer of the two chunk lengths the data has takes (the slab count is no monotone
// function of the chunk's points, so both are asked)
static long xscratch_need(const mi_gp_sparse* s) {
  const int full = std::min(s->chunk, s->n), last = s->n % s->chunk;
  long len = sparse_xgrad_scratch(full, s->m, s->d, s->xcap);
  if (last > 0) len = std::max(len, sparse_xgrad_scratch(last, s->m, s->d, s->xcap));
  return len;
}

extern "C" int mi_gp_sparse_bind_data_grad(mi_gp_sparse* s, double* gy_dev, double* gx_dev, int xgrad_slabs) {
  if (!s) {
    snprintf(g_sparse_err, sizeof(g_sparse_err), "mi_gp_sparse_bind_data_grad: null object");
    return -1;
  }
  if (!gy_dev && gx_dev) {
    snprintf(s->err, sizeof(s->err), "mi_gp_sparse_bind_data_grad: gx_dev needs gy_dev (gy_dev == NULL unbinds both)");
    return -1;
  }
  if (xgrad_slabs < 1) {
    snprintf(s->err, sizeof(s->err), "mi_gp_sparse_bind_data_grad: xgrad_slabs must be >= 1, got %d", xgrad_slabs);
    return -1;
  }
  s->gy_out = gy_dev;
  s->gx_out = gx_dev;
  s->xcap = xgrad_slabs;
  return 0;
}

namespace migp {

int sparse_data_grad_chunk(mi_gp_sparse* s, const SparseWork& w, long i0, int cnt, double sv) {
  hipError_t e = launch_sparse_ygrad(w.Wc, s->mp, s->m, w.ahat, s->y + i0, cnt, sv, s->gy_out + i0, s->stream);
  if (e == hipSuccess && s->gx_out) {
    const long need = xscratch_need(s);
    if (need > s->xscratch_len) {  // the first call, or a larger cap since (every earlier call has returned synchronised)
      (void)hipFree(s->xscratch);
      s->xscratch = nullptr;
      s->xscratch_len = 0;
      e = hipMalloc(&s->xscratch, sizeof(double) * (size_t)need);
      if (e == hipSuccess) s->xscratch_len = need;
    }
    if (e == hipSuccess)
      e = launch_sparse_xgrad(s->spec, s->theta_dev(), s->X + i0 * s->d, cnt, s->Z, s->m, w.Tc, s->mp, s->y + i0, w.tv, s->xcap,
                              s->xscratch, s->gx_out + i0 * s->d, s->stream);
  }
  if (e != hipSuccess) {
    snprintf(s->err, sizeof(s->err), "data-side gradients: %s", hipGetErrorString(e));
    return -2;
  }
  return 0;
}

}  // namespace migp
