// The sparse bound's object and the layout of its work block, shared by api_sparse.hip (the C-ABI of include/mi_gp_sparse.h) and
// api_sparse_data.hip (the one entry point more of include/mi_gp_sparse_data.h).  Internal: nothing here is exported.
#pragma once
#include <algorithm>
#include "migp_kernels.h"
#include "../../include/mi_gp_sparse.h"

namespace migp {

constexpr int SPARSE_MAX_M = 2048;       // 16 tile columns: the widest panel the factorisation uses
constexpr int SPARSE_CHUNK = 8192;       // default data points per pass step
constexpr int SPARSE_VECS = 8;           // vectors of mp doubles at the end of the work block (seven used)

inline int pad128(int x) { return (x + 127) / 128 * 128; }

// The caller's work block: nine mp x mp blocks (leading dimension mp), two blocks of chunk work rows, the leaf inverses of L and
// LB, eight vectors
struct SparseWork {
  double *Kuu, *Psi, *Bm, *U, *UB, *Binv, *H, *G0, *M2;  // Binv later holds G0 U^T, H later U G0 U^T (= -2 Guu)
  double *Wc, *Tc;                                       // K(X_c, Z) -> A_c^T; T_c^T (predict: b* rows)
  double *dinvL, *dinvB;
  double *v, *vs, *cvec, *ahat, *traw, *tv, *zero;       // v, v / s, c, a^, L^-T a^, that / s, the zero alpha of Kuu's contraction
};
inline long sparse_work_len(long mp, long chunk) { return 9 * mp * mp + 2 * chunk * mp + 2 * (mp / 128) * MINV_ELEMS + SPARSE_VECS * mp; }
inline SparseWork sparse_layout(double* base, long mp, long chunk) {
  SparseWork w;
  double* p = base;
  double** blocks[9] = {&w.Kuu, &w.Psi, &w.Bm, &w.U, &w.UB, &w.Binv, &w.H, &w.G0, &w.M2};
  for (auto b : blocks) { *b = p; p += mp * mp; }
  w.Wc = p; p += chunk * mp;
  w.Tc = p; p += chunk * mp;
  w.dinvL = p; p += (mp / 128) * MINV_ELEMS;
  w.dinvB = p; p += (mp / 128) * MINV_ELEMS;
  double** vecs[7] = {&w.v, &w.vs, &w.cvec, &w.ahat, &w.traw, &w.tv, &w.zero};
  for (auto v : vecs) { *v = p; p += mp; }
  return w;
}

}  // namespace migp

struct mi_gp_sparse {
  mi_gp_sparse_config cfg;
  migp::KernSpec spec;
  int n, m, mp, ntm, d, P, chunk;
  hipStream_t stream = nullptr;
  // the object's own scratch (first mi_gp_sparse_set_data): theta [P], the chunks' gradient [P], Kuu's gradient [P], two scalar
  // records [8] each, yy [2], the two bad-pivot words [2 doubles], dF/dZ [m d, with zgrad_slabs >= 1 only], then the partial sums
  // of the two contractions and, with zgrad_slabs >= 1, Kuu's part of dF/dZ [m d] and the slab scratch the two passes over Z share
  double* own_dev = nullptr;
  double* host = nullptr;  // pinned mirror of the first 3 P + 20 (+ m d) doubles
  const double *X = nullptr, *y = nullptr, *Z = nullptr;
  double* work = nullptr;
  bool have_data = false, factored = false;
  double fac_s = 0.0, fac_kdiag = 0.0;  // noise variance and prior variance at the factored theta
  char err[256] = "";
  // the data-side gradients (mi_gp_sparse_bind_data_grad, include/mi_gp_sparse_data.h): borrowed device outputs, the cap on the
  // X kernel's slabs and its slab scratch, an allocation of its own that the first gradient call with dF/dX bound makes.  Nothing
  // but that entry point sets them: in a library without it they stay null and every call is what it was before they existed
  double *gy_out = nullptr, *gx_out = nullptr;
  int xcap = 0;
  double* xscratch = nullptr;
  long xscratch_len = 0;  // doubles
  int zcap() const { return cfg.zgrad_slabs; }  // 0: no dF/dZ, every call as it was before the field existed
  long zlen() const { return zcap() > 0 ? (long)m * d : 0; }
  long small_len() const { return 3L * P + 20 + zlen(); }
  double* theta_dev() const { return own_dev; }
  double* gacc_dev() const { return own_dev + P; }
  double* gsym_dev() const { return own_dev + 2 * P; }
  double* scal_dev() const { return own_dev + 3 * P; }        // [0..8) pass 1's record, [8..16) the gradient's
  double* yy_dev() const { return own_dev + 3 * P + 16; }
  int* info_dev() const { return reinterpret_cast<int*>(own_dev + 3 * P + 18); }  // [0] Kuu, [1] B
  double* gz_dev() const { return own_dev + 3 * P + 20; }    // dF/dZ: the chunks' sums, then Kuu's part added
  double* part_rect_dev() const { return own_dev + small_len(); }
  double* part_sym_dev() const { return part_rect_dev() + (long)migp::sparse_contract_blocks(chunk, m) * P; }
  double* gzsym_dev() const { return part_sym_dev() + (long)migp::grad_contract_blocks(m) * P; }
  double* zscratch_dev() const { return gzsym_dev() + zlen(); }
  // the slab scratch: the largest chunk's slabs of sparse_zgrad, or the column splits of grad_x over Z (one after the other)
  long zscratch_len() const {
    if (zcap() <= 0) return 0;
    const int splits = migp::grad_x_splits(m, d);
    return std::max(migp::sparse_zgrad_scratch(std::min(chunk, n), m, d, zcap()), splits > 1 ? (long)splits * m * d : 0L);
  }
};

extern thread_local char g_sparse_err[256];  // (api_sparse.hip) the text behind mi_gp_sparse_last_error(NULL)

namespace migp {

// (api_sparse_data.hip) The data-side gradients of one chunk of pass 2, behind its contraction: dF/dy from the resident rows A_c^T
// and, with dF/dX bound, the X kernel on the weights the contraction read.  Weak, as the handle's mode functions are
// (gp_handle.h): libmi_gp_sparse.so is linked without it and never binds an output, so its pass 2 never asks for it.
// 0, or a C-ABI error code with the text in s->err
int sparse_data_grad_chunk(mi_gp_sparse* s, const SparseWork& w, long i0, int cnt, double sv) __attribute__((weak));

}  // namespace migp
