// The sparse inducing-point bound, the C-ABI of libmi_gp_sparse.so (include/mi_gp_sparse.h has the algebra and the contract): an
// object of its own in the manner of mi_gp_shard, built from the launchers the dense paths use -- the cross-assembly and blocked solve of
// mi_gp_predict, the panel factorisation of mi_gp_chol_panel, the GEMM, the symmetric contraction of mi_gp_lml_grad -- and the
// kernels of sparse_f64.hip and, for the gradient by the inducing locations, sparse_zgrad_f64.hip.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "sparse_object.h"  // struct mi_gp_sparse and the work block's layout (shared with api_sparse_data.hip)

using namespace migp;

thread_local char g_sparse_err[256] = "";

static int sfail(mi_gp_sparse* s, hipError_t e, const char* where) {
  snprintf(s->err, sizeof(s->err), "%s: %s", where, hipGetErrorString(e));
  return -2;
}
#define SCK(call, where)                                  \
  do {                                                    \
    hipError_t e__ = (call);                              \
    if (e__ != hipSuccess) return sfail(s, e__, where);   \
  } while (0)

extern "C" const char* mi_gp_sparse_last_error(mi_gp_sparse* s) { return s ? s->err : g_sparse_err; }

extern "C" long mi_gp_sparse_work(int m, int chunk) {
  if (m < 1 || m > SPARSE_MAX_M || chunk <= 0 || chunk % 128) {
    snprintf(g_sparse_err, sizeof(g_sparse_err), "mi_gp_sparse_work: 1 <= m <= %d and chunk a positive multiple of 128", SPARSE_MAX_M);
    return -1;
  }
  return sparse_work_len(pad128(m), chunk);
}

extern "C" int mi_gp_sparse_destroy(mi_gp_sparse* s) {
  if (!s) return 0;
  if (s->stream || s->own_dev || s->host || s->xscratch) {
    (void)hipSetDevice(s->cfg.device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    (void)hipFree(s->own_dev);
    (void)hipFree(s->xscratch);
    if (s->host) (void)hipHostFree(s->host);
    if (s->stream) (void)hipStreamDestroy(s->stream);
  }
  delete s;
  return 0;
}

extern "C" int mi_gp_sparse_create(const mi_gp_sparse_config* cfg, mi_gp_sparse** out) {
  if (!cfg || !out) { snprintf(g_sparse_err, sizeof(g_sparse_err), "mi_gp_sparse_create: null argument"); return -1; }
  if (cfg->n <= 0 || cfg->d <= 0 || cfg->device < 0) {
    snprintf(g_sparse_err, sizeof(g_sparse_err), "mi_gp_sparse_create: n and d must be positive, device >= 0");
    return -1;
  }
  if (cfg->m < 1 || cfg->m > SPARSE_MAX_M || cfg->m > cfg->n) {
    snprintf(g_sparse_err, sizeof(g_sparse_err), "mi_gp_sparse_create: 1 <= m <= min(n, %d), got m = %d, n = %d", SPARSE_MAX_M, cfg->m, cfg->n);
    return -1;
  }
  if (cfg->chunk < 0 || cfg->chunk % 128) {
    snprintf(g_sparse_err, sizeof(g_sparse_err), "mi_gp_sparse_create: chunk must be a multiple of 128 (0: the default), got %d", cfg->chunk);
    return -1;
  }
  if (cfg->zgrad_slabs < 0) {
    snprintf(g_sparse_err, sizeof(g_sparse_err), "mi_gp_sparse_create: zgrad_slabs must be >= 0 (0: no dF/dZ), got %d", cfg->zgrad_slabs);
    return -1;
  }
  if (const char* why = kern_spec_error(cfg->nkern, cfg->kernel_ids, cfg->ops)) {
    snprintf(g_sparse_err, sizeof(g_sparse_err), "mi_gp_sparse_create: %s", why);
    return -1;
  }
  mi_gp_sparse* s = new mi_gp_sparse();
  s->cfg = *cfg;
  s->spec = make_kern_spec(cfg->d, cfg->nkern, cfg->kernel_ids, cfg->ops);
  s->n = cfg->n;
  s->m = cfg->m;
  s->d = cfg->d;
  s->mp = pad128(cfg->m);
  s->ntm = s->mp / 128;
  s->P = cfg->nkern * cfg->d + 2 * cfg->nkern + 2;
  s->chunk = cfg->chunk ? cfg->chunk : SPARSE_CHUNK;
  *out = s;
  return 0;
}

extern "C" int mi_gp_sparse_set_data(mi_gp_sparse* s, const double* X_dev, const double* y_dev, int n, const double* Z_dev,
                                     double* work_dev, long work_len) {
  if (!s) { snprintf(g_sparse_err, sizeof(g_sparse_err), "mi_gp_sparse_set_data: null object"); return -1; }
  if (!X_dev || !y_dev || !Z_dev || !work_dev) { snprintf(s->err, sizeof(s->err), "mi_gp_sparse_set_data: null buffer"); return -1; }
  if (n != s->n) { snprintf(s->err, sizeof(s->err), "mi_gp_sparse_set_data: n = %d is not the configured %d", n, s->n); return -1; }
  const long need = sparse_work_len(s->mp, s->chunk);
  if (work_len < need || (work_len & 1) || (reinterpret_cast<uintptr_t>(work_dev) & 15)) {
    snprintf(s->err, sizeof(s->err), "mi_gp_sparse_set_data: work_len must be even and >= mi_gp_sparse_work(m, chunk) = %ld, the address 16-byte aligned (got %ld)",
             need, work_len);
    return -1;
  }
  s->have_data = s->factored = false;
  SCK(hipSetDevice(s->cfg.device), "hipSetDevice");
  if (!s->stream) SCK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "hipStreamCreate");
  if (!s->own_dev) {
    const long own = s->small_len() + ((long)sparse_contract_blocks(s->chunk, s->m) + grad_contract_blocks(s->m)) * s->P + s->zlen() +
                     s->zscratch_len();
    SCK(hipMalloc(&s->own_dev, sizeof(double) * own), "hipMalloc");
  }
  if (!s->host) SCK(hipHostMalloc(&s->host, sizeof(double) * s->small_len()), "hipHostMalloc");
  if (ensure_kernel_attributes() != 0) { snprintf(s->err, sizeof(s->err), "mi_gp_sparse_set_data: the kernels' LDS limits could not be set"); return -2; }
  s->X = X_dev;
  s->y = y_dev;
  s->Z = Z_dev;
  s->work = work_dev;
  s->have_data = true;
  return 0;
}

// A = L^-1 K(Z, X_c) as the rows A_c^T of Wc for the cnt points from i0 on (rows_c = cnt rounded up to 128, zeros in the padding)
static hipError_t chunk_rows(mi_gp_sparse* s, const SparseWork& w, const double* Xc, int cnt, int rows_c) {
  hipError_t e = launch_assemble(s->spec, s->theta_dev(), Xc, cnt, s->Z, s->m, w.Wc, s->mp, rows_c, s->mp, 0, 0, s->stream);
  if (e != hipSuccess) return e;
  return trsm_blocks(w.Kuu, s->mp, w.dinvL, w.Wc, s->mp, rows_c, 0, s->ntm, s->stream);
}

// C (mp x mp, leading dimension mp) = alpha op(A) op(B) over all tiles or the lower ones
static hipError_t square_gemm(mi_gp_sparse* s, const double* A, int ak, const double* B, int bk, double* C, double alpha, int tri) {
  GemmParams p;
  p.A = A; p.B = B; p.C = C;
  p.lda = p.ldb = p.ldc = s->mp;
  p.strideA = p.strideB = p.strideC = 0;
  p.mt = p.nt = s->ntm; p.k = s->mp; p.tri = tri; p.kmode = 0; p.alpha = alpha; p.beta = 0.0;
  return launch_gemm_f64(p, ak, bk, 1, s->stream);
}

// identity into an mp x mp block, then X L^T = I in place: X = L^-T
static hipError_t inverse_transpose_block(mi_gp_sparse* s, const double* L, const double* dinv, double* U) {
  hipError_t e = hipMemsetAsync(U, 0, sizeof(double) * (size_t)s->mp * s->mp, s->stream);
  if (e == hipSuccess) e = launch_set_identity_blocks(U, s->mp, s->ntm, s->stream);
  if (e == hipSuccess) e = trsm_blocks(L, s->mp, dinv, U, s->mp, s->mp, 0, s->ntm, s->stream);
  return e;
}

// the composite prior variance (predict_scalars' fold of kv) and its derivative by every kv_c (the fold's coefficients)
static double prior_diag(const KernSpec& spec, const double* th, double* dkv) {
  const int nk = spec.nkern, d = spec.d;
  const double* kv = th + nk * d;
  double pref[MAX_KERN];
  double T = kv[0];
  pref[0] = 1.0;
  for (int c = 1; c < nk; ++c) {
    pref[c] = (spec.op[c - 1] == 0) ? 1.0 : T;
    T = (spec.op[c - 1] == 0) ? T + kv[c] : T * kv[c];
  }
  if (dkv)
    for (int c = 0; c < nk; ++c) {
      double coef = pref[c];
      for (int c2 = c + 1; c2 < nk; ++c2)
        if (spec.op[c2 - 1] == 1) coef *= kv[c2];
      dkv[c] = coef;
    }
  return T;
}

// nullptr or why theta is refused
static const char* theta_error(const mi_gp_sparse* s, const double* th) {
  for (int i = 0; i < s->P; ++i)
    if (!std::isfinite(th[i])) return "theta must be finite";
  if (!(th[s->P - 2] + th[s->P - 1] > 0.0)) return "the noise variance s = gv + jitter must be positive";
  return nullptr;
}

// Pass 1 and the algebra of F at theta: L, LB, c, LB^-T and both sets of leaf inverses are left in the work block.  0 with
// *bound = F; info > 0 with *bound = -inf; or a C-ABI error code
static int pass_one(mi_gp_sparse* s, const double* theta, double* bound) {
  const SparseWork w = sparse_layout(s->work, s->mp, s->chunk);
  const int n = s->n, m = s->m, mp = s->mp, P = s->P;
  const double sv = theta[P - 2] + theta[P - 1];
  *bound = -INFINITY;
  SCK(hipSetDevice(s->cfg.device), "hipSetDevice");
  memcpy(s->host, theta, sizeof(double) * P);
  SCK(hipMemcpyAsync(s->theta_dev(), s->host, sizeof(double) * P, hipMemcpyHostToDevice, s->stream), "theta upload");
  SCK(hipMemsetAsync(s->info_dev(), 0x7f, 2 * sizeof(int), s->stream), "info reset");
  SCK(hipMemsetAsync(w.Psi, 0, sizeof(double) * (size_t)mp * mp, s->stream), "Psi reset");
  SCK(hipMemsetAsync(w.v, 0, sizeof(double) * (size_t)SPARSE_VECS * mp, s->stream), "vector reset");
  // Kuu = K(Z, Z) + jitter I (identity in the padding) and its factor
  SCK(launch_assemble(s->spec, s->theta_dev(), s->Z, m, s->Z, m, w.Kuu, mp, mp, mp, 1, 4, s->stream), "assemble Kuu");
  SCK(chol_panel_blocks(w.Kuu, mp, s->ntm, s->ntm, w.dinvL, s->info_dev(), 0, s->stream), "factor Kuu");
  int* info_host = reinterpret_cast<int*>(s->host + 3 * P + 18);
  SCK(hipMemcpyAsync(info_host, s->info_dev(), 2 * sizeof(int), hipMemcpyDeviceToHost, s->stream), "info download");
  SCK(hipStreamSynchronize(s->stream), "stream sync");
  if (info_host[0] != INFO_OK) return info_host[0];
  // the data in chunks of `chunk` points, in index order
  for (long i0 = 0; i0 < n; i0 += s->chunk) {
    const int cnt = (int)std::min<long>(s->chunk, n - i0), rows_c = pad128(cnt), first = i0 == 0;
    SCK(chunk_rows(s, w, s->X + i0 * s->d, cnt, rows_c), "chunk rows");
    GemmParams p;  // Psi += A_c A_c^T over the lower tiles: both operands the chunk's rows, stored [k][x]
    p.A = w.Wc; p.B = w.Wc; p.C = w.Psi;
    p.lda = p.ldb = p.ldc = mp;
    p.strideA = p.strideB = p.strideC = 0;
    p.mt = p.nt = s->ntm; p.k = rows_c; p.tri = 1; p.kmode = 0; p.alpha = 1.0; p.beta = 1.0;
    SCK(launch_gemm_f64(p, 1, 1, 1, s->stream), "Psi update");
    SCK(launch_sparse_accum_vy(w.Wc, mp, mp, s->y + i0, cnt, w.v, s->yy_dev(), first, s->stream), "v and yy");
  }
  // B = I + Psi / s, its factor, LB^-T and c = LB^-1 v / s
  SCK(launch_sparse_make_b(w.Psi, w.Bm, mp, sv, s->stream), "B");
  SCK(chol_panel_blocks(w.Bm, mp, s->ntm, s->ntm, w.dinvB, s->info_dev() + 1, 0, s->stream), "factor B");
  SCK(inverse_transpose_block(s, w.Bm, w.dinvB, w.UB), "LB^-T");
  SCK(launch_sparse_scale(w.v, w.vs, mp, sv, s->stream), "v / s");
  SCK(launch_trmv_upper_t(w.UB, mp, w.vs, m, w.cvec, s->stream), "c");
  SCK(launch_sparse_scalars(w.Bm, w.Psi, mp, w.cvec, nullptr, nullptr, m, s->scal_dev(), s->stream), "scalars");
  SCK(hipMemcpyAsync(s->host + 3 * P, s->scal_dev(), sizeof(double) * 20, hipMemcpyDeviceToHost, s->stream), "scalars download");
  SCK(hipStreamSynchronize(s->stream), "stream sync");
  if (info_host[1] != INFO_OK) return m + info_host[1];
  const double* sc = s->host + 3 * P;
  const double yy = s->host[3 * P + 16];
  const double kappa = (double)n * prior_diag(s->spec, theta, nullptr);
  *bound = -0.5 * n * (LOG_2PI + std::log(sv)) - sc[0] - yy / (2.0 * sv) + 0.5 * sc[2] - (kappa - sc[1]) / (2.0 * sv);
  return 0;
}

// The gradient behind a successful pass_one at the same theta
static int gradient(mi_gp_sparse* s, const double* theta, double* grad_out) {
  const SparseWork w = sparse_layout(s->work, s->mp, s->chunk);
  const int n = s->n, m = s->m, mp = s->mp, P = s->P, nk = s->spec.nkern, d = s->d;
  const double sv = theta[P - 2] + theta[P - 1];
  SCK(launch_trmv_upper(w.UB, mp, w.cvec, m, w.ahat, s->stream), "a^");
  SCK(inverse_transpose_block(s, w.Kuu, w.dinvL, w.U), "L^-T");
  SCK(square_gemm(s, w.UB, 0, w.UB, 0, w.Binv, 1.0, 0), "B^-1");  // B^-1 = LB^-T LB^-1
  SCK(launch_sparse_scalars(w.Bm, w.Psi, mp, w.cvec, w.ahat, w.Binv, m, s->scal_dev() + 8, s->stream), "scalars");
  SCK(launch_sparse_hg(w.Psi, w.Binv, w.ahat, mp, sv, w.H, w.G0, s->stream), "H and G0");
  SCK(square_gemm(s, w.H, 0, w.U, 0, w.M2, 1.0 / sv, 0), "M2");      // M2 = H L^-1 / s
  SCK(square_gemm(s, w.G0, 0, w.U, 0, w.Binv, 1.0, 0), "G0 L^-1");   // (B^-1 is done with)
  SCK(square_gemm(s, w.U, 0, w.Binv, 1, w.H, 1.0, 1), "-2 Guu");     // L^-T G0 L^-1 = -2 Guu, lower tiles (H is done with)
  SCK(launch_trmv_upper(w.U, mp, w.ahat, m, w.traw, s->stream), "L^-T a^");
  SCK(launch_sparse_scale(w.traw, w.tv, mp, sv, s->stream), "L^-T a^ / s");
  for (long i0 = 0; i0 < n; i0 += s->chunk) {
    const int cnt = (int)std::min<long>(s->chunk, n - i0), rows_c = pad128(cnt), first = i0 == 0;
    SCK(chunk_rows(s, w, s->X + i0 * d, cnt, rows_c), "chunk rows");
    GemmParams p;  // T_c^T = A_c^T M2 (the rank-one part y_c (L^-T a^)^T / s is added where the contraction reads its weights)
    p.A = w.Wc; p.B = w.M2; p.C = w.Tc;
    p.lda = p.ldb = p.ldc = mp;
    p.strideA = p.strideB = p.strideC = 0;
    p.mt = rows_c / 128; p.nt = s->ntm; p.k = mp; p.tri = 0; p.kmode = 0; p.alpha = 1.0; p.beta = 0.0;
    SCK(launch_gemm_f64(p, 0, 1, 1, s->stream), "T rows");
    SCK(launch_sparse_contract(s->spec, s->theta_dev(), s->X + i0 * d, cnt, s->Z, m, w.Tc, mp, s->y + i0, w.tv, s->part_rect_dev(),
                               s->gacc_dev(), first, s->stream), "contraction");
    if (s->zcap() > 0)  // Kuf's term of dF/dZ on the same weights: the chunks in chunk order onto gz
      SCK(launch_sparse_zgrad(s->spec, s->theta_dev(), s->X + i0 * d, cnt, s->Z, m, w.Tc, mp, s->y + i0, w.tv, s->zcap(),
                              s->zscratch_dev(), s->gz_dev(), first, s->stream), "dF/dZ contraction");
    if (s->gy_out) {  // bound outputs (include/mi_gp_sparse_data.h): dF/dy on the resident rows, dF/dX on the same weights
      if (!sparse_data_grad_chunk) { snprintf(s->err, sizeof(s->err), "mi_gp_sparse_bound_grad: the data-side gradients are not linked into this library"); return -1; }
      if (int r = sparse_data_grad_chunk(s, w, i0, cnt, sv)) return r;
    }
  }
  // Kuu's term through the symmetric contraction: W = -2 Guu and a zero alpha give sum_uv Guu_uv dK(Z,Z)_uv/dtheta (its gv and
  // jitter slots, 1/2 tr(-W), are not used)
  SCK(launch_grad_contract(s->spec, s->theta_dev(), s->Z, m, w.H, mp, w.zero, s->part_sym_dev(), s->gsym_dev(), s->stream), "Kuu's contraction");
  if (s->zcap() > 0) {
    // Kuu's term of dF/dZ through dLML/dX's kernel over Z: with a zero alpha its weight is -W_uv = 2 Guu_uv, read from the lower
    // triangle, and row and column of the symmetric sum contribute equally -- 2 sum_v Guu_uv dK(Z,Z)_uv/dz_u.  Then gz += that.
    SCK(launch_grad_x(s->spec, s->theta_dev(), s->Z, m, w.H, mp, w.zero, s->gzsym_dev(), grad_x_splits(m, d) > 1 ? s->zscratch_dev() : nullptr,
                      s->stream), "Kuu's dF/dZ");
    SCK(launch_sparse_zgrad_add(s->gzsym_dev(), 1, 0, s->zlen(), s->gz_dev(), 0, s->stream), "dF/dZ sum");
  }
  // (with dF/dZ the copy runs on over yy and the pivot words, which pass 1 has downloaded already, to the end of gz)
  SCK(hipMemcpyAsync(s->host + P, s->gacc_dev(), sizeof(double) * (s->zcap() > 0 ? 2 * P + 20 + s->zlen() : 2 * P + 16), hipMemcpyDeviceToHost,
                     s->stream), "gradient download");
  SCK(hipStreamSynchronize(s->stream), "stream sync");
  const double* ga = s->host + P;
  const double* gs = s->host + 2 * P;
  const double* sc = s->host + 3 * P;  // [1] tr Psi, [2] |c|^2; [8 + 3] |a^|^2, [8 + 4] tr B^-1
  const double yy = s->host[3 * P + 16];
  double dkv[MAX_KERN];
  const double kappa = (double)n * prior_diag(s->spec, theta, dkv);
  for (int k = 0; k < P - 2; ++k) grad_out[k] = ga[k] + gs[k];
  for (int c = 0; c < nk; ++c) grad_out[nk * d + c] -= (double)n / (2.0 * sv) * dkv[c];
  grad_out[P - 2] = -(double)n / (2.0 * sv) + yy / (2.0 * sv * sv) + (kappa - sc[1]) / (2.0 * sv * sv) + ((double)m - sc[12]) / (2.0 * sv) -
                    (sc[2] + sc[11]) / (2.0 * sv);
  grad_out[P - 1] = 0.0;  // jitter is a constant of the fit
  if (s->zcap() > 0) memcpy(grad_out + P, s->host + 3 * P + 20, sizeof(double) * s->zlen());
  return 0;
}

static int check_call(mi_gp_sparse* s, const double* theta, const char* entry) {
  if (!s) { snprintf(g_sparse_err, sizeof(g_sparse_err), "%s: null object", entry); return -1; }
  if (!theta) { snprintf(s->err, sizeof(s->err), "%s: null theta", entry); return -1; }
  if (const char* why = theta_error(s, theta)) { snprintf(s->err, sizeof(s->err), "%s: %s", entry, why); return -1; }
  if (!s->have_data) { snprintf(s->err, sizeof(s->err), "%s: call mi_gp_sparse_set_data first", entry); return -1; }
  return 0;
}

extern "C" int mi_gp_sparse_bound_grad(mi_gp_sparse* s, const double* theta_host, double* bound, double* grad_out) {
  if (int r = check_call(s, theta_host, "mi_gp_sparse_bound_grad")) return r;
  if (!bound) { snprintf(s->err, sizeof(s->err), "mi_gp_sparse_bound_grad: null bound"); return -1; }
  s->factored = false;
  if (grad_out)
    for (long k = 0; k < s->P + s->zlen(); ++k) grad_out[k] = 0.0;
  int r = pass_one(s, theta_host, bound);
  if (r == 0 && grad_out) {
    r = gradient(s, theta_host, grad_out);
    if (r != 0) *bound = -INFINITY;
  }
  if (r > 0 && grad_out && s->gy_out) {  // a bad pivot zeroes the bound data-side outputs too
    SCK(hipMemsetAsync(s->gy_out, 0, sizeof(double) * (size_t)s->n, s->stream), "dF/dy reset");
    if (s->gx_out) SCK(hipMemsetAsync(s->gx_out, 0, sizeof(double) * (size_t)s->n * s->d, s->stream), "dF/dX reset");
    SCK(hipStreamSynchronize(s->stream), "stream sync");
  }
  return r;
}

extern "C" int mi_gp_sparse_factor(mi_gp_sparse* s, const double* theta_host) {
  if (int r = check_call(s, theta_host, "mi_gp_sparse_factor")) return r;
  s->factored = false;
  double bound;
  const int r = pass_one(s, theta_host, &bound);
  if (r == 0) {
    s->factored = true;
    s->fac_s = theta_host[s->P - 2] + theta_host[s->P - 1];
    s->fac_kdiag = prior_diag(s->spec, theta_host, nullptr);
  }
  return r;
}

extern "C" int mi_gp_sparse_predict(mi_gp_sparse* s, const double* Xnew_dev, int mq, double* mean_dev, double* var_dev, int pred_noise) {
  if (!s) { snprintf(g_sparse_err, sizeof(g_sparse_err), "mi_gp_sparse_predict: null object"); return -1; }
  if (!Xnew_dev || !mean_dev || !var_dev || mq <= 0) { snprintf(s->err, sizeof(s->err), "mi_gp_sparse_predict: null buffer or mq <= 0"); return -1; }
  if (!s->have_data || !s->factored) { snprintf(s->err, sizeof(s->err), "mi_gp_sparse_predict: call mi_gp_sparse_factor first"); return -1; }
  const SparseWork w = sparse_layout(s->work, s->mp, s->chunk);
  const int mp = s->mp;
  SCK(hipSetDevice(s->cfg.device), "hipSetDevice");
  for (long q0 = 0; q0 < mq; q0 += s->chunk) {
    const int cq = (int)std::min<long>(s->chunk, mq - q0), rows_c = pad128(cq);
    SCK(chunk_rows(s, w, Xnew_dev + q0 * s->d, cq, rows_c), "query rows");  // a* = L^-1 k(Z, x*)
    SCK(hipMemcpyAsync(w.Tc, w.Wc, sizeof(double) * (size_t)rows_c * mp, hipMemcpyDeviceToDevice, s->stream), "copy rows");
    SCK(trsm_blocks(w.Bm, mp, w.dinvB, w.Tc, mp, rows_c, 0, s->ntm, s->stream), "second solve");  // b* = LB^-1 a*
    SCK(launch_sparse_predict_reduce(w.Wc, w.Tc, mp, w.cvec, s->m, cq, s->fac_kdiag, pred_noise ? s->fac_s : 0.0, mean_dev + q0,
                                     var_dev + q0, s->stream), "predict reduce");
  }
  SCK(hipStreamSynchronize(s->stream), "stream sync");
  return 0;
}
