// mi_gp_kfold (include/mi_gp.h): exact k-fold cross-validation at the theta of the last mi_gp_lml_grad, from the resident K^-1 and
// alpha = K^-1 y.  A consumer of resident state like mi_gp_logpdf: an entry point and a kernel file (kfold_f64.hip) of its own,
// the batched 128 x 128 leaf of the factorisation as it is.
#include <cstdint>
#include "gp_handle.h"

// ---------------------------------------------------------------- hold-out predictive of every fold
// For an index set I the conditional of the noisy observations y_I given all other points, at the same hyper-parameters, follows
// from the blocks of K^-1 alone (block inverse of K):
//   Sigma_I = (K^-1_II)^-1,   y_I - mu_I = Sigma_I alpha_I,
//   log p(y_I | y_-I) = -1/2 alpha_I^T Sigma_I alpha_I + 1/2 log det K^-1_II - |I|/2 log 2 pi.
// With C = chol(K^-1_II) and M = C^-1 from the leaf: Sigma_I = M^T M, t = M alpha_I, the quadratic form is |t|^2, the
// log-determinant term sum log C_ii.
// The work block for P folds per pass: fold_layout() (gp_handle.h).
extern "C" long mi_gp_kfold_work(int folds_per_pass, long total_idx) {
  return (folds_per_pass < 1 || total_idx < 1) ? -1 : fold_work_len(folds_per_pass, total_idx);
}

int fold_pass(mi_gp_handle* h, const FoldWork& w, int nfolds, const int* ptr_host, const int* idx_host,
              const std::function<hipError_t(int, int)>& step) {
  const hipStream_t st = h->stream;
  HCK(hipMemcpyAsync(w.idx, idx_host, sizeof(int) * ptr_host[nfolds], hipMemcpyHostToDevice, st), "index upload");
  HCK(hipMemcpyAsync(w.ptr, ptr_host, sizeof(int) * (nfolds + 1), hipMemcpyHostToDevice, st), "fold upload");
  for (int f0 = 0; f0 < nfolds; f0 += w.pass) {
    const int nf = nfolds - f0 < w.pass ? nfolds - f0 : w.pass;
    Batch bt;
    bt.nb = nf;
    bt.sK = bt.sdinv = MINV_ELEMS;
    bt.sinfo = 1;
    HCK(launch_kfold_gather(h->buf.W_dev, h->buf.lda, h->one.alpha_dev, h->buf.y_dev, w.idx, w.ptr, f0, nf, w.blocks, w.vecs, w.info,
                            st), "kfold_gather");
    HCK(launch_potrf_leaf128(w.blocks, 128, w.minv, 0, w.info + f0, st, nullptr, &bt), "kfold leaf");
    HCK(step(f0, nf), "fold step");
  }
  return 0;
}

namespace {
struct DevInts {  // the singleton path's index list and info words
  int* p = nullptr;
  ~DevInts() { (void)hipFree(p); }
};
}  // namespace

extern "C" int mi_gp_kfold(mi_gp_handle* h, int nfolds, const int* fold_ptr_host, const int* fold_idx_host, double* work_dev,
                           long work_len, double* logp_dev, double* mean_dev, double* var_dev, int* info_out) {
  if (!h) { set_global_error("mi_gp_kfold: null handle"); return -1; }
  if (int r = refuse_plain_model(h, "mi_gp_kfold")) return r;
  char why[160] = "";
  bool singletons = true;
  long total = 0;
  if (nfolds < 1) snprintf(why, sizeof(why), "nfolds >= 1 (got %d)", nfolds);
  else if (!fold_ptr_host || !fold_idx_host || !logp_dev) snprintf(why, sizeof(why), "null fold_ptr, fold_idx or logp buffer");
  else if (!mean_dev != !var_dev) snprintf(why, sizeof(why), "mean_dev and var_dev are given both or neither");
  else if (!h->have_kinv) snprintf(why, sizeof(why), "K^-1 is not resident: call mi_gp_lml_grad first");
  else if (fold_ptr_host[0] != 0) snprintf(why, sizeof(why), "fold_ptr[0] must be 0");
  else {
    std::vector<int> seen(h->n, -1);  // the last fold that held a point
    for (int f = 0; f < nfolds && !why[0]; ++f) {
      const long a = fold_ptr_host[f], s = (long)fold_ptr_host[f + 1] - a;
      if (s < 1 || s > 128) { snprintf(why, sizeof(why), "fold %d has %ld points (1 to 128)", f, s); break; }
      if (s != 1) singletons = false;
      for (long t = a; t < a + s; ++t) {
        const int i = fold_idx_host[t];
        if (i < 0 || i >= h->n) { snprintf(why, sizeof(why), "fold %d: index %d outside [0, %d)", f, i, h->n); break; }
        if (seen[i] == f) { snprintf(why, sizeof(why), "fold %d: index %d is repeated", f, i); break; }
        seen[i] = f;
      }
    }
    total = fold_ptr_host[nfolds];
  }
  long P = 0;
  if (!why[0] && !singletons) {
    // the most folds per pass whose work block fits work_len
    const long tail = fold_work_len(0, total), per_fold = fold_work_len(1, total) - tail;
    P = work_dev ? (work_len - tail) / per_fold : 0;
    if (!work_dev) snprintf(why, sizeof(why), "null work buffer");
    else if ((uintptr_t)work_dev & 15) snprintf(why, sizeof(why), "work_dev must be 16-byte aligned");
    else if (work_len < tail || P < 1)
      snprintf(why, sizeof(why), "work_len %ld is too small for one fold (mi_gp_kfold_work(1, %ld) = %ld)", work_len, total,
               mi_gp_kfold_work(1, total));
  }
  if (why[0]) { snprintf(h->err, sizeof(h->err), "mi_gp_kfold: %s", why); return -1; }
  HCK(hipSetDevice(h->device), "hipSetDevice");
  const hipStream_t st = h->stream;
  const double *W = h->buf.W_dev, *alpha = h->one.alpha_dev, *y = h->buf.y_dev;
  const long ld = h->buf.lda;
  std::vector<int> info(nfolds);
  if (singletons) {
    // leave-one-out: the closed form in one launch, on a scratch of the call's own (no work block)
    DevInts d;
    HCK(hipMalloc(&d.p, sizeof(int) * 2 * (size_t)nfolds), "kfold index list");
    HCK(hipMemcpyAsync(d.p, fold_idx_host, sizeof(int) * nfolds, hipMemcpyHostToDevice, st), "index upload");
    HCK(launch_kfold_loo(W, ld, alpha, y, d.p, nfolds, logp_dev, mean_dev, var_dev, d.p + nfolds, st), "kfold_loo");
    HCK(hipMemcpyAsync(info.data(), d.p + nfolds, sizeof(int) * nfolds, hipMemcpyDeviceToHost, st), "info download");
    HCK(hipStreamSynchronize(st), "stream sync");
  } else {
    if (P > nfolds) P = nfolds;
    const FoldWork w = fold_layout(work_dev, P, total, nfolds);
    const int r = fold_pass(h, w, nfolds, fold_ptr_host, fold_idx_host, [&](int f0, int nf) {
      return launch_kfold_moments(w.blocks, w.minv, w.vecs, w.ptr, w.info, f0, nf, logp_dev, mean_dev, var_dev, st);
    });
    if (r != 0) return r;
    HCK(hipMemcpyAsync(info.data(), w.info, sizeof(int) * nfolds, hipMemcpyDeviceToHost, st), "info download");
    HCK(hipStreamSynchronize(st), "stream sync");
    for (int f = 0; f < nfolds; ++f) info[f] = info[f] == INFO_OK ? 0 : info[f];
  }
  if (info_out)
    for (int f = 0; f < nfolds; ++f) info_out[f] = info[f];
  return 0;
}
