// sched_trace: what one handle-level evaluation ENQUEUES, without a device.
//
// Links the host-only objects of api_gp.hip and gp_sched.hip against the recording stand-ins of this directory.  The handle is
// made by the real mi_gp_create / mi_gp_set_option / mi_gp_set_data / mi_gp_set_batch, so every default and every refusal is the
// library's; the evaluation goes through the real entry point.  Output: JSON lines -- a "config" record, a "begin" record, one
// record per enqueued operation in enqueue order, an "end" record with the entry point's return value.
//
//   sched_trace N D BATCH ENTRY PANEL_TILES [ID=VALUE ...]
//   sched_trace --file LIST        (one such argument list per line)
//
// ENTRY: lml | factor | lml_grad | lml_batch | factor_batch | lml_grad_batch.  ID: an option id of mi_gp_set_option, or `prof`
// (mi_gp_set_profiling).  BATCH: problems of a batch entry point (ignored by the single ones).
#include "trace_rec.h"
#include "../../andvaranaut_amd/csrc/gp_handle.h"
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

static void name_scratch(const Scratch& s, const char* prefix) {
  const std::string p = prefix;
  trace::name_range(s.theta_dev, (p + "theta").c_str(), 8);
  trace::name_range(s.dinv_dev, (p + "dinv").c_str(), 8);
  trace::name_range(s.alpha_dev, (p + "alpha").c_str(), 8);
  trace::name_range(s.part_dev, (p + "part").c_str(), 8);
  trace::name_range(s.info_dev, (p + "info").c_str(), 4);
  trace::name_range(s.lr_part_dev, (p + "lr_part").c_str(), 8);
  trace::name_range(s.lr_sync_dev, (p + "lr_sync").c_str(), 4);
  trace::name_range(s.grad_host, (p + "grad_host").c_str(), 8);
  trace::name_range(s.out_host, (p + "out_host").c_str(), 8);
  trace::name_range(s.theta_host, (p + "theta_host").c_str(), 8);
}

static double* dev_doubles(size_t count, const char* name) {
  void* p = nullptr;
  (void)hipMalloc(&p, sizeof(double) * count);
  trace::name_range(p, name, 8);
  return static_cast<double*>(p);
}

static int fail(const char* what, const char* why) {
  char b[400];
  snprintf(b, sizeof(b), "{\"k\":\"error\",\"what\":\"%s\",\"why\":\"%s\"}", what, why ? why : "");
  trace::emit_line(b);
  return 2;
}

static int run(const std::vector<std::string>& a) {
  if (a.size() < 5) return fail("usage", "N D BATCH ENTRY PANEL_TILES [ID=VALUE ...]");
  const int n = atoi(a[0].c_str()), d = atoi(a[1].c_str()), nbatch = atoi(a[2].c_str()), panel = atoi(a[4].c_str());
  const std::string entry = a[3];
  const bool batched = entry.size() > 6 && entry.compare(entry.size() - 6, 6, "_batch") == 0;
  const int what = entry.compare(0, 8, "lml_grad") == 0 ? 2 : entry.compare(0, 6, "factor") == 0 ? 1 : entry.compare(0, 3, "lml") == 0 ? 0 : -1;
  if (what < 0) return fail("entry", entry.c_str());
  if (batched && nbatch < 1) return fail("batch", "a batch entry point needs BATCH >= 1");

  trace::recording = false;
  mi_gp_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.n = n;
  cfg.d = d;
  cfg.nkern = 1;
  cfg.kernel_ids[0] = MI_GP_RBF;
  cfg.panel_tiles = panel;
  mi_gp_handle* h = nullptr;
  if (mi_gp_create(&cfg, &h) != 0) return fail("mi_gp_create", mi_gp_last_global_error());
  trace::name_range(h->sig_dev, "sig", 4);
  name_scratch(h->one, "one.");

  std::string refused = "[";
  for (size_t i = 5; i < a.size(); ++i) {
    const size_t eq = a[i].find('=');
    if (eq == std::string::npos) { mi_gp_destroy(h); return fail("option", a[i].c_str()); }
    const std::string id = a[i].substr(0, eq);
    const int value = atoi(a[i].c_str() + eq + 1);
    const int r = id == "prof" ? mi_gp_set_profiling(h, value) : mi_gp_set_option(h, atoi(id.c_str()), value);
    if (r != 0) { refused += (refused.size() > 1 ? ",\"" : "\"") + a[i] + "\""; }
  }
  refused += "]";

  const long np = mi_gp_padded_n(h), lda = np;
  mi_gp_buffers buf;
  buf.X_dev = dev_doubles((size_t)n * d, "X");
  buf.y_dev = dev_doubles(n, "y");
  buf.K_dev = dev_doubles((size_t)(np + 128) * lda, "K");
  buf.Z_dev = dev_doubles((size_t)np * lda, "Z");
  buf.W_dev = dev_doubles((size_t)np * lda, "W");
  buf.lda = lda;
  int rc = mi_gp_set_data(h, &buf);
  mi_gp_batch_buffers bb;
  memset(&bb, 0, sizeof(bb));
  if (rc == 0 && batched) {
    bb.stride_k = (np + 128) * lda;
    bb.stride_zw = np * lda;
    bb.count = nbatch;
    bb.K_dev = dev_doubles((size_t)nbatch * bb.stride_k, "bK");
    bb.Z_dev = dev_doubles((size_t)nbatch * bb.stride_zw, "bZ");
    bb.W_dev = dev_doubles((size_t)nbatch * bb.stride_zw, "bW");
    rc = mi_gp_set_batch(h, &bb);
    name_scratch(h->batch, "batch.");
  }
  int ret = -100;
  if (rc == 0) {
    std::ostringstream c;
    c << "{\"k\":\"config\",\"n\":" << n << ",\"d\":" << d << ",\"np\":" << np << ",\"ntc\":" << np / 128 << ",\"lda\":" << lda
      << ",\"nb\":" << (batched ? nbatch : 1) << ",\"batched\":" << (batched ? 1 : 0) << ",\"entry\":\"" << entry << "\",\"what\":" << what
      << ",\"panel_tiles\":" << panel << ",\"sig_slots\":" << SIG_SLOTS << ",\"minv_elems\":" << MINV_ELEMS << ",\"stride_k\":" << bb.stride_k
      << ",\"stride_zw\":" << bb.stride_zw << ",\"refused\":" << refused << ",\"options\":{";
    const int ids[] = {0, 2, 4, 5, 6, 7, 8, 9, 14, 16, 18, 19, 20, 21, 26, 27, 28, 30, 31, 32, 35, 37, 38, 40, 45, 46, 47};
    bool first = true;
    for (int id : ids) {
      int v = 0;
      if (mi_gp_get_option(h, id, &v) != 0) continue;
      c << (first ? "" : ",") << "\"" << id << "\":" << v;
      first = false;
    }
    c << "}}";
    trace::emit_line(c.str());
    const int ntheta = mi_gp_num_theta(h);
    std::vector<double> theta((size_t)ntheta * (batched ? nbatch : 1), 1.0), grad(theta.size()), lml(batched ? nbatch : 1);
    std::vector<int> info(batched ? nbatch : 1);
    trace::emit_line("{\"k\":\"begin\"}");
    trace::recording = true;
    if (!batched) ret = what == 0 ? mi_gp_lml(h, theta.data(), lml.data()) : what == 1 ? mi_gp_factor(h, theta.data())
                                                                                       : mi_gp_lml_grad(h, theta.data(), lml.data(), grad.data());
    else ret = what == 0 ? mi_gp_lml_batch(h, nbatch, theta.data(), lml.data(), info.data())
             : what == 1 ? mi_gp_factor_batch(h, nbatch, theta.data(), info.data())
                         : mi_gp_lml_grad_batch(h, nbatch, theta.data(), lml.data(), grad.data(), info.data());
    trace::recording = false;
    double t[14] = {};
    mi_gp_timers(h, t, 14);
    std::ostringstream e;
    e.precision(17);
    e << "{\"k\":\"end\",\"ret\":" << ret << ",\"n_gemm\":" << t[6] << ",\"gemm_flops\":" << t[5] << "}";
    trace::emit_line(e.str());
  } else {
    fail("bind", mi_gp_last_error(h));
  }
  mi_gp_destroy(h);
  (void)hipFree((void*)buf.X_dev); (void)hipFree((void*)buf.y_dev); (void)hipFree(buf.K_dev); (void)hipFree(buf.Z_dev); (void)hipFree(buf.W_dev);
  (void)hipFree(bb.K_dev); (void)hipFree(bb.Z_dev); (void)hipFree(bb.W_dev);
  return rc != 0 ? 2 : ret < 0 ? 1 : 0;
}

int main(int argc, char** argv) {
  int worst = 0;
  if (argc == 3 && std::string(argv[1]) == "--file") {
    std::ifstream in(argv[2]);
    if (!in) { fprintf(stderr, "sched_trace: cannot read %s\n", argv[2]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ls(line);
      std::vector<std::string> a;
      for (std::string w; ls >> w;) a.push_back(w);
      if (a.empty()) continue;
      const int r = run(a);
      if (r > worst) worst = r;
    }
  } else {
    worst = run(std::vector<std::string>(argv + 1, argv + argc));
  }
  trace::flush();
  return worst;
}
