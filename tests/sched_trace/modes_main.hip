// sched_modes: the handle's mode options (48-57 of mi_gp_set_option) on the host, without a device.
//
// Links the same objects and stand-ins as sched_trace (trace_main.hip), with or without mode_standin.hip: without it every weak
// mode function of gp_handle.h is null and every "not part of this build" refusal fires; with it the modes are accepted and the
// entry points dispatch into the stand-ins.  Runs a script of calls, one per line:
//
//   handle N D | set ID VALUE | get ID | factor | lml_grad | predict_grad | predict_cov | reserve CAP
//
// `handle` replaces the current handle by a fresh one.  After every other call one JSON record: the call, its return code (and the
// value of a `get`), mi_gp_last_error's text, options 48-57, the resident-state flags and whether the outputs' block is allocated.
//
//   sched_modes SCRIPT
#include "trace_rec.h"
#include "../../andvaranaut_amd/csrc/gp_handle.h"
#include <fstream>
#include <sstream>
#include <string>

// (the record of the parent commit, tests/golden/mode_options_parent.json, was built with -DMULTI_BLOCK naming the block as that
// commit's handle did)
#ifndef MULTI_BLOCK
#define MULTI_BLOCK(h) (h)->blocks[BLK_MULTI]
#endif
CapBlock& modes_multi_block(mi_gp_handle* h) { return MULTI_BLOCK(h); }

namespace {

struct Session {
  mi_gp_handle* h = nullptr;
  mi_gp_buffers buf = {};
  long ldw = 0;
  double *Xnew = nullptr, *work = nullptr, *out[4] = {};

  static double* dev(size_t count) {
    void* p = nullptr;
    (void)hipMalloc(&p, sizeof(double) * count);
    return static_cast<double*>(p);
  }
  void close() {
    if (!h) return;
    mi_gp_destroy(h);
    h = nullptr;
    for (void* p : {(void*)buf.X_dev, (void*)buf.y_dev, (void*)buf.K_dev, (void*)buf.Z_dev, (void*)buf.W_dev, (void*)Xnew, (void*)work})
      (void)hipFree(p);
    for (double* p : out) (void)hipFree(p);
  }
  // a fresh handle on buffers with room for 256 more points (reserve) and 128 outputs (option 51); false: the script ends
  bool open(int n, int d) {
    close();
    mi_gp_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.n = n;
    cfg.d = d;
    cfg.nkern = 1;
    cfg.kernel_ids[0] = MI_GP_RBF;
    if (mi_gp_create(&cfg, &h) != 0) return false;
    const long lda = mi_gp_padded_n(h) + 256;
    buf.X_dev = dev((size_t)lda * d);
    buf.y_dev = dev((size_t)128 * lda);
    buf.K_dev = dev((size_t)(lda + 128) * lda);
    buf.Z_dev = dev((size_t)lda * lda);
    buf.W_dev = dev((size_t)lda * lda);
    buf.lda = lda;
    ldw = lda;
    Xnew = dev((size_t)16 * d);
    work = dev((size_t)256 * ldw);
    for (double*& p : out) p = dev((size_t)128 * 128);
    return mi_gp_set_data(h, &buf) == 0;
  }
};

std::string json_text(const char* s) {
  std::string o = "\"";
  for (; *s; ++s) {
    if (*s == '"' || *s == '\\') o += '\\';
    o += *s;
  }
  return o + "\"";
}

void record(mi_gp_handle* h, const std::string& call, int ret, const int* got) {
  std::ostringstream r;
  r << "{\"k\":\"call\",\"call\":" << json_text(call.c_str()) << ",\"ret\":" << ret;
  if (got) r << ",\"value\":" << *got;
  r << ",\"err\":" << json_text(mi_gp_last_error(h)) << ",\"options\":[";
  for (int id = 48; id <= 57; ++id) {
    int v = 0;
    const int rc = mi_gp_get_option(h, id, &v);
    r << (id > 48 ? "," : "");
    if (rc == 0) r << v;
    else r << "null";
  }
  r << "],\"factored\":" << h->factored << ",\"have_u\":" << h->have_u << ",\"have_kinv\":" << h->have_kinv
    << ",\"b_cond_k\":" << h->b_cond_k << ",\"multi\":" << (modes_multi_block(h).p != nullptr) << "}";
  trace::emit_line(r.str());
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: sched_modes SCRIPT\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "sched_modes: cannot read %s\n", argv[1]); return 2; }
  trace::recording = false;  // (the launches of an evaluation are sched_trace's subject; the mode stand-ins write their own lines)
  Session s;
  std::string line;
  int status = 0;
  while (status == 0 && std::getline(in, line)) {
    std::istringstream ls(line);
    std::string op;
    long a = 0, b = 0;
    if (!(ls >> op)) continue;
    ls >> a >> b;
    if (op == "handle") {
      if (!s.open((int)a, (int)b)) { fprintf(stderr, "sched_modes: no handle for `%s`\n", line.c_str()); status = 2; }
      continue;
    }
    if (!s.h) { fprintf(stderr, "sched_modes: `%s` before a handle\n", line.c_str()); status = 2; break; }
    mi_gp_handle* h = s.h;
    std::vector<double> theta((size_t)mi_gp_num_theta(h), 1.0), grad(theta.size());
    double lml = 0.0;
    int got = 0;
    if (op == "set") record(h, line, mi_gp_set_option(h, (int)a, (int)b), nullptr);
    else if (op == "get") { const int r = mi_gp_get_option(h, (int)a, &got); record(h, line, r, &got); }
    else if (op == "factor") record(h, line, mi_gp_factor(h, theta.data()), nullptr);
    else if (op == "lml_grad") record(h, line, mi_gp_lml_grad(h, theta.data(), &lml, grad.data()), nullptr);
    else if (op == "predict_grad")
      record(h, line, mi_gp_predict_grad(h, s.Xnew, 4, s.work, s.ldw, s.out[0], s.out[1], 0, s.out[2], s.out[3]), nullptr);
    else if (op == "predict_cov") record(h, line, mi_gp_predict_cov(h, s.Xnew, 4, s.work, s.ldw, s.out[0], s.out[1], 128, 0), nullptr);
    else if (op == "reserve") record(h, line, mi_gp_reserve(h, (int)a), nullptr);
    else { fprintf(stderr, "sched_modes: unknown call `%s`\n", line.c_str()); status = 2; }
  }
  s.close();
  trace::flush();
  return status;
}
