// Stand-ins for the mode functions that api_gp.hip links weakly (gp_handle.h: api_loo, api_trend, api_multi, api_sweep, api_paths
// and api_design).  With this file in the link the mode options 48-57 are "part of this build"; every function writes a line
// naming itself and succeeds.  multi_factor also allocates the outputs' block, as the real one does: option 52 drops it.
#include "trace_rec.h"
#include "../../andvaranaut_amd/csrc/gp_handle.h"

CapBlock& modes_multi_block(mi_gp_handle* h);  // modes_main.hip

static void called(const char* fn) { trace::emit_line(std::string("{\"k\":\"mode\",\"fn\":\"") + fn + "\"}"); }

int loo_objective(mi_gp_handle*, double*, double*) { called("loo_objective"); return 0; }
int trend_objective(mi_gp_handle*, double*, double*) { called("trend_objective"); return 0; }
int trend_factor(mi_gp_handle*) { called("trend_factor"); return 0; }
hipError_t trend_predict_reduce(mi_gp_handle*, const double*, const double*, long, int, double*, double*, int) {
  called("trend_predict_reduce");
  return hipSuccess;
}
hipError_t trend_reserve(mi_gp_handle*, int) { called("trend_reserve"); return hipSuccess; }
int multi_objective(mi_gp_handle*, double*, double*) { called("multi_objective"); return 0; }
int multi_factor(mi_gp_handle* h) {
  called("multi_factor");
  CapBlock& b = modes_multi_block(h);
  if (!b.p && hipMalloc(&b.p, sizeof(double)) == hipSuccess) b.cap = h->cap;
  return 0;
}
hipError_t multi_predict_reduce(mi_gp_handle*, const double*, long, int, double*, double*, int) {
  called("multi_predict_reduce");
  return hipSuccess;
}
hipError_t multi_reserve(mi_gp_handle*, int) { called("multi_reserve"); return hipSuccess; }
int mean_sweep(mi_gp_handle*, const double*, int, double*, double*) { called("mean_sweep"); return 0; }
int path_sweep(mi_gp_handle*, const double*, int, double*, long, double*, int, double*) { called("path_sweep"); return 0; }
int design_select(mi_gp_handle*, const double*, int, double*, long, double*, double*, long, int) { called("design_select"); return 0; }
