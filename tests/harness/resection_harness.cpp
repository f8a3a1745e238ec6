// TEST HARNESS (tests/ only): the host side of the spherical resection (csrc/sba_resection.hpp, header-only, no HIP) and the
// product's host LM (csrc/sba_lm.hpp) with a caller-supplied evaluator that fills a FULL sba_normal_eq -- the resection's H
// has no SBA_PACK_* form -- so that the row expansion, the DLT finish, the log map and the LM schedule run on the CPU.
#include "../../spherical_bundle_adjuster_amd/csrc/sba_lm.hpp"
#include "../../spherical_bundle_adjuster_amd/csrc/sba_resection.hpp"
#include "../../spherical_bundle_adjuster_amd/csrc/sba_rotation.hpp"

// eq45: H row-major (36), g (6), cost, sum_w, n_outlier
typedef int (*resection_eval_cb)(const double* rot, const double* tran, double* eq45, void* user);

extern "C" int resection_harness_lm_solve(double* rot, double* tran, const sba_lm_options* opt, resection_eval_cb cb, void* user,
                                          sba_lm_summary* summary) {
  auto evaluate = [&](const double r[3], const double t[3], sba_normal_eq* ne) -> bool {
    double eq[45];
    if (cb(r, t, eq, user) != 0) return false;
    for (int i = 0; i < 36; ++i) ne->H[i] = eq[i];
    for (int i = 0; i < 6; ++i) ne->g[i] = eq[36 + i];
    ne->cost = eq[42]; ne->sum_w = eq[43]; ne->n_outlier = eq[44];
    return true;
  };
  return sba::lm_solve(SBA_MODE_RT, rot, tran, *opt, evaluate, summary);
}

extern "C" void resection_harness_default_options(sba_lm_options* o) { sba::lm_default_options(o); }

// row32 (SBA_RESECT_* layout) -> eq45 as above, then n_behind
extern "C" void resection_harness_expand(const double* row32, double* eq46) {
  sba_normal_eq ne;
  double nb = 0.0;
  sba::resect_expand_row(row32, &ne, &nb);
  for (int i = 0; i < 36; ++i) eq46[i] = ne.H[i];
  for (int i = 0; i < 6; ++i) eq46[36 + i] = ne.g[i];
  eq46[42] = ne.cost; eq46[43] = ne.sum_w; eq46[44] = ne.n_outlier; eq46[45] = nb;
}

extern "C" int resection_harness_layout(int which) {
  const int v[] = {SBA_RESECT_H, SBA_RESECT_G, SBA_RESECT_COST, SBA_RESECT_SW, SBA_RESECT_NOUT, SBA_RESECT_NBEHIND, SBA_RESECT_SIZE};
  return which >= 0 && which < 7 ? v[which] : -1;
}

// info7: lambda1, lambda2, lambda12, sv[3], scale
extern "C" int resection_harness_dlt(const double* mom60, double count, double* rot, double* tran, double* info7) {
  sba_resection_guess_info info;
  const char* why = "";
  const int rc = sba::resect_dlt_finish(mom60, count, rot, tran, &info, &why);
  info7[0] = info.lambda1; info7[1] = info.lambda2; info7[2] = info.lambda12;
  for (int k = 0; k < 3; ++k) info7[3 + k] = info.sv[k];
  info7[6] = info.scale;
  return rc;
}

extern "C" void resection_harness_log(const double* R9, double* w3) { sba::rotation_log(R9, w3); }
extern "C" void resection_harness_rotation(const double* w3, double* R9) { sba::rotation_and_derivatives(w3, R9, nullptr); }
