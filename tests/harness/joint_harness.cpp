// TEST HARNESS (tests/ only): exposes the product's joint step logic (csrc/sba_joint_solver.hpp, header-only, no HIP) so
// that it can be driven on the CPU with numpy-emulated device passes.
#include "../../spherical_bundle_adjuster_amd/csrc/sba_joint_solver.hpp"
#include "../../spherical_bundle_adjuster_amd/csrc/sba_lm.hpp"

extern "C" {
void* joint_harness_create(const double* rot, const double* tran, const sba_lm_options* opt) {
  sba::JointSolver* s = new sba::JointSolver();
  s->start(rot, tran, *opt);
  return s;
}
void joint_harness_destroy(void* h) { delete static_cast<sba::JointSolver*>(h); }
int joint_harness_done(void* h) { return static_cast<sba::JointSolver*>(h)->done() ? 1 : 0; }
int joint_harness_status(void* h) { return static_cast<sba::JointSolver*>(h)->status(); }
// out21: kind, first, radius, rot[3], tran[3], delta_c[6], rot_cand[3], tran_cand[3]
void joint_harness_request(void* h, double* out21) {
  const sba::JointPassRequest& r = static_cast<sba::JointSolver*>(h)->request();
  out21[0] = r.kind; out21[1] = r.first ? 1.0 : 0.0; out21[2] = r.radius;
  for (int a = 0; a < 3; ++a) { out21[3 + a] = r.rot[a]; out21[6 + a] = r.tran[a]; out21[15 + a] = r.rot_cand[a]; out21[18 + a] = r.tran_cand[a]; }
  for (int a = 0; a < 6; ++a) out21[9 + a] = r.delta_c[a];
}
void joint_harness_feed(void* h, const double* row) { static_cast<sba::JointSolver*>(h)->feed(row); }
int joint_harness_take_candidate(void* h) { return static_cast<sba::JointSolver*>(h)->take_candidate() ? 1 : 0; }
void joint_harness_result(void* h, double* rot, double* tran, sba_lm_summary* s) {
  const sba::JointSolver* j = static_cast<sba::JointSolver*>(h);
  for (int a = 0; a < 3; ++a) { rot[a] = j->rot()[a]; tran[a] = j->tran()[a]; }
  *s = j->summary();
}
void joint_harness_default_options(sba_lm_options* o) { sba::lm_default_options(o); o->tran_param = SBA_TRAN_SPHERE; }
int joint_harness_row_layout(int* out5) {
  out5[0] = sba::JOINT_OUT_S; out5[1] = sba::JOINT_OUT_GS; out5[2] = sba::JOINT_OUT_GDMAX; out5[3] = sba::JOINT_OUT_COUNT; out5[4] = sba::JOINT_ROW;
  return 0;
}
}
