// tests/top_host/harness.cpp — CPU view of the launch plan's decision for the register-exchange top (TEST INFRASTRUCTURE ONLY).
//
// Compiles launch_plan.cpp and symbolic.cpp unchanged.  The form itself (tran_v2_run.h: TR) is GPU code — host executors
// run spicey_pcr_stage whatever the build — so what is held here is which runs take it: spicey_create's plan for a real
// circuit, and the decision function for a synthetic top.
#include <cstring>
#include <string>

#include "../../spicey_amd/csrc/launch_plan.h"

// spicey_create's plan on a device of `ncu` CUs (knobs from the environment, as there), and what a run of `steps` steps on
// such a handle launches: out13 = {top_regs, addr, ready, packed, fresh, threads, inst_per_wg, pcr_n, spicey_top_stages,
// spicey_addr_run, spicey_top_regs_run, lds_bytes, pcr_level}
extern "C" int32_t spicey_trhost_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t steps, int64_t *out13) {
  const SpiceyOptions o = opt ? *opt : SpiceyOptions{};
  const PlanDevice dev{[ncu](int, int *n, std::string &) { *n = ncu; return (int32_t)SPICEY_OK; }, [](const SpiceyProg &, int, int) { return 1; }};
  HostProgram hp;
  HostResident hres;
  LaunchPlan plan;
  std::string msg;
  const int32_t rc = spicey_plan(d, o, spicey_read_knobs(), dev, hp, hres, plan, msg);
  if (rc != SPICEY_OK) return rc;
  SpiceyInfo info;
  fill_info(plan, hp, hres, o, &info);
  out13[0] = plan.top_regs; out13[1] = plan.addr; out13[2] = plan.ready; out13[3] = plan.packed; out13[4] = plan.fresh; out13[5] = plan.T; out13[6] = plan.K;
  out13[7] = info.pcr_rows; out13[8] = spicey_top_stages(info.pcr_rows); out13[9] = spicey_addr_run(plan, steps); out13[10] = spicey_top_regs_run(plan, steps);
  out13[11] = (int64_t)plan.lds_bytes; out13[12] = info.pcr_level;
  return SPICEY_OK;
}

// The decision for a SYNTHETIC top of pcr_n rows on build `shape` (an index into SPICEY_V2_SHAPES) of a plan whose `addr` is
// given, knobs from the environment.  out4 = {LaunchPlan::top_regs, spicey_top_stages, then for a plan with slots, ready
// and that addr: spicey_top_regs_run (10 000 steps), shape's `top_regs`}
extern "C" void spicey_trhost_decide(int32_t addr, int32_t pcr_n, int32_t shape, int64_t *out4) {
  LaunchPlan plan;
  plan.slots = true; plan.ready = true; plan.addr = addr != 0;
  plan.top_regs = spicey_plan_top_regs(plan.addr, pcr_n, shape, spicey_read_knobs());
  out4[0] = plan.top_regs; out4[1] = spicey_top_stages(pcr_n); out4[2] = spicey_top_regs_run(plan, 10000);
  out4[3] = (shape >= 0 && shape < SPICEY_V2_NSHAPES) ? SPICEY_V2_SHAPES[shape].top_regs : 0;
}

// the packed fresh shape's index in SPICEY_V2_SHAPES, the packed default shape's, the 1024-thread latency shape's
extern "C" void spicey_trhost_shapes(int32_t *out3) {
  out3[0] = spicey_v2_shape(512, true, false, true);
  out3[1] = spicey_v2_shape(512, true, false, false);
  out3[2] = spicey_v2_shape(1024, false, false, false);
}
