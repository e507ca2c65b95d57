// tests/batch_host/harness.cpp — per-instance source tables on the CPU (TEST INFRASTRUCTURE).
//
// The emulator (tests/emul/emul.cpp) and the reference-order harness (tests/exact_host/harness.cpp) are compiled into this
// translation unit unchanged; the two entry points below set up a run the way theirs do and add what they cannot set:
// SpiceyRun::src_stride, the distance between the instances' source tables (0 = one shared table).  The phase code is the
// HIP kernels' own (tran_exec.h, exact_exec.h).  Never loaded by spicey_amd/: libspicey_hip.so has no CPU path.
#include "../emul/emul.cpp"
#include "../exact_host/harness.cpp"

// v1 (rmax < 0) or v2 (rmax >= 0 resident slots, hybrid: the hybrid workspace layout) with K interleaved instances;
// status [ceil(n_inst / K)][4] = the workgroups' {code, inst, step, iter}.
extern "C" int32_t spicey_batch_emul_run(const SpiceyDesc *d, int32_t K, int32_t T, int32_t rmax, int32_t hybrid, int64_t steps, double dt,
                                         const double *src, int64_t src_stride, double *out_v, double *out_i, int32_t *iters, double *C_vprev,
                                         double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t *status) {
  HostProgram hp;
  std::string err;
  const bool want_hyb = hybrid && rmax >= 0 && K == 1;
  int32_t rc = spicey_build_program(d, hp, err, true, 0, K == 1, want_hyb);
  if (rc != SPICEY_OK) return rc;
  SpiceyProg P = hp.bind(hp.blob.data());
  if ((want_hyb && !P.hybrid) || hp.structurally_singular || P.nFronts > 0) return SPICEY_ERR_BAD_DESC;
  if (T <= 0 || (T & 63) || rmax > 16 || (rmax >= 0 && (!P.has16 || K > 2))) return SPICEY_ERR_BAD_DESC;
  const int ni = d->n_inst;
  SpiceyRun R{};
  R.n_inst = ni; R.want_currents = out_i != nullptr; R.steps = steps; R.dt = dt;
  R.R_val = d->R_val; R.C_val = d->C_val; R.L_val = d->L_val;
  R.S_ron = d->S_ron; R.S_roff = d->S_roff; R.S_von = d->S_von; R.S_voff = d->S_voff;
  R.D_is = d->D_is; R.D_n = d->D_n;
  R.C_vprev = C_vprev; R.L_iprev = L_iprev; R.D_vdprev = D_vdprev; R.S_ison = S_ison;
  std::vector<double> gstat((size_t)ni * P.nGstat), statv((size_t)ni * P.nLU), rcoef((size_t)ni * (P.nRhsIdx + 1));
  std::vector<double> dpar((size_t)ni * (P.nD + 1) * 2);
  R.gstat = gstat.data(); R.statv = statv.data(); R.rcoef = rcoef.data(); R.dpar = dpar.data();
  R.src = src; R.src_stride = src_stride; R.out_v = out_v; R.out_i = out_i; R.iters = iters;
  const int ngroups = (ni + K - 1) / K;
  std::vector<unsigned long long> solves(ngroups);
  R.status = status; R.solves = solves.data();
  std::vector<double> hybG, hybUG;
  if (P.hybrid) {
    hybG.assign((size_t)ni * (size_t)P.nLU, 0.0);
    hybUG.assign((size_t)ni * (size_t)(P.nU + P.nGdyn + 1), 0.0);
    R.hyb_G = hybG.data(); R.hyb_ug = hybUG.data();
  }
  switch (K) {
    case 1: run_groups<1>(hp, P, R, T, false, rmax); break;
    case 2: run_groups<2>(hp, P, R, T, false, rmax); break;
    case 4: run_groups<4>(hp, P, R, T, false, rmax); break;
    default: return SPICEY_ERR_BAD_DESC;
  }
  for (int g = 0; g < ngroups; g++)
    if (status[(size_t)g * 4]) return SPICEY_ERR_SINGULAR;
  return SPICEY_OK;
}

// The reference-order engine, every instance with its own workspace; status [n_inst][4].
extern "C" int32_t spicey_batch_exact_run(const SpiceyDesc *d, int32_t T, int64_t steps, double dt, const double *src, int64_t src_stride,
                                          double *out_v, double *out_i, int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev,
                                          int32_t *S_ison, int32_t *status) {
  LaunchPlan plan;
  HostExactProg xp;
  std::string err;
  int32_t rc = plan_of(d, T, 0, plan, xp, err);
  if (rc != SPICEY_OK) return rc;
  const SpiceyExactProg P = xp.bind(xp.blob.data());
  const int ni = d->n_inst;
  std::vector<unsigned long long> solves((size_t)ni), skipc((size_t)ni);
  SpiceyRun R{};
  R.n_inst = ni; R.steps = steps; R.dt = dt;
  R.R_val = d->R_val; R.C_val = d->C_val; R.L_val = d->L_val;
  R.S_ron = d->S_ron; R.S_roff = d->S_roff; R.S_von = d->S_von; R.S_voff = d->S_voff;
  R.D_is = d->D_is; R.D_n = d->D_n;
  R.C_vprev = C_vprev; R.L_iprev = L_iprev; R.D_vdprev = D_vdprev; R.S_ison = S_ison;
  R.src = src; R.src_stride = src_stride; R.out_v = out_v; R.out_i = out_i; R.iters = iters;
  R.status = status; R.solves = solves.data(); R.skip_risk = skipc.data();
  std::vector<double> ws;
  int32_t scal[8];
  for (int inst = 0; inst < ni; inst++) {
    ws.assign((size_t)P.ws_doubles, NAN);
    SerialExec ex{plan.T, false};
    spicey_exact_run(ex, P, R, ws.data(), scal, inst, inst);
  }
  for (int g = 0; g < ni; g++)
    if (status[(size_t)g * 4]) return SPICEY_ERR_SINGULAR;
  return SPICEY_OK;
}
