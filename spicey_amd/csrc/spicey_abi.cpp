// spicey_abi.cpp — the C-ABI of include/spicey_hip.h: handle management, uploads, launches, state, diagnostics and the
// multi-device handle (the reduced runs behind a launch are in reduced_abi.cpp, the handle-less device entry points in
// device_abi.cpp, what the three share in tran_handle.h).  Host code only (HIP runtime API); the kernels are in kernels.hip,
// the symbolic phase in symbolic.cpp.  There is NO CPU solve path in this library: without a HIP device every entry
// point that would compute returns SPICEY_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "tran_handle.h"
#include "fronts_exec_consts.h"

// (d: the descriptor's state; null: zeros)
static hipError_t upload_state(StateBufs &s, const SpiceyDesc *d, const SpiceyProg &P, size_t ni) {
  hipError_t e;
  if ((e = dev_upload(s.Cv, ni * P.nC, d ? d->C_vprev : nullptr)) != hipSuccess) return e;
  if ((e = dev_upload(s.Li, ni * P.nL, d ? d->L_iprev : nullptr)) != hipSuccess) return e;
  if ((e = dev_upload(s.Dv, ni * P.nD, d ? d->D_vdprev : nullptr)) != hipSuccess) return e;
  return dev_upload(s.Son, ni * P.nS, d ? d->S_ison : nullptr);
}
// Copies the kinds the program has, skipping a side's null pointers; async: ordered on `st`, else a blocking hipMemcpy.
static hipError_t copy_state(const StatePtrs &dst, const StatePtrs &src, const SpiceyProg &P, size_t ni, hipMemcpyKind kind, bool async,
                             hipStream_t st = nullptr) {
  const struct { void *d; const void *s; size_t bytes; } kinds[] = {{dst.Cv, src.Cv, ni * P.nC * sizeof(double)}, {dst.Li, src.Li, ni * P.nL * sizeof(double)},
                                                                    {dst.Dv, src.Dv, ni * P.nD * sizeof(double)}, {dst.Son, src.Son, ni * P.nS * sizeof(int32_t)}};
  for (const auto &k : kinds) {
    if (!k.d || !k.s || !k.bytes) continue;
    const hipError_t e = async ? hipMemcpyAsync(k.d, k.s, k.bytes, kind, st) : hipMemcpy(k.d, k.s, k.bytes, kind);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

thread_local std::string g_err;  // (tran_handle.h)

// ---- launch admission per device (include/spicey_hip.h, "Launch admission") ------------------------------------------
// A group-mode launch (G > 1 workgroups per instance that wait for one another inside the kernel) needs all its workgroups
// resident.  The host sizes it to at most one workgroup per CU, so that holds on an otherwise idle device; what must not
// happen is a second launch of this library taking CUs away while the group is starting, or two groups each holding some
// CUs and waiting for the rest.  Per device: `ev_group` = completion of the last group-mode launch; `ring` = completions of
// the recent launches that are not group-mode.  A group-mode launch first makes its stream wait for ev_group and for every
// ring event; any other launch waits for ev_group only (and for the ring slot it is about to reuse, which keeps "waiting
// for the ring" = "waiting for every earlier launch" when more than RING launches are in flight).  All of it is
// stream-ordered (hipStreamWaitEvent): nothing blocks on the host, so one thread may hold several launches in flight.
// The bookkeeping is skipped while no group-mode handle exists on the device; the first one to be created drains the
// device once (hipDeviceSynchronize) so that earlier, unrecorded launches are known to have finished.
namespace {
struct DeviceGate {
  static const int RING = 16;
  std::mutex mu;
  int group_handles = 0;
  hipEvent_t ev_group = nullptr;
  bool group_recorded = false;
  hipEvent_t ring[RING] = {};
  bool ring_used[RING] = {};
  int ring_next = 0;
};
DeviceGate &device_gate(int device) {
  static std::mutex m;
  static std::map<int, DeviceGate *> gates;  // (never freed: a gate may be touched by a handle destroyed at process exit)
  std::lock_guard<std::mutex> lk(m);
  DeviceGate *&g = gates[device];
  if (!g) g = new DeviceGate();
  return *g;
}
// with g.mu held and the device current; `st` is the launch stream.  Returns a HIP error or hipSuccess.
hipError_t gate_before_launch(DeviceGate &g, bool group, hipStream_t st, int *slot) {
  *slot = -1;
  if (!group && g.group_handles == 0) return hipSuccess;
  hipError_t e;
  if (g.group_recorded && (e = hipStreamWaitEvent(st, g.ev_group, 0)) != hipSuccess) return e;
  if (group) {
    for (int i = 0; i < DeviceGate::RING; i++)
      if (g.ring_used[i] && (e = hipStreamWaitEvent(st, g.ring[i], 0)) != hipSuccess) return e;
    return hipSuccess;
  }
  const int i = g.ring_next;
  if (!g.ring[i] && (e = hipEventCreateWithFlags(&g.ring[i], hipEventDisableTiming)) != hipSuccess) return e;
  if (g.ring_used[i] && (e = hipStreamWaitEvent(st, g.ring[i], 0)) != hipSuccess) return e;
  *slot = i;
  return hipSuccess;
}
hipError_t gate_after_launch(DeviceGate &g, bool group, hipStream_t st, int slot) {
  hipError_t e;
  if (group) {
    if (!g.ev_group && (e = hipEventCreateWithFlags(&g.ev_group, hipEventDisableTiming)) != hipSuccess) return e;
    if ((e = hipEventRecord(g.ev_group, st)) != hipSuccess) return e;
    g.group_recorded = true;
    for (int i = 0; i < DeviceGate::RING; i++) g.ring_used[i] = false;  // (this launch waited for all of them)
    return hipSuccess;
  }
  if (slot < 0) return hipSuccess;
  if ((e = hipEventRecord(g.ring[slot], st)) != hipSuccess) return e;
  g.ring_used[slot] = true;
  g.ring_next = (slot + 1) % DeviceGate::RING;
  return hipSuccess;
}
}  // namespace

extern "C" const char *spicey_version(void) { return "spicey_hip abi2 gfx950 (persistent LDS-resident sparse-LU transient kernel)"; }

extern "C" const char *spicey_last_error(SpiceyHandle *h) { return h ? h->err.c_str() : g_err.c_str(); }

extern "C" void spicey_destroy(SpiceyHandle *h) {
  if (!h) return;
  if (h->pending && h->last_stream) (void)hipStreamSynchronize(h->last_stream);
  if (h->gated) {
    DeviceGate &g = device_gate(h->device);
    std::lock_guard<std::mutex> lk(g.mu);
    g.group_handles--;
  }
  delete h;  // (events and stream, then every device buffer)
}

// per-instance element values and the state (live and as the descriptor carried it)
static int32_t upload_values(SpiceyHandle *h, const SpiceyDesc *desc) {
  const SpiceyProg &P = h->hp.hdr;
  const size_t ni = (size_t)h->plan.n_inst;
  HIPCHK(h, dev_upload(h->d_R, ni * P.nR, desc->R_val));
  HIPCHK(h, dev_upload(h->d_C, ni * P.nC, desc->C_val));
  HIPCHK(h, dev_upload(h->d_L, ni * P.nL, desc->L_val));
  HIPCHK(h, dev_upload(h->d_Sron, ni * P.nS, desc->S_ron));
  HIPCHK(h, dev_upload(h->d_Sroff, ni * P.nS, desc->S_roff));
  HIPCHK(h, dev_upload(h->d_Svon, ni * P.nS, desc->S_von));
  HIPCHK(h, dev_upload(h->d_Svoff, ni * P.nS, desc->S_voff));
  HIPCHK(h, dev_upload(h->d_Dis, ni * P.nD, desc->D_is));
  HIPCHK(h, dev_upload(h->d_Dn, ni * P.nD, desc->D_n));
  HIPCHK(h, upload_state(h->state, desc, P, ni));
  HIPCHK(h, upload_state(h->state0, desc, P, ni));
  return SPICEY_OK;
}

// the device side of a reference-order handle: stamp lists, argument structs, values and state, status words, workspace
static int32_t allocate_exact(SpiceyHandle *h, const SpiceyDesc *desc) {
  const LaunchPlan &pl = h->plan;
  const size_t ni = (size_t)pl.n_inst;
  spicey_build_exact(*desc, pl.xws, h->xp);
  HIPCHK(h, dev_upload(h->d_xblob, h->xp.blob.size(), h->xp.blob.data()));
  const SpiceyExactProg xd = h->xp.bind(h->d_xblob);
  HIPCHK(h, dev_upload(h->d_xprog, 1, &xd));
  HIPCHK(h, dev_upload(h->d_Rstruct, 1));
  if (const int32_t rc = upload_values(h, desc); rc != SPICEY_OK) return rc;
  HIPCHK(h, dev_upload(h->d_status, (size_t)pl.grid * 4));
  HIPCHK(h, dev_upload(h->d_solves, (size_t)pl.grid));
  if (h->opt.diagnostics & 1) HIPCHK(h, dev_upload(h->d_skip, ni));
  if (!pl.lds) {  // one n x (n + 1) slab (and the vectors beside it) per instance
    const size_t per = (size_t)pl.xws.doubles;
    if (per > (SIZE_MAX / sizeof(double)) / ni || h->d_xws.alloc(per * ni) != hipSuccess) {
      (void)hipGetLastError();
      char buf[256];
      snprintf(buf, sizeof(buf), "interpreter 3 (reference order): cannot allocate the global workspace of %zu instances x %zu bytes (n = %d: a dense n x (n + 1) matrix each)",
               ni, per * sizeof(double), h->hp.hdr.n);
      h->err = buf;
      return SPICEY_ERR_HIP;
    }
  }
  return h->q.create(h);
}

// the device side of a planned handle: program, argument structs, per-instance values and state, workspaces, stream, events
static int32_t allocate(SpiceyHandle *h, const SpiceyDesc *desc) {
  if (h->plan.interp == 3) return allocate_exact(h, desc);
  const SpiceyProg &P = h->hp.hdr;
  const LaunchPlan &pl = h->plan;
  const size_t ni = (size_t)pl.n_inst;
  HIPCHK(h, dev_upload(h->d_blob, h->hp.blob.size(), h->hp.blob.data()));
  h->dprog = h->hp.bind(h->d_blob);
  if (pl.interp == 2) {
    HIPCHK(h, dev_upload(h->d_res, h->hres.blob.size(), h->hres.blob.data()));
    h->dres = h->hres.bind(h->d_res);
    HIPCHK(h, dev_upload(h->d_Pstruct, 1, &h->dprog));
    HIPCHK(h, dev_upload(h->d_Qstruct, 1, &h->dres));
    HIPCHK(h, dev_upload(h->d_Rstruct, 1));
  }
  if (const int32_t rc = upload_values(h, desc); rc != SPICEY_OK) return rc;
  HIPCHK(h, dev_upload(h->d_gstat, ni * P.nGstat));
  HIPCHK(h, dev_upload(h->d_statv, ni * P.nLU));
  HIPCHK(h, dev_upload(h->d_rcoef, ni * (size_t)(P.nRhsIdx + 1)));
  HIPCHK(h, dev_upload(h->d_dpar, ni * (size_t)P.nD * 2));
  if (const size_t nz = spicey_zpar_doubles(pl, h->hp)) {
    // (a plan that folds the last factor level keeps that form's record table behind the record: program.h)
    std::vector<uint32_t> table;
    if (pl.top_fold && !spicey_top_fold_table(h->hp, h->hres.tail_n, table)) { h->err = "internal: the plan folds the last factor level, but the program has no table for it"; return SPICEY_ERR_BAD_DESC; }
    if (pl.top_fold && table.size() != SPICEY_TOP_FOLD_WORDS) { h->err = "internal: the table of the folded last factor level has the wrong size"; return SPICEY_ERR_BAD_DESC; }
    // (... and a plan whose Z stamps the next step keeps that form's table behind the fold's: tran_pt_layout.h)
    if (pl.stamp_fuse) {
      const int shape = spicey_v2_shape(pl.T, pl.packed, h->hp.hdr.hybrid != 0, pl.packed && h->hp.hdr.fresh_fill != 0);
      std::vector<uint32_t> fuse;
      if (!pl.top_fold || shape < 0 || !spicey_stamp_fuse_table(h->hp, h->hres.tail_n, pl.T, SPICEY_V2_SHAPES[shape].nsv, SPICEY_V2_SHAPES[shape].nel, fuse) ||
          fuse.size() != spicey_stamp_fuse_words(pl.T) || (fuse.size() & 1)) { h->err = "internal: the plan fuses the stamps into Z, but the program has no table for it"; return SPICEY_ERR_BAD_DESC; }
      table.insert(table.end(), fuse.begin(), fuse.end());
    }
    h->zpar_doubles = nz + table.size() * sizeof(uint32_t) / sizeof(double);
    HIPCHK(h, dev_upload(h->d_zpar, h->zpar_doubles));
    if (!table.empty()) HIPCHK(h, hipMemcpy((double *)h->d_zpar + nz, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  if (!pl.lds) HIPCHK(h, dev_upload(h->d_gW, (size_t)pl.grid * spicey_gw_doubles_per_wg(P, pl.K)));
  if (pl.G > 1) {
    HIPCHK(h, dev_upload(h->d_gsync, (size_t)pl.grid * SPICEY_GRP_SYNC_WORDS));
    HIPCHK(h, dev_upload(h->d_gflags, (size_t)pl.grid * 4));
    HIPCHK(h, upload_state(h->state_s, nullptr, P, ni));
  }
  if (P.nFronts > 0) {
    std::vector<uint32_t> first, list, owner((size_t)P.nFronts, 0u);
    spicey_build_front_schedule(h->hp, pl.G, first, list);
    for (int w = 0; w < pl.G; w++)
      for (uint32_t s2 = first[w]; s2 < first[w + 1]; s2++) owner[list[s2]] = (uint32_t)w;
    std::vector<uint32_t> all(first);
    all.insert(all.end(), list.begin(), list.end());
    all.insert(all.end(), owner.begin(), owner.end());
    HIPCHK(h, dev_upload(h->d_fs, all.size(), all.data()));
    HIPCHK(h, dev_upload(h->d_front_ws, (size_t)pl.grid * (size_t)P.front_ws));
    HIPCHK(h, dev_upload(h->d_front_flags, (size_t)pl.grid * 2 * (size_t)P.nFronts));
  }
  HIPCHK(h, dev_upload(h->d_status, (size_t)pl.grid * 4));
  HIPCHK(h, dev_upload(h->d_solves, (size_t)pl.grid));
  // (+ per-front event times behind the per-workgroup section timers)
  if (h->opt.profile) HIPCHK(h, dev_upload(h->d_prof, (size_t)pl.grid * pl.G * 72 + (size_t)pl.grid * 4 * (size_t)P.nFronts));
  if (P.hybrid) {
    HIPCHK(h, dev_upload(h->d_hybG, ni * (size_t)P.nLU));
    HIPCHK(h, dev_upload(h->d_hybUG, ni * (size_t)(P.nU + P.nGdyn)));
  }
  if (h->opt.diagnostics & 1) HIPCHK(h, dev_upload(h->d_skip, ni));
  if ((h->opt.diagnostics & 2) && P.nD > 0) HIPCHK(h, dev_upload(h->d_linvd, ni * P.nD));
  return h->q.create(h);
}

extern "C" int32_t spicey_create(const SpiceyDesc *desc, const SpiceyOptions *opt, SpiceyHandle **out) {
  if (!out) { g_err = "null out pointer"; return SPICEY_ERR_BAD_DESC; }
  *out = nullptr;
  SpiceyHandle *h = new SpiceyHandle();
  if (opt) h->opt = *opt;
  h->knobs = spicey_read_knobs();
  h->device = h->opt.device;
  Roctx range_create("spicey_create");
  const PlanDevice dev{spicey_open_device, spicey_grp_blocks_per_cu};
  int32_t rc = spicey_plan(desc, h->opt, h->knobs, dev, h->hp, h->hres, h->plan, h->err);
  if (rc == SPICEY_OK && h->plan.G > 1) {
    // the first group-mode handle on a device drains it once: launches enqueued before were not recorded (DeviceGate)
    DeviceGate &g = device_gate(h->device);
    std::lock_guard<std::mutex> lk(g.mu);
    if (g.group_handles++ == 0) (void)hipDeviceSynchronize();
    h->gated = true;
  }
  if (rc == SPICEY_OK) rc = allocate(h, desc);
  if (rc != SPICEY_OK) { g_err = h->err; spicey_destroy(h); return rc; }
  *out = h;
  return SPICEY_OK;
}

extern "C" int32_t spicey_get_info(SpiceyHandle *h, SpiceyInfo *info) {
  if (!h || !info) return SPICEY_ERR_BAD_DESC;
  fill_info(h->plan, h->hp, h->hres, h->opt, info);
  return SPICEY_OK;
}

// enqueue the kernel of a prepared launch behind its device's admission gate; ev0 / ev1 bracket the kernel alone
static int32_t enqueue_kernel(SpiceyHandle *h, const SpiceyRun &R, hipStream_t st) {
  // (the folded kernel reads its table behind the record of R.n_inst instances: only where the allocation holds both)
  const size_t fuse_doubles = h->plan.stamp_fuse ? spicey_stamp_fuse_words(h->plan.T) * sizeof(uint32_t) / sizeof(double) : 0;  // (that form's table, behind the fold's)
  const bool top_fold = h->plan.interp == 2 && spicey_top_fold_run(h->plan, R.steps) && R.n_inst == h->plan.n_inst &&
                        h->zpar_doubles == spicey_zpar_doubles(h->plan, h->hp) + SPICEY_TOP_FOLD_WORDS * sizeof(uint32_t) / sizeof(double) + fuse_doubles;
  const bool stamp_fuse = top_fold && spicey_stamp_fuse_run(h->plan, R.steps);
  if (h->plan.interp == 2 && spicey_top_fold_run(h->plan, R.steps) && !top_fold) { h->err = "internal: the plan folds the last factor level, but the table is not behind the parameter record"; return SPICEY_ERR_BAD_DESC; }
  DeviceGate &g = device_gate(h->device);
  std::lock_guard<std::mutex> lk(g.mu);  // (wait, launch and record are one step with respect to other launches)
  const bool group = h->plan.G > 1;
  int slot = -1;
  HIPCHK(h, gate_before_launch(g, group, st, &slot));
  HIPCHK(h, hipEventRecord(h->q.ev0, st));  // (argument upload, flag resets and admission waits stay outside the timed kernel)
  if (h->plan.interp == 3) {
    HIPCHK(h, spicey_launch_exact(h->d_xprog, h->d_Rstruct, h->plan.grid, h->plan.T, h->plan.lds ? h->plan.lds_bytes : 0, st));
  } else if (h->plan.interp == 2) {
    HIPCHK(h, spicey_launch_tran_v2(h->dprog, h->dres, h->d_Pstruct, h->d_Qstruct, h->d_Rstruct, h->plan.K, h->plan.grid, h->plan.T, st, h->plan.packed, !h->knobs.no_phase_table, h->d_zpar != nullptr, h->plan.slots, spicey_ready_run(h->plan, R.steps), spicey_addr_run(h->plan, R.steps), spicey_top_regs_run(h->plan, R.steps), spicey_u0_resident_run(h->plan, R.steps), top_fold, stamp_fuse, stamp_fuse && spicey_fixed_schedule_run(h->plan, R.steps), h->d_prof != nullptr));
  } else if (group) {
    HIPCHK(h, spicey_launch_tran_grp(h->dprog, R, h->plan.K, h->plan.grid, h->plan.T, st));
  } else {
    HIPCHK(h, spicey_launch_tran(h->dprog, R, h->plan.K, h->plan.lds, h->plan.grid, h->plan.T, st));
  }
  HIPCHK(h, hipEventRecord(h->q.ev1, st));
  HIPCHK(h, gate_after_launch(g, group, st, slot));
  return SPICEY_OK;
}

// The words every launch starts from zero: profile timers, diagnostics counters, front done-flags, group barrier words.
// (lin_err is an atomic max: zeroing it again before a repeated launch leaves the result as it was.)
static int32_t reset_launch_words(SpiceyHandle *h, hipStream_t st) {
  const LaunchPlan &pl = h->plan;
  const size_t nf = (size_t)h->hp.hdr.nFronts;
  if (h->d_prof) HIPCHK(h, hipMemsetAsync(h->d_prof, 0, ((size_t)pl.grid * pl.G * 72 + (size_t)pl.grid * 4 * nf) * sizeof(unsigned long long), st));
  if (h->d_skip) HIPCHK(h, hipMemsetAsync(h->d_skip, 0, (size_t)pl.n_inst * sizeof(unsigned long long), st));
  if (h->opt.diagnostics & 2) HIPCHK(h, hipMemsetAsync(h->d_linerr, 0, (size_t)pl.n_inst * (size_t)(h->last_steps + 1) * sizeof(unsigned long long), st));
  if (nf > 0) HIPCHK(h, hipMemsetAsync(h->d_front_flags, 0, (size_t)pl.grid * 2 * nf * sizeof(unsigned int), st));
  if (pl.G > 1) HIPCHK(h, hipMemsetAsync(h->d_gsync, 0, (size_t)pl.grid * SPICEY_GRP_SYNC_WORDS * sizeof(unsigned int), st));
  return SPICEY_OK;
}

// A new run begins: what spicey_last_inst_status reported about the previous one no longer holds (until this run's launch
// has finished, or it was refused as structurally singular, there is no per-instance answer).
void forget_last_run(SpiceyHandle *h) {
  h->last_status.clear();
  h->last_structural = false;
}

// The refusals of every transient entry point, in their order: the run arguments (out: the call's result buffer, src: its
// source table), then a matrix that is singular by its structure (every instance then fails: spicey_last_inst_status).
int32_t check_run_args(SpiceyHandle *h, int64_t steps, const void *out, const void *src, int32_t src_per_inst) {
  forget_last_run(h);
  if (steps < 0 || !out || (h->hp.hdr.nV > 0 && !src)) { h->err = "bad run arguments"; return SPICEY_ERR_BAD_DESC; }
  if (src_per_inst != 0 && src_per_inst != 1) { h->err = "src_per_inst must be 0 (one shared table) or 1 (one table per instance)"; return SPICEY_ERR_BAD_DESC; }
  return SPICEY_OK;
}
int32_t check_structure(SpiceyHandle *h) {
  if (!h->hp.structurally_singular) return SPICEY_OK;
  h->err = "singular at inst 0 step 0 iter 0 (structurally singular matrix)";
  h->last_structural = true;
  return SPICEY_ERR_SINGULAR;
}

// The body of spicey_run_device_src.  vals: null, or the device arrays {R, C, L} ([n_inst][n<kind>]: ohms, farads, henries)
// this run reads in the place of the handle's own (spicey_run_mc: the drawn values); the kernels derive everything they
// keep about the values in their own prologue, so nothing else changes.
int32_t run_device_src(SpiceyHandle *h, int64_t steps, double dt, const double *d_src_table, int32_t src_per_inst, double *d_out_v, double *d_out_i,
                              int32_t *d_iters, void *stream, const double *const *vals) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  if (const int32_t rc0 = check_run_args(h, steps, d_out_v, d_src_table, src_per_inst); rc0 != SPICEY_OK) return rc0;
  if (const int32_t rc0 = check_structure(h); rc0 != SPICEY_OK) return rc0;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  // a run still in flight on ANOTHER stream: this launch would reset status words, barrier words and front flags under
  // it — finish it first (its result is then reported here instead of by the next spicey_sync)
  if (h->pending && h->last_stream != st) {
    const int32_t rc0 = spicey_sync(h);
    forget_last_run(h);  // (that run's words are not this one's)
    if (rc0 != SPICEY_OK) return rc0;
  }
  const LaunchPlan &pl = h->plan;
  const SpiceyProg &P = h->hp.hdr;
  SpiceyRun R{};
  R.n_inst = pl.n_inst;
  R.want_currents = d_out_i != nullptr;
  R.debug_empty_phases = h->opt.debug >> 8;
  R.no_reuse = (h->opt.debug >> 1) & 1;
  R.steps = steps;
  R.dt = dt;
  R.R_val = vals ? vals[0] : h->d_R; R.C_val = vals ? vals[1] : h->d_C; R.L_val = vals ? vals[2] : h->d_L;
  R.S_ron = h->d_Sron; R.S_roff = h->d_Sroff; R.S_von = h->d_Svon; R.S_voff = h->d_Svoff;
  R.D_is = h->d_Dis; R.D_n = h->d_Dn;
  R.C_vprev = h->state.Cv; R.L_iprev = h->state.Li; R.D_vdprev = h->state.Dv; R.S_ison = h->state.Son;
  R.gstat = h->d_gstat; R.statv = h->d_statv; R.rcoef = h->d_rcoef; R.gW = pl.interp == 3 ? h->d_xws : h->d_gW; R.dpar = h->d_dpar;
  R.zpar = h->d_zpar;
  R.src = d_src_table; R.out_v = d_out_v; R.out_i = d_out_i; R.iters = d_iters;
  R.src_stride = src_per_inst ? (int64_t)(steps + 1) * P.nV : 0;
  R.status = h->d_status; R.solves = h->d_solves; R.prof = h->d_prof;
  // diagnostics: counters and per-step maxima start from zero in every run (reset_launch_words)
  h->last_steps = steps;
  R.skip_risk = h->d_skip;
  if (h->opt.diagnostics & 2) {
    const size_t need = (size_t)pl.n_inst * (size_t)(steps + 1);
    if (need > h->linerr_cap) {
      if (h->pending) { const int32_t rc0 = spicey_sync(h); forget_last_run(h); if (rc0 != SPICEY_OK) return rc0; }
      h->linerr_cap = 0;
      HIPCHK(h, h->d_linerr.alloc(need));
      h->linerr_cap = need;
    }
    R.lin_err = h->d_linerr;
    R.lin_vd = h->d_linvd;  // (null without diodes: the error stays 0)
  }
  if (const int32_t rc0 = reset_launch_words(h, st); rc0 != SPICEY_OK) return rc0;
  R.hyb_G = h->d_hybG; R.hyb_ug = h->d_hybUG;
  R.front_ticks = (h->d_prof && P.nFronts > 0) ? h->d_prof + (size_t)pl.grid * pl.G * 72 : nullptr;
  R.wgs_per_group = pl.G;
  R.grp_sync = h->d_gsync;
  R.grp_flags = h->d_gflags;
  if (P.nFronts > 0) {
    R.front_ws = h->d_front_ws;
    R.fs_first = h->d_fs;
    R.fs_list = h->d_fs + (pl.G + 1);
    R.fs_owner = R.fs_list + P.nFronts;
    R.front_flags = h->d_front_flags;
    R.front_lds_doubles = (h->opt.debug & 8) ? SPICEY_FRONT_LDS_DOUBLES_DEBUG : SPICEY_FRONT_LDS_DOUBLES;  // diagnostics: bit 3 = stage every front above 64 rows through panels
    R.front_right_looking = h->knobs.front_right_looking ? 1 : 0;
  }
  if (pl.G > 1) {
    // longest single cross-workgroup wait, in ticks of the chip-wide 100 MHz counter
    int ms = h->opt.group_timeout_ms;
    if (ms <= 0) ms = h->knobs.group_timeout_ms;
    if (ms <= 0) ms = 5000;
    R.grp_timeout_ticks = (unsigned long long)ms * 100000ull;
    // the state entering this launch, for the one relaunch after a bounded-wait abort (spicey_sync)
    if (h->opt.group_retry)
      HIPCHK(h, copy_state(h->state_s.ptrs(), h->state.ptrs(), P, (size_t)pl.n_inst, hipMemcpyDeviceToDevice, true, st));
    R.force_abort = h->knobs.force_group_abort ? 1 : 0;
    h->grp_R = R;
  }
  if (pl.interp == 2 || pl.interp == 3) {  // (these kernels read their SpiceyRun from device memory)
    h->run_args = R;
    HIPCHK(h, hipMemcpyAsync(h->d_Rstruct, &h->run_args, sizeof(SpiceyRun), hipMemcpyHostToDevice, st));
  }
  const int32_t rc = enqueue_kernel(h, R, st);
  if (rc != SPICEY_OK) return rc;
  h->pending = true;
  h->last_stream = st;
  return SPICEY_OK;
}

extern "C" int32_t spicey_run_device_src(SpiceyHandle *h, int64_t steps, double dt, const double *d_src_table, int32_t src_per_inst,
                                         double *d_out_v, double *d_out_i, int32_t *d_iters, void *stream) {
  return run_device_src(h, steps, dt, d_src_table, src_per_inst, d_out_v, d_out_i, d_iters, stream, nullptr);
}

extern "C" int32_t spicey_run_device(SpiceyHandle *h, int64_t steps, double dt, const double *d_src_table, double *d_out_v,
                                     double *d_out_i, int32_t *d_iters, void *stream) {
  return spicey_run_device_src(h, steps, dt, d_src_table, 0, d_out_v, d_out_i, d_iters, stream);
}

extern "C" int32_t spicey_sync(SpiceyHandle *h) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  if (!h->pending) return SPICEY_OK;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<int32_t> status((size_t)h->plan.grid * 4);
  std::vector<unsigned long long> solves((size_t)h->plan.grid);
  int best = -1;
  std::string aborted;  // text of an aborted attempt that was repeated
  for (int attempt = 0;; attempt++) {
    HIPCHK(h, hipStreamSynchronize(h->last_stream));
    h->pending = false;
    StreamTimers::elapsed(h->q.ev0, h->q.ev1, &h->last_ms);
    HIPCHK(h, hipMemcpy(status.data(), h->d_status, status.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(solves.data(), h->d_solves, solves.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    h->last_status = status;
    h->last_solves = 0;
    for (auto s : solves) h->last_solves += (int64_t)s;
    std::vector<unsigned int> gsync;
    if (h->plan.G > 1 && h->d_gsync) {
      gsync.resize((size_t)h->plan.grid * SPICEY_GRP_SYNC_WORDS);
      HIPCHK(h, hipMemcpy(gsync.data(), h->d_gsync, gsync.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
      for (int g = 0; g < h->plan.grid; g++) h->stale_polls += (int64_t)gsync[(size_t)g * SPICEY_GRP_SYNC_WORDS + 8];
    }
    // earliest failure wins (the reference throws at the first singular solve)
    best = -1;
    for (int g = 0; g < h->plan.grid; g++)
      if (status[(size_t)g * 4] != 0 && (best < 0 || status[(size_t)g * 4 + 2] < status[(size_t)best * 4 + 2])) best = g;
    if (best < 0 || status[(size_t)best * 4] != 3) break;
    // (the first workgroup that gave up left a note in its group's barrier words, GpuGroupExec::note_timeout)
    const unsigned int none[9] = {0};
    const unsigned int *note = gsync.empty() ? none : gsync.data() + (size_t)best * SPICEY_GRP_SYNC_WORDS;
    const char *kind = note[2] == 2 ? "front hand-over" : note[2] == 3 ? "census barrier" : note[2] == 1 ? "group barrier" : note[2] == 4 ? "XCD census does not add up" : "abort word raised";
    char buf[384];
    snprintf(buf, sizeof(buf), "cross-workgroup wait timed out (group mode) at step %d: %s, group %d of %d, workgroup %u of %d (XCD %u), %s %u, waited for %u, saw %u; %d threads, %d fronts, timeout %.0f ms",
             status[(size_t)best * 4 + 2], kind, best, h->plan.grid, note[3], h->plan.G, note[7], note[2] == 2 ? "front flag" : "barrier", note[4], note[5], note[6], h->plan.T,
             h->hp.hdr.nFronts, (double)h->grp_R.grp_timeout_ticks / 1e5);
    h->err = buf;
    fprintf(stderr, "spicey: %s%s\n", buf, (attempt == 0 && h->opt.group_retry) ? " -- repeating the launch once (SpiceyOptions.group_retry)" : "");
    if (attempt > 0 || h->plan.G <= 1 || !h->opt.group_retry) return SPICEY_ERR_HIP;
    // The bounded wait turned what would have been a hang into an abort; nothing of the aborted launch is kept.  On request
    // the launch is repeated ONCE from the state it started with (the kernel writes state only in its last step, but that
    // step may be the one that aborted): same arguments, same stream, fresh barrier words and front flags.
    h->group_retries++;
    aborted = buf;
    hipStream_t st = h->last_stream;
    HIPCHK(h, copy_state(h->state.ptrs(), h->state_s.ptrs(), h->hp.hdr, (size_t)h->plan.n_inst, hipMemcpyDeviceToDevice, true, st));
    if (const int32_t rc0 = reset_launch_words(h, st); rc0 != SPICEY_OK) return rc0;
    h->grp_R.force_abort = 0;
    const int32_t rc = enqueue_kernel(h, h->grp_R, st);
    if (rc != SPICEY_OK) return rc;
    h->pending = true;
  }
  // (the text of an aborted attempt stays readable although its repetition went through)
  if (!aborted.empty() && best < 0) h->err = "recovered: " + aborted;
  if (best >= 0 && status[(size_t)best * 4] == 2) {  // (an operand-address kernel refused to run: kernels.hip, SPICEY_KERNEL_OA)
    h->err = "internal: the operand-address kernel found its workspace away from LDS offset 0 (SPICEY_NO_OPERAND_ADDR selects the kernel without that condition)";
    return SPICEY_ERR_HIP;
  }
  if (best >= 0) {
    char buf[160];
    snprintf(buf, sizeof(buf), "singular at inst %d step %d iter %d", status[(size_t)best * 4 + 1], status[(size_t)best * 4 + 2],
             status[(size_t)best * 4 + 3]);
    h->err = buf;
    return SPICEY_ERR_SINGULAR;
  }
  return SPICEY_OK;
}

extern "C" int32_t spicey_group_retries(const SpiceyHandle *h) { return h ? h->group_retries : 0; }
extern "C" int32_t spicey_top_regs_form(const SpiceyHandle *h, int64_t steps) { return (h && h->plan.interp == 2 && spicey_top_regs_run(h->plan, steps)) ? 1 : 0; }
extern "C" int32_t spicey_u0_resident_form(const SpiceyHandle *h, int64_t steps) { return (h && h->plan.interp == 2 && spicey_u0_resident_run(h->plan, steps)) ? 1 : 0; }
extern "C" int32_t spicey_top_fold_form(const SpiceyHandle *h, int64_t steps) { return (h && h->plan.interp == 2 && spicey_top_fold_run(h->plan, steps)) ? 1 : 0; }
extern "C" int32_t spicey_fixed_schedule_form(const SpiceyHandle *h, int64_t steps) { return (h && h->plan.interp == 2 && spicey_fixed_schedule_run(h->plan, steps)) ? 1 : 0; }
extern "C" int32_t spicey_stamp_fuse_form(const SpiceyHandle *h, int64_t steps) { return (h && h->plan.interp == 2 && spicey_stamp_fuse_run(h->plan, steps)) ? 1 : 0; }
extern "C" int64_t spicey_group_stale_polls(const SpiceyHandle *h) { return h ? h->stale_polls : 0; }

// Per instance of the last run, from the status words {code, inst, step, iter} of its workgroups: workgroup (or group) g
// ran instances g K .. g K + K - 1 (kernels.hip, exact.hip), and its code names only the instance that failed first — the
// others of that workgroup stopped with it, unfinished.
extern "C" int32_t spicey_last_inst_status(SpiceyHandle *h, int32_t *status) {
  if (!h || !status) return -1;
  if (h->pending) spicey_sync(h);
  if (h->last_status.empty() && !h->last_structural) return -1;  // no run yet, a run refused before its launch, or a lost one
  const int ni = h->plan.n_inst, K = h->plan.K;
  int32_t bad = 0;
  for (int i = 0; i < ni; i++) status[i] = h->last_structural ? SPICEY_ERR_SINGULAR : 0;
  if (h->last_structural) return ni;
  const int grid = std::min<int>(h->plan.grid, (int)(h->last_status.size() / 4));
  for (int g = 0; g < grid; g++) {
    const int32_t code = h->last_status[(size_t)g * 4], who = h->last_status[(size_t)g * 4 + 1];
    if (code == 0) continue;
    for (int k = 0; k < K && g * K + k < ni; k++) {
      const int in = g * K + k;
      status[in] = code != 1 ? SPICEY_ERR_HIP : in == who ? SPICEY_ERR_SINGULAR : -1;
    }
  }
  for (int i = 0; i < ni; i++) bad += status[i] != 0;
  return bad;
}


// keep_partial: the results also come back after SPICEY_ERR_SINGULAR (spicey_run_src: the instances that finished are complete)
static int32_t run_host(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, double *out_v,
                        double *out_i, int32_t *iters, bool keep_partial) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  if (const int32_t rc0 = check_run_args(h, steps, out_v, src_table, src_per_inst); rc0 != SPICEY_OK) return rc0;
  if (const int32_t rc0 = check_structure(h); rc0 != SPICEY_OK) return rc0;
  HIPCHK(h, hipSetDevice(h->device));
  Roctx range_run("spicey_run");
  HostRun r;
  if (const int32_t rc0 = r.stage(h, steps, src_table, src_per_inst, out_i != nullptr, iters != nullptr); rc0 != SPICEY_OK) return rc0;
  int32_t rc;
  {
    Roctx range_kernel("spicey_run:kernel");
    rc = spicey_run_device_src(h, steps, dt, r.d_src, src_per_inst, r.d_v, r.d_i, r.d_it, h->q.stream);
    if (rc == SPICEY_OK) rc = spicey_sync(h);
  }
  if (rc == SPICEY_OK || (keep_partial && rc == SPICEY_ERR_SINGULAR)) {
    Roctx range_copy("spicey_run:results");
    if (const int32_t rc0 = r.copy_out(h, out_v, out_i, iters); rc0 != SPICEY_OK) return rc0;
  }
  return rc;
}

extern "C" int32_t spicey_run_src(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, double *out_v,
                                  double *out_i, int32_t *iters) {
  return run_host(h, steps, dt, src_table, src_per_inst, out_v, out_i, iters, true);
}

extern "C" int32_t spicey_run(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, double *out_v, double *out_i,
                              int32_t *iters) {
  return run_host(h, steps, dt, src_table, 0, out_v, out_i, iters, false);
}

extern "C" int32_t spicey_get_state(SpiceyHandle *h, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  int32_t rc = spicey_sync(h);
  if (rc != SPICEY_OK && rc != SPICEY_ERR_SINGULAR) return rc;
  HIPCHK(h, copy_state({C_vprev, L_iprev, D_vdprev, S_ison}, h->state.ptrs(), h->hp.hdr, (size_t)h->plan.n_inst, hipMemcpyDeviceToHost, false));
  return SPICEY_OK;
}

extern "C" int32_t spicey_set_state(SpiceyHandle *h, const double *C_vprev, const double *L_iprev, const double *D_vdprev,
                                    const int32_t *S_ison) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  int32_t rc = spicey_sync(h);
  if (rc != SPICEY_OK && rc != SPICEY_ERR_SINGULAR) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  // (a copy source only: StatePtrs names the state's kinds, not whether they may be written)
  const StatePtrs src{const_cast<double *>(C_vprev), const_cast<double *>(L_iprev), const_cast<double *>(D_vdprev), const_cast<int32_t *>(S_ison)};
  HIPCHK(h, copy_state(h->state.ptrs(), src, h->hp.hdr, (size_t)h->plan.n_inst, hipMemcpyHostToDevice, false));
  return SPICEY_OK;
}

extern "C" int32_t spicey_reset_state(SpiceyHandle *h, void *stream) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, copy_state(h->state.ptrs(), h->state0.ptrs(), h->hp.hdr, (size_t)h->plan.n_inst, hipMemcpyDeviceToDevice, true, (hipStream_t)stream));
  return SPICEY_OK;
}

extern "C" int64_t spicey_last_solve_count(SpiceyHandle *h) { return h ? h->last_solves : 0; }

extern "C" int64_t spicey_last_skip_risk(SpiceyHandle *h, int64_t *per_inst) {
  if (!h || !h->d_skip) return -1;
  if (spicey_sync(h) == SPICEY_ERR_HIP) return -1;
  std::vector<unsigned long long> tmp((size_t)h->plan.n_inst);
  if (hipSetDevice(h->device) != hipSuccess || hipMemcpy(tmp.data(), h->d_skip, tmp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  int64_t tot = 0;
  for (size_t i = 0; i < tmp.size(); i++) { tot += (int64_t)tmp[i]; if (per_inst) per_inst[i] = (int64_t)tmp[i]; }
  return tot;
}

extern "C" int32_t spicey_get_lin_err(SpiceyHandle *h, double *out) {
  if (!h || !out) return SPICEY_ERR_BAD_DESC;
  if (!(h->opt.diagnostics & 2) || !h->d_linerr || h->last_steps < 0) { h->err = "spicey_get_lin_err needs SpiceyOptions.diagnostics bit 1 and a finished run"; return SPICEY_ERR_BAD_DESC; }
  const int32_t rc = spicey_sync(h);
  if (rc != SPICEY_OK && rc != SPICEY_ERR_SINGULAR) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  // (bit patterns of non-negative doubles: a plain copy)
  HIPCHK(h, hipMemcpy(out, h->d_linerr, (size_t)h->plan.n_inst * (size_t)(h->last_steps + 1) * sizeof(double), hipMemcpyDeviceToHost));
  return SPICEY_OK;
}
extern "C" double spicey_last_kernel_ms(SpiceyHandle *h) { return h ? h->last_ms : 0.0; }

extern "C" int32_t spicey_debug_phase_cycles(SpiceyHandle *h, uint64_t *out, int32_t n) {
  if (!h || !out) return 0;
  for (int i = 0; i < n; i++) out[i] = 0;
  if (!h->d_prof) return 0;
  if (spicey_sync(h) == SPICEY_ERR_HIP) return 0;
  unsigned long long tmp[72];
  if (hipMemcpy(tmp, h->d_prof, sizeof(tmp), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  for (int i = 0; i < n && i < 72; i++) out[i] = tmp[i];
  return 72;
}

// Same for launched workgroup `wg` (group mode: wg = group * wgs_per_inst + index; the slots then hold 100 MHz wall ticks
// per SECTION: [1] B, [8] factor levels below the cut, [9] fronts forward, [10] fronts backward, [11] sync + publish,
// [12..20] inside the fronts (wait, assemble, panel load, diagonal block, triangular solves, trailing update, ...), [40] backward
// levels, [4] Z).
extern "C" int32_t spicey_debug_phase_cycles_wg(SpiceyHandle *h, int32_t wg, uint64_t *out, int32_t n) {
  if (!h || !out) return 0;
  for (int i = 0; i < n; i++) out[i] = 0;
  if (!h->d_prof || wg < 0 || wg >= h->plan.grid * h->plan.G) return 0;
  if (spicey_sync(h) == SPICEY_ERR_HIP) return 0;
  unsigned long long tmp[72];
  if (hipMemcpy(tmp, h->d_prof + (size_t)wg * 72, sizeof(tmp), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  for (int i = 0; i < n && i < 72; i++) out[i] = tmp[i];
  return 72;
}

// Per-front event times of group `grp` in the last run (profile option; program.h, SpiceyRun::front_ticks): out[f * 4 + e]
// = 100 MHz ticks since the owner entered the forward sweep, SUMMED over the solves; also the fronts' shape and owner
// (meta[f * 4 + {0: pivots, 1: boundary, 2: parent, 3: owning workgroup}]).  Returns the number of fronts.
extern "C" int32_t spicey_debug_front_ticks(SpiceyHandle *h, int32_t grp, uint64_t *out, int32_t *meta, int32_t cap_fronts) {
  if (!h || !out || !meta || !h->d_prof || grp < 0 || grp >= h->plan.grid) return 0;
  const int nf = h->hp.hdr.nFronts;
  if (nf <= 0 || cap_fronts < nf) return 0;
  if (spicey_sync(h) == SPICEY_ERR_HIP) return 0;
  std::vector<unsigned long long> tmp((size_t)nf * 4);
  if (hipMemcpy(tmp.data(), h->d_prof + (size_t)h->plan.grid * h->plan.G * 72 + (size_t)grp * 4 * nf, tmp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  for (size_t i = 0; i < tmp.size(); i++) out[i] = tmp[i];
  std::vector<uint32_t> first, list;
  spicey_build_front_schedule(h->hp, h->plan.G, first, list);
  for (int w = 0; w < h->plan.G; w++)
    for (uint32_t s2 = first[w]; s2 < first[w + 1]; s2++) meta[(size_t)list[s2] * 4 + 3] = w;
  for (int f = 0; f < nf; f++) {
    meta[(size_t)f * 4 + 0] = h->hp.fronts[f].p; meta[(size_t)f * 4 + 1] = h->hp.fronts[f].q; meta[(size_t)f * 4 + 2] = h->hp.fronts[f].parent;
  }
  return nf;
}

// ---------------------------------------------------------------------------------------------------------------------
// Several devices behind one handle: instance shards, one SpiceyHandle per shard, host threads around the blocking runs.
struct SpiceyMulti {
  struct Shard { SpiceyHandle *h = nullptr; int device = 0, first = 0, count = 0; };
  std::vector<Shard> shards;
  int n_inst = 0;
  int nC = 0, nL = 0, nD = 0, nS = 0, nV = 0, nOut = 0, nCur = 0;
  int64_t last_solves = 0;
  double last_ms = 0.0;
  std::string err;
};

extern "C" const char *spicey_multi_last_error(SpiceyMulti *m) { return m ? m->err.c_str() : g_err.c_str(); }

extern "C" void spicey_destroy_multi(SpiceyMulti *m) {
  if (!m) return;
  for (auto &s : m->shards) spicey_destroy(s.h);
  delete m;
}

extern "C" int32_t spicey_create_multi(const SpiceyDesc *desc, const SpiceyOptions *opt, const int32_t *devices, int32_t n_dev, SpiceyMulti **out) {
  if (!out) { g_err = "null out pointer"; return SPICEY_ERR_BAD_DESC; }
  *out = nullptr;
  if (!desc || !devices || n_dev < 1) { g_err = "spicey_create_multi needs a descriptor and a list of >= 1 devices"; return SPICEY_ERR_BAD_DESC; }
  if (desc->n_inst < 1) { g_err = "negative count or n_inst < 1"; return SPICEY_ERR_BAD_DESC; }
  for (int d = 0; d < n_dev; d++)
    if (devices[d] < 0) { g_err = "device ordinal out of range"; return SPICEY_ERR_BAD_DESC; }
  SpiceyMulti *m = new SpiceyMulti();
  m->n_inst = desc->n_inst;
  const int ni = desc->n_inst;
  for (int d = 0; d < n_dev; d++) {
    // block partition: shard d = instances [ceil(d ni / n_dev), ceil((d + 1) ni / n_dev))
    const int lo = (int)(((int64_t)d * ni + n_dev - 1) / n_dev), hi = (int)(((int64_t)(d + 1) * ni + n_dev - 1) / n_dev);
    if (hi <= lo) continue;
    SpiceyDesc sd = *desc;
    sd.n_inst = hi - lo;
    auto adv = [&](const double *p, int n) { return p ? p + (size_t)lo * (size_t)n : p; };
    sd.R_val = adv(desc->R_val, desc->nR);
    sd.C_val = adv(desc->C_val, desc->nC); sd.C_vprev = adv(desc->C_vprev, desc->nC);
    sd.L_val = adv(desc->L_val, desc->nL); sd.L_iprev = adv(desc->L_iprev, desc->nL);
    sd.S_ron = adv(desc->S_ron, desc->nS); sd.S_roff = adv(desc->S_roff, desc->nS);
    sd.S_von = adv(desc->S_von, desc->nS); sd.S_voff = adv(desc->S_voff, desc->nS);
    sd.S_ison = desc->S_ison ? desc->S_ison + (size_t)lo * (size_t)desc->nS : nullptr;
    sd.D_is = adv(desc->D_is, desc->nD); sd.D_n = adv(desc->D_n, desc->nD); sd.D_vdprev = adv(desc->D_vdprev, desc->nD);
    SpiceyOptions so{};
    if (opt) so = *opt;
    so.device = devices[d];
    SpiceyMulti::Shard s;
    s.device = devices[d]; s.first = lo; s.count = hi - lo;
    const int32_t rc = spicey_create(&sd, &so, &s.h);
    if (rc != SPICEY_OK) {
      char buf[64];
      snprintf(buf, sizeof(buf), " (shard %d on device %d)", d, devices[d]);
      g_err += buf;
      spicey_destroy_multi(m);
      return rc;
    }
    m->shards.push_back(s);
  }
  const SpiceyProg &P = m->shards[0].h->hp.hdr;
  m->nC = P.nC; m->nL = P.nL; m->nD = P.nD; m->nS = P.nS; m->nV = P.nV; m->nOut = P.nOut; m->nCur = P.nCur;
  *out = m;
  return SPICEY_OK;
}

extern "C" int32_t spicey_run_multi_src(SpiceyMulti *m, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, double *out_v,
                                        double *out_i, int32_t *iters) {
  if (!m) return SPICEY_ERR_BAD_DESC;
  if (steps < 0 || !out_v) { m->err = "bad run arguments"; return SPICEY_ERR_BAD_DESC; }
  if (src_per_inst != 0 && src_per_inst != 1) { m->err = "src_per_inst must be 0 (one shared table) or 1 (one table per instance)"; return SPICEY_ERR_BAD_DESC; }
  const size_t np = (size_t)steps + 1;
  std::vector<int32_t> rcs(m->shards.size(), SPICEY_OK);
  std::vector<std::thread> th;
  for (size_t i = 0; i < m->shards.size(); i++) {
    th.emplace_back([&, i]() {
      const SpiceyMulti::Shard &s = m->shards[i];
      // (per-instance tables: the shard's slice, instances first .. first + count - 1)
      const double *tab = src_table && src_per_inst ? src_table + (size_t)s.first * np * (size_t)m->nV : src_table;
      // (the shared layout keeps spicey_run's behaviour: no results come back after an error)
      rcs[i] = run_host(s.h, steps, dt, tab, src_per_inst, out_v + (size_t)s.first * np * (size_t)m->nOut,
                        out_i ? out_i + (size_t)s.first * np * (size_t)m->nCur : nullptr, iters ? iters + (size_t)s.first * np : nullptr, src_per_inst != 0);
    });
  }
  for (auto &t : th) t.join();
  m->last_solves = 0;
  m->last_ms = 0.0;
  int32_t rc = SPICEY_OK;
  for (size_t i = 0; i < m->shards.size(); i++) {
    const SpiceyMulti::Shard &s = m->shards[i];
    if (rcs[i] != SPICEY_OK && rc == SPICEY_OK) {  // first failing shard in instance order; its instance number made global
      rc = rcs[i];
      char buf[96];
      snprintf(buf, sizeof(buf), " (shard %d: instances %d..%d on device %d)", (int)i, s.first, s.first + s.count - 1, s.device);
      m->err = std::string(spicey_last_error(s.h)) + buf;
    }
    m->last_solves += spicey_last_solve_count(s.h);
    m->last_ms = std::max(m->last_ms, spicey_last_kernel_ms(s.h));
  }
  return rc;
}

extern "C" int32_t spicey_run_multi(SpiceyMulti *m, int64_t steps, double dt, const double *src_table, double *out_v, double *out_i, int32_t *iters) {
  return spicey_run_multi_src(m, steps, dt, src_table, 0, out_v, out_i, iters);
}

extern "C" int32_t spicey_get_state_multi(SpiceyMulti *m, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison) {
  if (!m) return SPICEY_ERR_BAD_DESC;
  for (auto &s : m->shards) {
    const int32_t rc = spicey_get_state(s.h, C_vprev ? C_vprev + (size_t)s.first * m->nC : nullptr, L_iprev ? L_iprev + (size_t)s.first * m->nL : nullptr,
                                        D_vdprev ? D_vdprev + (size_t)s.first * m->nD : nullptr, S_ison ? S_ison + (size_t)s.first * m->nS : nullptr);
    if (rc != SPICEY_OK) { m->err = spicey_last_error(s.h); return rc; }
  }
  return SPICEY_OK;
}

extern "C" int32_t spicey_multi_get_shard(SpiceyMulti *m, int32_t shard, SpiceyInfo *info, int32_t *device, int32_t *first_inst, int32_t *n_inst) {
  if (!m || shard < 0 || shard >= (int32_t)m->shards.size()) return SPICEY_ERR_BAD_DESC;
  const SpiceyMulti::Shard &s = m->shards[shard];
  if (info) spicey_get_info(s.h, info);
  if (device) *device = s.device;
  if (first_inst) *first_inst = s.first;
  if (n_inst) *n_inst = s.count;
  return SPICEY_OK;
}

extern "C" int32_t spicey_multi_group_retries(SpiceyMulti *m) {
  int32_t n = 0;
  if (m) for (auto &s : m->shards) n += spicey_group_retries(s.h);
  return n;
}
extern "C" int64_t spicey_multi_group_stale_polls(SpiceyMulti *m) {
  int64_t n = 0;
  if (m) for (auto &s : m->shards) n += spicey_group_stale_polls(s.h);
  return n;
}
extern "C" int64_t spicey_multi_last_solve_count(SpiceyMulti *m) { return m ? m->last_solves : 0; }
extern "C" double spicey_multi_last_kernel_ms(SpiceyMulti *m) { return m ? m->last_ms : 0.0; }
