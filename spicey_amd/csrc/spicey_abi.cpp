// spicey_abi.cpp — the C-ABI of include/spicey_hip.h: handle management, uploads, launches.
// Host code only (HIP runtime API); the kernels are in kernels.hip, the symbolic phase in
// symbolic.cpp.  There is NO CPU solve path in this library: without a HIP device every entry
// point that would compute returns SPICEY_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/spicey_hip.h"
#include "devbuf.h"
#include "exact_plan.h"
#include "kernels.h"
#include "launch_plan.h"
#include "ac_measure.h"
#include "ac_measure_exec.h"
#include "fourier.h"
#include "fourier_exec.h"
#include "measure.h"
#include "measure_exec.h"
#include "noise.h"
#include "mc.h"
#include "sens.h"
#include "power.h"
#include "values.h"
#include "spectrum.h"
#include "timing.h"
#include "timing_exec.h"
#include "tran_mc.h"
#include "tran_sens.h"
#include "symbolic.h"
#include "fronts_exec_consts.h"

// The instance state a transient step carries: C_vprev, L_iprev, D_vdprev, S_ison ([n_inst][nC | nL | nD | nS] each).
struct StatePtrs { double *Cv, *Li, *Dv; int32_t *Son; };
struct StateBufs {
  DevBuf<double> Cv, Li, Dv;
  DevBuf<int32_t> Son;
  StatePtrs ptrs() const { return {Cv, Li, Dv, Son}; }
};
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

struct SpiceyHandle {
  HostProgram hp;
  HostResident hres;
  LaunchPlan plan;       // K, T, grid, G, interpreter, geometry, workspace (launch_plan.h)
  SpiceyOptions opt{};
  SpiceyKnobs knobs;     // environment, read once by spicey_create
  SpiceyProg dprog{}; SpiceyResident dres{};
  int device = 0;
  DevBuf<uint8_t> d_blob, d_res;
  // v2 kernels take their argument structs from device memory (scalar loads per phase instead of ~110 pointers in SGPRs)
  DevBuf<SpiceyProg> d_Pstruct; DevBuf<SpiceyResident> d_Qstruct; DevBuf<SpiceyRun> d_Rstruct;
  SpiceyRun run_args{};  // host copy of the last launch's SpiceyRun (source of the asynchronous upload)
  DevBuf<double> d_R, d_C, d_L, d_Sron, d_Sroff, d_Svon, d_Svoff, d_Dis, d_Dn;
  // live, the descriptor's (spicey_reset_state), and in group mode the state as it entered the launch in flight (a launch
  // that ends in the bounded-spin abort is repeated once)
  StateBufs state, state0, state_s;
  // reference-order engine (interpreter 3): stamp lists and terminals, their device copy and descriptor, global workspace
  HostExactProg xp;
  DevBuf<uint32_t> d_xblob; DevBuf<SpiceyExactProg> d_xprog; DevBuf<double> d_xws;
  DevBuf<unsigned int> d_gsync; DevBuf<int32_t> d_gflags;
  // dense fronts: workspace [grid][front_ws], schedule of the G workgroups, done flags [grid][2 nFronts]
  DevBuf<double> d_front_ws;
  DevBuf<uint32_t> d_fs;  // first[G + 1] | list[nFronts] | owner[nFronts]
  DevBuf<unsigned int> d_front_flags;
  SpiceyRun grp_R{};      // group mode: the launch's arguments
  int group_retries = 0;  // launches repeated so far (spicey_group_retries)
  // diagnostics (SpiceyOptions.diagnostics): skip-risk counters [n_inst], linearisation points [n_inst][nD], per-step
  // linearisation error [n_inst][steps + 1] of the last run (grown on demand)
  DevBuf<double> d_hybG, d_hybUG;  // hybrid workspace: leaf-owned entries [n_inst][nLU], u | gd [n_inst][nU + nGdyn]
  DevBuf<unsigned long long> d_skip, d_linerr; DevBuf<double> d_linvd;
  size_t linerr_cap = 0;
  int64_t last_steps = -1;
  int64_t stale_polls = 0;  // group mode: waits that only the read-modify-write poll saw satisfied (spicey_group_stale_polls)
  bool gated = false;     // this handle is counted in its device's group-mode handles (DeviceGate)
  DevBuf<double> d_gstat, d_statv, d_rcoef, d_gW, d_dpar;
  size_t zpar_doubles = 0;  // doubles allocated in d_zpar: the record, and behind it the table of the folded last factor level where the plan says top_fold
  DevBuf<double> d_zpar;  // early-prefetch builds: Z's parameter record (SpiceyRun::zpar), written by every launch's prologue; else null
  DevBuf<int32_t> d_status; DevBuf<unsigned long long> d_solves, d_prof;
  hipStream_t last_stream = nullptr;
  double last_pass_ms[N_PASS] = {};  // the reduction passes of the last spicey_run_measure* (0: the pass did not run)
  double last_tran_mc_ms = 0.0, last_tran_mc_draw_ms = 0.0;  // the last spicey_run_mc: its scalars and reduction, its draw
  double last_tran_sens_ms = 0.0, last_tran_sens_design_ms = 0.0;  // the last spicey_run_sens / spicey_run_levels: the same, its design
  bool pending = false;
  int64_t last_solves = 0;
  double last_ms = 0.0;
  // status words [grid][4] of the last finished launch (spicey_sync), and whether the last run was refused as structurally
  // singular before any launch (every instance then fails): the per-instance answer of spicey_last_inst_status
  std::vector<int32_t> last_status;
  bool last_structural = false;
  std::string err;
  StreamTimers q;  // the owned stream of spicey_run and its events (last: they go before the device buffers)
};

static thread_local std::string g_err;  // message of the calling thread's last failed spicey_create (no handle to hang it on)

// roctx ranges around the host-side phases (SURVEY §5 tracing hook): `rocprofv3 --marker-trace` shows symbolic phase, uploads,
// kernel and result copies as named ranges.  The marker library is looked up at run time (no link dependency: without it,
// or outside a profiler, the ranges cost one null check).
namespace {
struct Roctx {
  typedef int (*push_t)(const char *);
  typedef int (*pop_t)();
  static push_t push_fn() {
    static push_t f = []() -> push_t {
      for (const char *lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"})
        if (void *hnd = dlopen(lib, RTLD_LAZY | RTLD_GLOBAL))
          if (void *sym = dlsym(hnd, "roctxRangePushA")) { pop_fn_ref() = (pop_t)dlsym(hnd, "roctxRangePop"); return (push_t)sym; }
      return nullptr;
    }();
    return f;
  }
  static pop_t &pop_fn_ref() { static pop_t p = nullptr; return p; }
  bool on;
  explicit Roctx(const char *name) : on(false) {
    if (push_t f = push_fn()) { f(name); on = pop_fn_ref() != nullptr; }
  }
  ~Roctx() { if (on) pop_fn_ref()(); }
};
}  // namespace

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
    HIPCHK(h, spicey_launch_tran_v2(h->dprog, h->dres, h->d_Pstruct, h->d_Qstruct, h->d_Rstruct, h->plan.K, h->plan.grid, h->plan.T, st, h->plan.packed, !h->knobs.no_phase_table, h->d_zpar != nullptr, h->plan.slots, spicey_ready_run(h->plan, R.steps), spicey_addr_run(h->plan, R.steps), spicey_top_regs_run(h->plan, R.steps), spicey_u0_resident_run(h->plan, R.steps), top_fold, stamp_fuse));
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
static void forget_last_run(SpiceyHandle *h) {
  h->last_status.clear();
  h->last_structural = false;
}

// The refusals of every transient entry point, in their order: the run arguments (out: the call's result buffer, src: its
// source table), then a matrix that is singular by its structure (every instance then fails: spicey_last_inst_status).
static int32_t check_run_args(SpiceyHandle *h, int64_t steps, const void *out, const void *src, int32_t src_per_inst) {
  forget_last_run(h);
  if (steps < 0 || !out || (h->hp.hdr.nV > 0 && !src)) { h->err = "bad run arguments"; return SPICEY_ERR_BAD_DESC; }
  if (src_per_inst != 0 && src_per_inst != 1) { h->err = "src_per_inst must be 0 (one shared table) or 1 (one table per instance)"; return SPICEY_ERR_BAD_DESC; }
  return SPICEY_OK;
}
static int32_t check_structure(SpiceyHandle *h) {
  if (!h->hp.structurally_singular) return SPICEY_OK;
  h->err = "singular at inst 0 step 0 iter 0 (structurally singular matrix)";
  h->last_structural = true;
  return SPICEY_ERR_SINGULAR;
}

// The body of spicey_run_device_src.  vals: null, or the device arrays {R, C, L} ([n_inst][n<kind>]: ohms, farads, henries)
// this run reads in the place of the handle's own (spicey_run_mc: the drawn values); the kernels derive everything they
// keep about the values in their own prologue, so nothing else changes.
static int32_t run_device_src(SpiceyHandle *h, int64_t steps, double dt, const double *d_src_table, int32_t src_per_inst, double *d_out_v, double *d_out_i,
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

// The device side of a run on host buffers (run_host, spicey_run_measure): the source table up on the handle's stream,
// the buffers the run records into, and the way back.
struct HostRun {
  size_t np = 0, ni = 0;
  DevBuf<double> d_src, d_v, d_i;
  DevBuf<int32_t> d_it;
  int32_t stage(SpiceyHandle *h, int64_t steps, const double *src_table, int32_t src_per_inst, bool want_i, bool want_iters) {
    const SpiceyProg &P = h->hp.hdr;
    np = (size_t)steps + 1, ni = (size_t)h->plan.n_inst;
    const size_t ntab = src_per_inst ? ni : 1;
    HIPCHK(h, d_src.alloc(std::max<size_t>(ntab * np * P.nV, 1)));
    if (P.nV) HIPCHK(h, hipMemcpyAsync(d_src, src_table, ntab * np * P.nV * sizeof(double), hipMemcpyHostToDevice, h->q.stream));
    HIPCHK(h, d_v.alloc(std::max<size_t>(ni * np * P.nOut, 1)));
    if (want_i) HIPCHK(h, d_i.alloc(std::max<size_t>(ni * np * P.nCur, 1)));
    if (want_iters) HIPCHK(h, d_it.alloc(ni * np));
    return SPICEY_OK;
  }
  // (blocking copies behind a finished run; null: not wanted)
  int32_t copy_out(SpiceyHandle *h, double *out_v, double *out_i, int32_t *iters) const {
    const SpiceyProg &P = h->hp.hdr;
    if (out_v) HIPCHK(h, hipMemcpy(out_v, d_v, ni * np * P.nOut * sizeof(double), hipMemcpyDeviceToHost));
    if (out_i) HIPCHK(h, hipMemcpy(out_i, d_i, ni * np * P.nCur * sizeof(double), hipMemcpyDeviceToHost));
    if (iters) HIPCHK(h, hipMemcpy(iters, d_it, ni * np * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SPICEY_OK;
  }
};

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
// Waveform measurements (include/spicey_hip.h): the reduction pass of measure.hip behind a transient run.

extern "C" int64_t spicey_measure_workspace_bytes(int32_t n_inst, int64_t n_points, int32_t n_req) {
  return spicey_meas_workspace_bytes(n_inst, n_points, n_req);
}

// The tail of the handle-less spicey_*_device entry points, behind their judge: the device opened, the launch enqueued, a
// failure as "<launcher>: <the runtime's text>" in the calling thread's error.
static int32_t launch_on_device(int32_t device, const char *launcher, const std::function<hipError_t()> &launch) {
  int ncu = 0;
  if (const int32_t rc = spicey_open_device(device, &ncu, g_err); rc != SPICEY_OK) return rc;
  const hipError_t e = launch();
  if (e != hipSuccess) { g_err = std::string(launcher) + ": " + hipGetErrorString(e); return SPICEY_ERR_HIP; }
  return SPICEY_OK;
}

extern "C" int32_t spicey_measure_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                         int32_t n_i, const SpiceyMeasReq *reqs, int32_t n_req, double *d_meas, void *d_work, int64_t work_bytes,
                                         void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  std::vector<SpiceyMeasDevReq> table;
  if (const int32_t rc = spicey_judge_measure("measure", spicey_meas_plan, spicey_meas_workspace_bytes, n_inst, n_points, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs,
                                              n_req, d_meas && d_work, work_bytes, table, g_err); rc != SPICEY_OK)
    return rc;
  return launch_on_device(device, "spicey_launch_measure", [&]() {
    return spicey_launch_measure(device, n_inst, n_points, dt, d_v, n_v, d_i, n_i, table.data(), n_req, d_meas, d_work, (hipStream_t)stream);
  });
}

// The lists of spicey_run_measure, spicey_run_measure_fourier, spicey_run_measure_timing, spicey_run_measure_spectrum and spicey_run_measure_power: per pass
// the caller's requests, their count and the out pointer.  entry = the entry point's own pass, its last: that list may not be empty, the lists
// before it may, and there are none behind it.
struct ReducedLists {
  int entry;
  const SpiceyMeasReq *reqs; int32_t n_req; double *meas;
  const SpiceyFourReq *freqs; int32_t n_four; double *four; int32_t four_stride;
  const SpiceyTimingReq *treqs; int32_t n_tim; double *timing;
  const SpiceySpecReq *sreqs = nullptr; int32_t n_spec = 0; double *spec = nullptr; int32_t spec_stride = 0;
  const SpiceyPowerReq *preqs = nullptr; int32_t n_power = 0; double *power = nullptr;
  // (spicey_run_reduced only, entry = -1: every list may be empty but not all of them, and a pass runs iff its count is > 0)
  const SpiceyValReq *vreqs = nullptr; int32_t n_values = 0; const SpiceyValPoint *pts = nullptr; int64_t n_pts = 0; double *values = nullptr;
  int32_t values_stride = 0;
};

// What spicey_run_mc adds to a reduced run: the draw in front of the transient, which then reads the drawn values, and behind
// the passes — whose rows stay on the device — the scalars and the reduction across the instances (tran_mc.hip).
struct TranMcCall {
  const SpiceyTranMcReq *req; const double *tol, *icdf;
  const SpiceyMcScalar *scalars; int32_t n_scalar;
  const double *lo, *hi, *probs; int32_t n_prob;
  double *stat; int64_t *sample; double *x;
};
// What spicey_run_sens and spicey_run_levels add to a reduced run: the design in front of the transient, which then reads the
// designed values, and behind the passes the scalars and — spicey_run_sens — the reduction across the instances (tran_sens.hip).
struct TranSensCall {
  int32_t mode;  // the design the entry point takes
  const SpiceyTranSensReq *req; const int32_t *act; const double *step; const int8_t *lvl; const double *tol;
  const SpiceyMcScalar *scalars; int32_t n_scalar;
  double *sens; int8_t *sign; double *bound; double *x;
};
namespace {
struct EventPair {  // (a call's own pair of timing events)
  hipEvent_t a = nullptr, b = nullptr;
  EventPair() = default;
  EventPair(const EventPair &) = delete;
  ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  hipError_t create() { const hipError_t e = hipEventCreate(&a); return e != hipSuccess ? e : hipEventCreate(&b); }
};
}  // namespace

// What the entry points share: one transient run into device buffers of this call's own, the reductions on the
// handle's stream behind it, and only their results and `iters` on the way back.  mc: null, or what spicey_run_mc adds; ts: null,
// or what spicey_run_sens / spicey_run_levels add (at most one of the two).
static int32_t run_reduced(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const ReducedLists &a, int32_t *iters,
                           const TranMcCall *mc = nullptr, const TranSensCall *ts = nullptr) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  const bool bound = mc || ts;  // the run reads scratch value arrays and its passes' rows stay on the device
  double *const outs[N_PASS] = {a.meas, a.four, a.timing, a.spec, a.power, a.values};
  const int32_t counts[N_PASS] = {a.n_req, a.n_four, a.n_tim, a.n_spec, a.n_power, a.n_values};
  if (mc) {
    h->last_tran_mc_ms = h->last_tran_mc_draw_ms = 0.0;
    const char *what = !mc->stat || !mc->sample ? "tran mc: null buffer"
                       : a.n_four > 0 || a.n_spec > 0 || a.n_values > 0 ? "tran mc: the fourier, spectrum and values lists are not reduced by this call (measure, timing and power are)"
                       : nullptr;
    if (what) { forget_last_run(h); h->err = what; return SPICEY_ERR_BAD_DESC; }
  }
  if (ts) {
    h->last_tran_sens_ms = h->last_tran_sens_design_ms = 0.0;
    const bool levels = ts->mode == SPICEY_TS_LEVELS;
    const char *what = (levels ? !ts->x : (!ts->sens || !ts->sign || !ts->bound)) ? "tran sens: null buffer"
                       : a.n_four > 0 || a.n_spec > 0 || a.n_values > 0 ? "tran sens: the fourier, spectrum and values lists are not reduced by this call (measure, timing and power are)"
                       : nullptr;
    if (what) { forget_last_run(h); h->err = what; return SPICEY_ERR_BAD_DESC; }
  }
  if (a.entry < 0) {
    int first_on = -1;
    for (int p = N_PASS - 1; p >= 0; p--) {
      if (counts[p] < 0) { forget_last_run(h); h->err = "reduced: every count must be >= 0"; return SPICEY_ERR_BAD_DESC; }
      if (counts[p] > 0) first_on = p;
    }
    if (first_on < 0) { forget_last_run(h); h->err = "reduced: every list is empty (at least one count must be > 0)"; return SPICEY_ERR_BAD_DESC; }
    // (a Monte Carlo run leaves the passes' rows on the device: what it brings back is `stat`, and the lists' result pointers
    // are not looked at)
    double *const some_out = mc ? mc->stat : ts ? (ts->mode == SPICEY_TS_LEVELS ? ts->x : ts->bound) : outs[first_on];
    if (const int32_t rc0 = check_run_args(h, steps, some_out, src_table, src_per_inst); rc0 != SPICEY_OK) return rc0;
    for (int p = 0; p < N_PASS && !bound; p++)
      if (counts[p] > 0 && !outs[p]) { h->err = "reduced: a result pointer is null where its count is > 0"; return SPICEY_ERR_BAD_DESC; }
  } else if (const int32_t rc0 = check_run_args(h, steps, outs[a.entry], src_table, src_per_inst); rc0 != SPICEY_OK) return rc0;
  if (a.entry == 1 && (a.n_req < 0 || (a.n_req > 0 && !a.meas))) { h->err = "fourier: n_req must be >= 0, and meas not null when n_req > 0"; return SPICEY_ERR_BAD_DESC; }
  if (a.entry == 2 && (a.n_req < 0 || (a.n_req > 0 && !a.meas) || a.n_four < 0 || (a.n_four > 0 && !a.four))) {
    h->err = "timing: n_req and n_four must be >= 0, and meas / four not null when their count is > 0";
    return SPICEY_ERR_BAD_DESC;
  }
  if (a.entry == 3 && (a.n_req < 0 || (a.n_req > 0 && !a.meas) || a.n_four < 0 || (a.n_four > 0 && !a.four) || a.n_tim < 0 || (a.n_tim > 0 && !a.timing))) {
    h->err = "spectrum: n_req, n_four and n_timing must be >= 0, and meas / four / timing not null when their count is > 0";
    return SPICEY_ERR_BAD_DESC;
  }
  if (a.entry == 4 && (a.n_req < 0 || (a.n_req > 0 && !a.meas) || a.n_four < 0 || (a.n_four > 0 && !a.four) || a.n_tim < 0 || (a.n_tim > 0 && !a.timing) ||
                       a.n_spec < 0 || (a.n_spec > 0 && !a.spec))) {
    h->err = "power: n_req, n_four, n_timing and n_spec must be >= 0, and meas / four / timing / spec not null when their count is > 0";
    return SPICEY_ERR_BAD_DESC;
  }
  // (a pass runs if it is the entry point's own, or an earlier one whose list is not empty)
  bool on[N_PASS];
  for (int p = 0; p < N_PASS; p++) on[p] = a.entry < 0 ? counts[p] > 0 : p == a.entry || (p < a.entry && counts[p] != 0);
  const SpiceyProg &P = h->hp.hdr;
  const int32_t ni = h->plan.n_inst;
  const int64_t np = steps + 1;
  // (a refused request list runs nothing; the buffers are this call's own)
  const int64_t work_bytes = on[PASS_MEASURE] ? spicey_meas_workspace_bytes(ni, np, a.n_req) : 0;
  std::vector<SpiceyMeasDevReq> table;
  if (on[PASS_MEASURE])
    if (const int32_t rc0 = spicey_judge_measure("measure", spicey_meas_plan, spicey_meas_workspace_bytes, ni, np, true, P.nOut, true, P.nCur, a.reqs, a.n_req, true,
                                                 work_bytes, table, h->err); rc0 != SPICEY_OK)
      return rc0;
  SpiceyFourPlan fplan;
  if (on[PASS_FOURIER] && !spicey_four_judge(ni, np, dt, true, P.nOut, true, P.nCur, a.freqs, a.n_four, true, a.four_stride, INT64_MAX, fplan, h->err))
    return SPICEY_ERR_BAD_DESC;
  SpiceyTimPlan tplan;
  if (on[PASS_TIMING] && !spicey_tim_judge(ni, np, dt, true, P.nOut, true, P.nCur, a.treqs, a.n_tim, true, INT64_MAX, tplan, h->err)) return SPICEY_ERR_BAD_DESC;
  SpiceySpecPlan splan;
  if (on[PASS_SPECTRUM] && !spicey_spec_judge(ni, np, dt, true, P.nOut, true, P.nCur, a.sreqs, a.n_spec, true, a.spec_stride, INT64_MAX, splan, h->err))
    return SPICEY_ERR_BAD_DESC;
  std::vector<SpiceyPowerDevReq> ptable;
  if (on[PASS_POWER] && !spicey_power_judge(ni, np, dt, true, P.nOut, true, P.nCur, a.preqs, a.n_power, true, INT64_MAX, ptable, h->err)) return SPICEY_ERR_BAD_DESC;
  SpiceyValPlan vplan;
  if (on[PASS_VALUES] && !spicey_val_judge(ni, np, dt, true, P.nOut, true, P.nCur, a.vreqs, a.n_values, a.pts, a.n_pts, on[PASS_TIMING], a.n_tim, true, a.values_stride,
                                           INT64_MAX, vplan, h->err))
    return SPICEY_ERR_BAD_DESC;
  // (the Monte Carlo request, tolerances, table, programs, limits and probabilities, judged on placeholder buffers: the scratch
  // arrays and the passes' rows are bound below)
  SpiceyMcDrawArgs mcD{};
  SpiceyTmcArgs mcA{};
  int64_t mc_work_bytes = 0;
  if (mc) {
    double dummy = 0.0, *some = &dummy;  // (any non-null pointer: the judges look at null-ness only)
    const int64_t draw_bytes = mc->req ? spicey_mc_draw_bytes(P.nR + P.nC + P.nL, mc->req->log2K) : 0;
    const int64_t red_bytes = spicey_tmc_reduce_bytes(ni, mc->n_scalar, mc->n_prob);
    const SpiceyMcRows jr[SPICEY_TMC_N_PASS] = {{on[PASS_MEASURE] ? some : nullptr, on[PASS_MEASURE] ? a.n_req : 0, 8},
                                                {on[PASS_TIMING] ? some : nullptr, on[PASS_TIMING] ? a.n_tim : 0, 8},
                                                {on[PASS_POWER] ? some : nullptr, on[PASS_POWER] ? a.n_power : 0, SPICEY_POWER_ROW}};
    if (!spicey_tmc_draw_judge(ni, P.nR, P.nC, P.nL, some, some, some, mc->tol, mc->icdf, mc->req, some, some, some, true, draw_bytes, mcD, h->err) ||
        !spicey_tmc_reduce_judge(ni, jr, mc->scalars, mc->n_scalar, mc->lo, mc->hi, mc->probs, mc->n_prob, true, red_bytes, mcA, h->err))
      return SPICEY_ERR_BAD_DESC;
    mc_work_bytes = std::max(draw_bytes, red_bytes);
  }
  // (the same for a sensitivity or levels run: the design's request and arrays, the programs, the steps and tolerances)
  SpiceyTsDesignArgs tsD{};
  SpiceyTmcArgs tsT{};
  SpiceyTsReduceArgs tsA{};
  std::vector<double> ts_tol_act;
  if (ts) {
    double dummy = 0.0, *some = &dummy;
    const int32_t nE = P.nR + P.nC + P.nL, nA = ts->req ? ts->req->nA : 0;
    const SpiceyMcRows jr[SPICEY_TMC_N_PASS] = {{on[PASS_MEASURE] ? some : nullptr, on[PASS_MEASURE] ? a.n_req : 0, 8},
                                                {on[PASS_TIMING] ? some : nullptr, on[PASS_TIMING] ? a.n_tim : 0, 8},
                                                {on[PASS_POWER] ? some : nullptr, on[PASS_POWER] ? a.n_power : 0, SPICEY_POWER_ROW}};
    if (!spicey_ts_design_judge(ni, P.nR, P.nC, P.nL, some, some, some, ts->req, ts->mode, ts->act, ts->step, ts->lvl, ts->tol, some, some, some, true, INT64_MAX, tsD,
                                h->err))
      return SPICEY_ERR_BAD_DESC;
    if (ts->mode == SPICEY_TS_LEVELS) {
      if (!spicey_ts_scalar_judge(ni, jr, ts->scalars, ts->n_scalar, true, tsT, h->err)) return SPICEY_ERR_BAD_DESC;
    } else {
      if (!ts->tol) { h->err = "tran sens: null buffer"; return SPICEY_ERR_BAD_DESC; }
      if (const char *what = spicey_ts_judge_tol(ts->tol, nE)) { h->err = std::string("tran sens: ") + what; return SPICEY_ERR_BAD_DESC; }
      ts_tol_act.resize((size_t)nA);
      for (int32_t k = 0; k < nA; k++) ts_tol_act[(size_t)k] = ts->tol[ts->act[k]];
      if (!spicey_ts_reduce_judge(ni, jr, ts->scalars, ts->n_scalar, ts->step, ts_tol_act.data(), nA, true, INT64_MAX, tsT, tsA, h->err)) return SPICEY_ERR_BAD_DESC;
    }
    mc_work_bytes = spicey_ts_workspace_bytes(ni, ts->n_scalar, nE, nA);
  }
  const auto names_a_current = [](const auto &list) { return std::any_of(list.begin(), list.end(), [](const auto &q) { return q.signal == 1; }); };
  const bool need_i = names_a_current(table) || names_a_current(fplan.table) || names_a_current(tplan.edges) || names_a_current(splan.table) ||
                      std::any_of(ptable.begin(), ptable.end(), [](const SpiceyPowerDevReq &q) { return q.a_signal == 1 || q.b_signal == 1; }) ||
                      names_a_current(vplan.traces) || std::any_of(vplan.points.begin(), vplan.points.end(), [](const SpiceyValDevPts &q) {
                        return q.signal == 1 || (q.kind == SPICEY_VAL_FIND && q.x_signal == 1);
                      });
  if (const int32_t rc0 = check_structure(h); rc0 != SPICEY_OK) return rc0;
  HIPCHK(h, hipSetDevice(h->device));
  static const char *const entry_name[N_PASS] = {"spicey_run_measure", "spicey_run_measure_fourier", "spicey_run_measure_timing", "spicey_run_measure_spectrum",
                                                 "spicey_run_measure_power", "spicey_run_reduced"};
  Roctx range_run(entry_name[a.entry < 0 ? N_PASS - 1 : a.entry]);
  HostRun r;
  hipStream_t st = h->q.stream;
  // The pass table: what the blocks below do per pass.  A further pass is one more entry here (and its judge above).
  struct Pass {
    bool on;
    size_t n_out, work_bytes;  // doubles of the result, bytes of the workspace
    double *out;               // the caller's
    const char *failed;        // prefix of a launch error's text
    std::function<hipError_t(double *d_out, void *d_work)> launch;
    DevBuf<double> d_out;
    DevBuf<uint8_t> d_work;
  };
  const double *d_timing_rows = nullptr;  // (the timing pass's device rows, once they are allocated: the values pass reads them)
  Pass pass[N_PASS] = {
      {on[PASS_MEASURE], (size_t)ni * (size_t)a.n_req * 8, (size_t)work_bytes, a.meas, "spicey_launch_measure: ", [&](double *d_out, void *d_work) {
         return spicey_launch_measure(h->device, ni, np, dt, r.d_v, P.nOut, r.d_i, P.nCur, table.data(), a.n_req, d_out, d_work, st);
       }},
      {on[PASS_FOURIER], (size_t)ni * (size_t)a.n_four * (size_t)a.four_stride, (size_t)fplan.workspace_bytes(ni), a.four, "spicey_launch_fourier: ",
       [&](double *d_out, void *d_work) {
         return spicey_launch_fourier(h->device, ni, np, dt, r.d_v, P.nOut, r.d_i, P.nCur, fplan, d_out, a.four_stride, d_work, st);
       }},
      {on[PASS_TIMING], (size_t)ni * (size_t)a.n_tim * 8, (size_t)tplan.workspace_bytes(ni, np), a.timing, "spicey_launch_timing: ", [&](double *d_out, void *d_work) {
         return spicey_launch_timing(h->device, ni, np, dt, r.d_v, P.nOut, r.d_i, P.nCur, tplan, d_out, d_work, st);
       }},
      {on[PASS_SPECTRUM], (size_t)ni * (size_t)a.n_spec * (size_t)a.spec_stride, (size_t)splan.workspace_bytes(), a.spec, "spicey_launch_spectrum: ",
       [&](double *d_out, void *d_work) {
         return spicey_launch_spectrum(h->device, ni, np, r.d_v, P.nOut, r.d_i, P.nCur, splan, d_out, a.spec_stride, d_work, st);
       }},
      {on[PASS_POWER], (size_t)ni * (size_t)a.n_power * SPICEY_POWER_ROW, on[PASS_POWER] ? (size_t)spicey_pow_workspace_bytes(ni, np, a.n_power) : 0, a.power,
       "spicey_launch_power: ", [&](double *d_out, void *d_work) {
         return spicey_launch_power(h->device, ni, np, r.d_v, P.nOut, r.d_i, P.nCur, ptable.data(), a.n_power, d_out, d_work, st);
       }},
      {on[PASS_VALUES], (size_t)ni * (size_t)a.n_values * (size_t)a.values_stride, on[PASS_VALUES] ? (size_t)vplan.workspace_bytes(ni) : 0, a.values,
       "spicey_launch_values: ", [&](double *d_out, void *d_work) {
         return spicey_launch_values(h->device, ni, np, dt, r.d_v, P.nOut, r.d_i, P.nCur, vplan, a.pts, d_timing_rows, a.n_tim, d_out, a.values_stride, d_work, st);
       }},
  };
  for (int p = 0; p < N_PASS; p++)
    if (pass[p].on) HIPCHK(h, h->q.want_pass_events(p));
  // (no current request: the run records no currents)
  if (const int32_t rc0 = r.stage(h, steps, src_table, src_per_inst, need_i, iters != nullptr); rc0 != SPICEY_OK) return rc0;
  for (Pass &t : pass) {
    if (!t.on) continue;
    HIPCHK(h, t.d_out.alloc(t.n_out));
    HIPCHK(h, t.d_work.alloc(t.work_bytes));
  }
  if (on[PASS_TIMING]) d_timing_rows = pass[PASS_TIMING].d_out;
  for (double &ms : h->last_pass_ms) ms = 0.0;
  // (a Monte Carlo run: the draw into scratch value arrays of this call's own, which the transient then reads; they live
  // until the call returns, so a launch that spicey_sync repeats reads them again)
  DevBuf<double> d_sR, d_sC, d_sL;
  DevBuf<uint8_t> d_mc_work;
  EventPair ev_draw, ev_red;
  const double *mc_vals[3] = {nullptr, nullptr, nullptr};
  if (bound) {
    HIPCHK(h, d_sR.alloc(std::max<size_t>(1, (size_t)ni * (size_t)P.nR)));
    HIPCHK(h, d_sC.alloc(std::max<size_t>(1, (size_t)ni * (size_t)P.nC)));
    HIPCHK(h, d_sL.alloc(std::max<size_t>(1, (size_t)ni * (size_t)P.nL)));
    HIPCHK(h, d_mc_work.alloc((size_t)mc_work_bytes));
    HIPCHK(h, ev_draw.create());
    HIPCHK(h, ev_red.create());
    HIPCHK(h, hipEventRecord(ev_draw.a, st));
    if (mc) {
      mcD.R = h->d_R; mcD.C = h->d_C; mcD.L = h->d_L; mcD.oR = d_sR; mcD.oC = d_sC; mcD.oL = d_sL;
      HIPCHK(h, spicey_launch_tmc_draw(h->device, mcD, mc->tol, mc->icdf, d_mc_work, st));
    } else {
      tsD.R = h->d_R; tsD.C = h->d_C; tsD.L = h->d_L; tsD.oR = d_sR; tsD.oC = d_sC; tsD.oL = d_sL;
      HIPCHK(h, spicey_launch_ts_design(h->device, tsD, ts->act, ts->step, ts->lvl, ts->tol, d_mc_work, st));
    }
    HIPCHK(h, hipEventRecord(ev_draw.b, st));
    mc_vals[0] = d_sR; mc_vals[1] = d_sC; mc_vals[2] = d_sL;
  }
  int32_t rc = run_device_src(h, steps, dt, r.d_src, src_per_inst, r.d_v, r.d_i, r.d_it, st, bound ? mc_vals : nullptr);
  if (rc != SPICEY_OK) return rc;
  const char *failed = "";
  auto reduce = [&]() {
    hipError_t e = hipSuccess;
    for (int p = 0; p < N_PASS && e == hipSuccess; p++) {
      Pass &t = pass[p];
      if (!t.on) continue;
      failed = t.failed;
      e = hipEventRecord(h->q.pass_ev[p][0], st);
      if (e == hipSuccess) e = t.launch(t.d_out, t.d_work);
      if (e == hipSuccess) e = hipEventRecord(h->q.pass_ev[p][1], st);
    }
    return e;
  };
  const int retries = h->group_retries;
  hipError_t e = reduce();
  rc = spicey_sync(h);  // (the stream's end: the transient's status, with the reductions behind it; also before the buffers go)
  // (group mode with group_retry: spicey_sync repeated the transient behind the reductions, so the reductions run again)
  if (e == hipSuccess && h->group_retries != retries && rc == SPICEY_OK && (e = reduce()) == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { h->err = std::string(failed) + hipGetErrorString(e); return SPICEY_ERR_HIP; }
  if (rc == SPICEY_OK || rc == SPICEY_ERR_SINGULAR) {
    for (int p = 0; p < N_PASS; p++)
      if (pass[p].on) StreamTimers::elapsed(h->q.pass_ev[p][0], h->q.pass_ev[p][1], &h->last_pass_ms[p]);
    if (mc) {
      StreamTimers::elapsed(ev_draw.a, ev_draw.b, &h->last_tran_mc_draw_ms);
      // a sample is valid iff it finished; with none nothing is reduced and the outputs stay as they are
      std::vector<int32_t> ist((size_t)ni);
      std::vector<uint8_t> valid((size_t)ni);
      spicey_last_inst_status(h, ist.data());
      int32_t n_valid = 0;
      for (int32_t s = 0; s < ni; s++) n_valid += valid[(size_t)s] = ist[(size_t)s] == 0;
      if (n_valid > 0) {
        // (the record was judged before anything ran, on placeholders: the passes' rows take their place)
        const int row_pass[SPICEY_TMC_N_PASS] = {PASS_MEASURE, PASS_TIMING, PASS_POWER};
        for (int p = 0; p < SPICEY_TMC_N_PASS; p++) mcA.rows[p] = mcA.n_rows[p] > 0 ? (const double *)pass[row_pass[p]].d_out : nullptr;
        const size_t n_x = (size_t)ni * (size_t)mc->n_scalar, n_stat = (size_t)mc->n_scalar * (size_t)(SPICEY_TMC_STAT_HEAD + 2 * mc->n_prob);
        DevBuf<double> d_x, d_stat;
        DevBuf<int64_t> d_sample;
        HIPCHK(h, d_x.alloc(n_x));
        HIPCHK(h, d_stat.alloc(n_stat));
        HIPCHK(h, d_sample.alloc((size_t)ni * 2));
        HIPCHK(h, hipEventRecord(ev_red.a, st));
        HIPCHK(h, spicey_launch_tmc_reduce(h->device, mcA, mc->scalars, n_valid == ni ? nullptr : valid.data(), mc->lo, mc->hi, mc->probs, d_x, d_stat, d_sample,
                                           d_mc_work, st));
        HIPCHK(h, hipEventRecord(ev_red.b, st));
        HIPCHK(h, hipMemcpyAsync(mc->stat, d_stat, n_stat * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync(mc->sample, d_sample, (size_t)ni * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (mc->x) HIPCHK(h, hipMemcpyAsync(mc->x, d_x, n_x * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        StreamTimers::elapsed(ev_red.a, ev_red.b, &h->last_tran_mc_ms);
      } else if (rc == SPICEY_OK) {
        h->err = "tran mc: no valid sample";
        rc = SPICEY_ERR_SINGULAR;
      } else h->err += " (tran mc: no valid sample, nothing reduced)";
    } else if (ts) {
      StreamTimers::elapsed(ev_draw.a, ev_draw.b, &h->last_tran_sens_design_ms);
      // an instance is valid iff it finished; a sensitivity needs the nominal instance, a levels run any instance
      const bool levels = ts->mode == SPICEY_TS_LEVELS;
      std::vector<int32_t> ist((size_t)ni);
      std::vector<uint8_t> valid((size_t)ni);
      spicey_last_inst_status(h, ist.data());
      int32_t n_valid = 0;
      for (int32_t s = 0; s < ni; s++) n_valid += valid[(size_t)s] = ist[(size_t)s] == 0;
      if (levels ? n_valid > 0 : valid[0] != 0) {
        const int row_pass[SPICEY_TMC_N_PASS] = {PASS_MEASURE, PASS_TIMING, PASS_POWER};
        for (int p = 0; p < SPICEY_TMC_N_PASS; p++) tsT.rows[p] = tsT.n_rows[p] > 0 ? (const double *)pass[row_pass[p]].d_out : nullptr;
        const uint8_t *va = n_valid == ni ? nullptr : valid.data();
        const size_t n_x = (size_t)ni * (size_t)ts->n_scalar, n_el = levels ? 0 : (size_t)ts->n_scalar * (size_t)tsA.nA;
        DevBuf<double> d_x, d_sens, d_bound;
        DevBuf<int8_t> d_sign;
        HIPCHK(h, d_x.alloc(n_x));
        if (!levels) {
          HIPCHK(h, d_sens.alloc(2 * n_el));
          HIPCHK(h, d_sign.alloc(n_el));
          HIPCHK(h, d_bound.alloc((size_t)ts->n_scalar * SPICEY_TS_BOUND_ROW));
        }
        HIPCHK(h, hipEventRecord(ev_red.a, st));
        if (levels) HIPCHK(h, spicey_launch_tmc_scalars(h->device, tsT, ts->scalars, va, nullptr, nullptr, nullptr, d_x, d_mc_work, st));
        else HIPCHK(h, spicey_launch_ts_reduce(h->device, tsT, tsA, ts->scalars, va, ts->step, ts_tol_act.data(), d_x, d_sens, d_sign, d_bound, d_mc_work, st));
        HIPCHK(h, hipEventRecord(ev_red.b, st));
        if (!levels) {
          HIPCHK(h, hipMemcpyAsync(ts->sens, d_sens, 2 * n_el * sizeof(double), hipMemcpyDeviceToHost, st));
          HIPCHK(h, hipMemcpyAsync(ts->sign, d_sign, n_el, hipMemcpyDeviceToHost, st));
          HIPCHK(h, hipMemcpyAsync(ts->bound, d_bound, (size_t)ts->n_scalar * SPICEY_TS_BOUND_ROW * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        if (ts->x) HIPCHK(h, hipMemcpyAsync(ts->x, d_x, n_x * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        StreamTimers::elapsed(ev_red.a, ev_red.b, &h->last_tran_sens_ms);
      } else if (rc == SPICEY_OK) {
        h->err = levels ? "tran sens: no valid instance" : "tran sens: the nominal instance is not valid";
        rc = SPICEY_ERR_SINGULAR;
      } else h->err += levels ? " (tran sens: no valid instance, nothing reduced)" : " (tran sens: the nominal instance is not valid, nothing reduced)";
    } else {
      Roctx range_copy("spicey_run_measure:results");
      for (const Pass &t : pass)
        if (t.on) HIPCHK(h, hipMemcpy(t.out, t.d_out, t.n_out * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (const int32_t rc0 = r.copy_out(h, nullptr, nullptr, iters); rc0 != SPICEY_OK) return rc0;
  }
  return rc;
}

extern "C" int32_t spicey_run_mc(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *l,
                                 const SpiceyTranMcReq *req, const double *tol, const double *icdf, const SpiceyMcScalar *scalars, int32_t n_scalar,
                                 const double *lo, const double *hi, const double *probs, int32_t n_prob, double *stat, int64_t *sample, double *x,
                                 int32_t *iters) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  const char *what = !l ? "tran mc: lists must not be null"
                     : l->struct_bytes < (int64_t)sizeof(SpiceyReducedLists) ? "tran mc: lists.struct_bytes is smaller than sizeof(SpiceyReducedLists)"
                     : l->reserved != 0 ? "tran mc: lists.reserved must be 0" : nullptr;
  if (what) { forget_last_run(h); h->err = what; return SPICEY_ERR_BAD_DESC; }
  ReducedLists a{-1, l->reqs, l->n_req, nullptr, l->freqs, l->n_four, nullptr, l->four_stride, l->treqs, l->n_timing, nullptr,
                 l->sreqs, l->n_spec, nullptr, l->spec_stride, l->preqs, l->n_power, nullptr};
  a.vreqs = l->vreqs; a.n_values = l->n_values; a.pts = l->pts; a.n_pts = l->n_pts; a.values_stride = l->values_stride;
  const TranMcCall mc{req, tol, icdf, scalars, n_scalar, lo, hi, probs, n_prob, stat, sample, x};
  return run_reduced(h, steps, dt, src_table, src_per_inst, a, iters, &mc);
}

extern "C" double spicey_last_tran_mc_ms(SpiceyHandle *h) { return h ? h->last_tran_mc_ms : 0.0; }
extern "C" double spicey_last_tran_mc_draw_ms(SpiceyHandle *h) { return h ? h->last_tran_mc_draw_ms : 0.0; }

// The lists of spicey_run_sens / spicey_run_levels, judged as spicey_run_mc's.
static int32_t run_tran_sens(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *l, int32_t *iters,
                             const TranSensCall &ts) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  const char *what = !l ? "tran sens: lists must not be null"
                     : l->struct_bytes < (int64_t)sizeof(SpiceyReducedLists) ? "tran sens: lists.struct_bytes is smaller than sizeof(SpiceyReducedLists)"
                     : l->reserved != 0 ? "tran sens: lists.reserved must be 0" : nullptr;
  if (what) { forget_last_run(h); h->err = what; return SPICEY_ERR_BAD_DESC; }
  ReducedLists a{-1, l->reqs, l->n_req, nullptr, l->freqs, l->n_four, nullptr, l->four_stride, l->treqs, l->n_timing, nullptr,
                 l->sreqs, l->n_spec, nullptr, l->spec_stride, l->preqs, l->n_power, nullptr};
  a.vreqs = l->vreqs; a.n_values = l->n_values; a.pts = l->pts; a.n_pts = l->n_pts; a.values_stride = l->values_stride;
  return run_reduced(h, steps, dt, src_table, src_per_inst, a, iters, nullptr, &ts);
}

extern "C" int32_t spicey_run_sens(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *l,
                                   const SpiceyTranSensReq *req, const int32_t *act, const double *step, const double *tol, const SpiceyMcScalar *scalars,
                                   int32_t n_scalar, double *sens, int8_t *sign, double *bound, double *x, int32_t *iters) {
  return run_tran_sens(h, steps, dt, src_table, src_per_inst, l, iters, {SPICEY_TS_ONE_AT_A_TIME, req, act, step, nullptr, tol, scalars, n_scalar, sens, sign, bound, x});
}

extern "C" int32_t spicey_run_levels(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *l,
                                     const SpiceyTranSensReq *req, const int8_t *lvl, const double *tol, const SpiceyMcScalar *scalars, int32_t n_scalar, double *x,
                                     int32_t *iters) {
  return run_tran_sens(h, steps, dt, src_table, src_per_inst, l, iters, {SPICEY_TS_LEVELS, req, nullptr, nullptr, lvl, tol, scalars, n_scalar, nullptr, nullptr, nullptr, x});
}

extern "C" double spicey_last_tran_sens_ms(SpiceyHandle *h) { return h ? h->last_tran_sens_ms : 0.0; }
extern "C" double spicey_last_tran_sens_design_ms(SpiceyHandle *h) { return h ? h->last_tran_sens_design_ms : 0.0; }

extern "C" int32_t spicey_run_measure(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyMeasReq *reqs,
                                      int32_t n_req, double *meas, int32_t *iters) {
  return run_reduced(h, steps, dt, src_table, src_per_inst, {0, reqs, n_req, meas, nullptr, 0, nullptr, 0, nullptr, 0, nullptr}, iters);
}

extern "C" int32_t spicey_run_measure_fourier(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyMeasReq *reqs,
                                              int32_t n_req, double *meas, const SpiceyFourReq *freqs, int32_t n_four, double *four, int32_t four_stride,
                                              int32_t *iters) {
  return run_reduced(h, steps, dt, src_table, src_per_inst, {1, reqs, n_req, meas, freqs, n_four, four, four_stride, nullptr, 0, nullptr}, iters);
}

extern "C" int32_t spicey_run_measure_timing(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyMeasReq *reqs,
                                             int32_t n_req, double *meas, const SpiceyFourReq *freqs, int32_t n_four, double *four, int32_t four_stride,
                                             const SpiceyTimingReq *treqs, int32_t n_timing, double *timing, int32_t *iters) {
  return run_reduced(h, steps, dt, src_table, src_per_inst, {2, reqs, n_req, meas, freqs, n_four, four, four_stride, treqs, n_timing, timing}, iters);
}

extern "C" int32_t spicey_run_measure_spectrum(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyMeasReq *reqs,
                                               int32_t n_req, double *meas, const SpiceyFourReq *freqs, int32_t n_four, double *four, int32_t four_stride,
                                               const SpiceyTimingReq *treqs, int32_t n_timing, double *timing, const SpiceySpecReq *sreqs, int32_t n_spec, double *spec,
                                               int32_t spec_stride, int32_t *iters) {
  return run_reduced(h, steps, dt, src_table, src_per_inst,
                     {3, reqs, n_req, meas, freqs, n_four, four, four_stride, treqs, n_timing, timing, sreqs, n_spec, spec, spec_stride}, iters);
}

extern "C" int32_t spicey_run_measure_power(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyMeasReq *reqs,
                                            int32_t n_req, double *meas, const SpiceyFourReq *freqs, int32_t n_four, double *four, int32_t four_stride,
                                            const SpiceyTimingReq *treqs, int32_t n_timing, double *timing, const SpiceySpecReq *sreqs, int32_t n_spec, double *spec,
                                            int32_t spec_stride, const SpiceyPowerReq *preqs, int32_t n_power, double *power, int32_t *iters) {
  return run_reduced(h, steps, dt, src_table, src_per_inst,
                     {4, reqs, n_req, meas, freqs, n_four, four, four_stride, treqs, n_timing, timing, sreqs, n_spec, spec, spec_stride, preqs, n_power, power}, iters);
}

extern "C" int32_t spicey_run_reduced(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *l,
                                      int32_t *iters) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  const char *what = !l ? "reduced: lists must not be null"
                     : l->struct_bytes < (int64_t)sizeof(SpiceyReducedLists) ? "reduced: struct_bytes is smaller than sizeof(SpiceyReducedLists)"
                     : l->reserved != 0 ? "reduced: reserved must be 0" : nullptr;
  if (what) { forget_last_run(h); h->err = what; return SPICEY_ERR_BAD_DESC; }
  ReducedLists a{-1, l->reqs, l->n_req, l->meas, l->freqs, l->n_four, l->four, l->four_stride, l->treqs, l->n_timing, l->timing,
                 l->sreqs, l->n_spec, l->spec, l->spec_stride, l->preqs, l->n_power, l->power};
  a.vreqs = l->vreqs; a.n_values = l->n_values; a.pts = l->pts; a.n_pts = l->n_pts; a.values = l->values; a.values_stride = l->values_stride;
  return run_reduced(h, steps, dt, src_table, src_per_inst, a, iters);
}

extern "C" double spicey_last_measure_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_MEASURE] : 0.0; }
extern "C" double spicey_last_fourier_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_FOURIER] : 0.0; }
extern "C" double spicey_last_timing_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_TIMING] : 0.0; }
extern "C" double spicey_last_spectrum_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_SPECTRUM] : 0.0; }
extern "C" double spicey_last_power_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_POWER] : 0.0; }
extern "C" double spicey_last_values_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_VALUES] : 0.0; }

// Edge timing (include/spicey_hip.h): the reduction of timing.hip on any device buffers, no handle.
extern "C" int64_t spicey_timing_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyTimingReq *reqs, int32_t n_req) {
  return spicey_tim_workspace_bytes(n_inst, n_points, reqs, n_req);
}

extern "C" int32_t spicey_timing_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                        int32_t n_i, const SpiceyTimingReq *reqs, int32_t n_req, double *d_out, void *d_work, int64_t work_bytes,
                                        void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyTimPlan plan;
  if (!spicey_tim_judge(n_inst, n_points, dt, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs, n_req, d_out && d_work, work_bytes, plan, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_timing", [&]() {
    return spicey_launch_timing(device, n_inst, n_points, dt, d_v, n_v, d_i, n_i, plan, d_out, d_work, (hipStream_t)stream);
  });
}

// Spectrum (include/spicey_hip.h): the FFT pass of spectrum.hip on any device buffers, no handle.
extern "C" int64_t spicey_spectrum_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceySpecReq *reqs, int32_t n_req) {
  return spicey_spec_workspace_bytes(n_inst, n_points, reqs, n_req);
}

extern "C" int32_t spicey_spectrum_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                          int32_t n_i, const SpiceySpecReq *reqs, int32_t n_req, double *d_out, int32_t out_stride, void *d_work,
                                          int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceySpecPlan plan;
  if (!spicey_spec_judge(n_inst, n_points, dt, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs, n_req, d_out && d_work, out_stride, work_bytes, plan, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_spectrum", [&]() {
    return spicey_launch_spectrum(device, n_inst, n_points, d_v, n_v, d_i, n_i, plan, d_out, out_stride, d_work, (hipStream_t)stream);
  });
}

// Products of two signals (include/spicey_hip.h): the reduction of power.hip on any device buffers, no handle.
extern "C" int64_t spicey_power_workspace_bytes(int32_t n_inst, int64_t n_points, int32_t n_req) {
  return spicey_pow_workspace_bytes(n_inst, n_points, n_req);
}

extern "C" int32_t spicey_power_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                       int32_t n_i, const SpiceyPowerReq *reqs, int32_t n_req, double *d_out, void *d_work, int64_t work_bytes,
                                       void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  std::vector<SpiceyPowerDevReq> table;
  if (!spicey_power_judge(n_inst, n_points, dt, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs, n_req, d_out && d_work, work_bytes, table, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_power", [&]() {
    return spicey_launch_power(device, n_inst, n_points, d_v, n_v, d_i, n_i, table.data(), n_req, d_out, d_work, (hipStream_t)stream);
  });
}

// Waveform values (include/spicey_hip.h): the pass of values.hip on any device buffers, no handle.
extern "C" int64_t spicey_values_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyValReq *reqs, int32_t n_req, int64_t n_pts) {
  return spicey_val_workspace_bytes(n_inst, n_points, reqs, n_req, n_pts);
}

extern "C" int32_t spicey_values_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                        int32_t n_i, const SpiceyValReq *reqs, int32_t n_req, const SpiceyValPoint *pts, int64_t n_pts, const double *d_timing,
                                        int32_t n_timing, double *d_out, int32_t out_stride, void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyValPlan plan;
  if (!spicey_val_judge(n_inst, n_points, dt, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs, n_req, pts, n_pts, d_timing != nullptr, n_timing, d_out && d_work,
                        out_stride, work_bytes, plan, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_values", [&]() {
    return spicey_launch_values(device, n_inst, n_points, dt, d_v, n_v, d_i, n_i, plan, pts, d_timing, n_timing, d_out, out_stride, d_work, (hipStream_t)stream);
  });
}

// Harmonics (include/spicey_hip.h): the reduction of fourier.hip on any device buffers, no handle.
extern "C" int64_t spicey_fourier_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyFourReq *reqs, int32_t n_req) {
  return spicey_four_workspace_bytes(n_inst, n_points, reqs, n_req);
}

extern "C" int32_t spicey_fourier_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                         int32_t n_i, const SpiceyFourReq *reqs, int32_t n_req, double *d_out, int32_t out_stride, void *d_work,
                                         int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyFourPlan plan;
  if (!spicey_four_judge(n_inst, n_points, dt, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs, n_req, d_out && d_work, out_stride, work_bytes, plan, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_fourier", [&]() {
    return spicey_launch_fourier(device, n_inst, n_points, dt, d_v, n_v, d_i, n_i, plan, d_out, out_stride, d_work, (hipStream_t)stream);
  });
}

// The same for an AC sweep's complex buffers (include/spicey_hip.h): the reduction of ac_measure.hip, no handle.
extern "C" int64_t spicey_ac_measure_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t n_req) {
  return spicey_acm_workspace_bytes(n_inst, n_freq, n_req);
}

extern "C" int32_t spicey_ac_measure_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                            const SpiceyAcMeasReq *reqs, int32_t n_req, double *d_meas, void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  std::vector<SpiceyAcMeasDevReq> table;
  if (const int32_t rc = spicey_judge_measure("ac measure", spicey_acm_plan, spicey_acm_workspace_bytes, n_inst, n_freq, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs,
                                              n_req, d_meas && d_work, work_bytes, table, g_err); rc != SPICEY_OK)
    return rc;
  return launch_on_device(device, "spicey_launch_ac_measure", [&]() {
    return spicey_launch_ac_measure(device, n_inst, n_freq, d_v, n_v, d_i, n_i, table.data(), n_req, d_meas, d_work, (hipStream_t)stream);
  });
}

// Thermal noise of an injected AC sweep (include/spicey_hip.h): the reduction of noise.hip on any device buffers, no handle.
extern "C" int64_t spicey_ac_noise_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nR) { return spicey_noise_workspace_bytes(n_inst, n_freq, nR); }

extern "C" int32_t spicey_ac_noise_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                          const double *d_R, int32_t nR, const double *d_freqs, const SpiceyAcNoiseReq *req, double *d_spec, double *d_contrib,
                                          double *d_total, void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyNoiseArgs A;
  if (!spicey_noise_judge(n_inst, n_freq, d_v, n_v, d_i, n_i, d_R, nR, d_freqs, req, d_spec && d_contrib && d_total && d_work, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_noise", [&]() { return spicey_launch_noise(device, A, d_spec, d_contrib, d_total, d_work, (hipStream_t)stream); });
}

// AC sensitivities of a direct and an adjoint sweep (include/spicey_hip.h): the reduction of sens.hip on any device buffers, no
// handle.  tol is a HOST array: judged here, uploaded through the workspace.
extern "C" int64_t spicey_ac_sens_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nE) { return spicey_sens_workspace_bytes(n_inst, n_freq, nE); }

extern "C" int32_t spicey_ac_sens_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v_dir, int32_t n_v, const double *d_i_dir,
                                         const double *d_i_adj, int32_t n_i, const double *d_R, const double *d_C, const double *d_L, const double *tol,
                                         const double *d_freqs, const SpiceyAcSensReq *req, double *d_spec, double *d_peak, double *d_full, void *d_work,
                                         int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceySensArgs A;
  if (!spicey_sens_judge(n_inst, n_freq, d_v_dir, n_v, d_i_dir, d_i_adj, n_i, d_R, d_C, d_L, tol, d_freqs, req, d_spec && d_peak && d_work, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_sens", [&]() { return spicey_launch_sens(device, A, tol, d_spec, d_peak, d_full, d_work, (hipStream_t)stream); });
}

extern "C" int64_t spicey_ac_mc_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nE, int32_t log2K, int32_t n_rank) {
  return spicey_mc_workspace_bytes(n_inst, n_freq, nE, log2K, n_rank);
}

extern "C" int32_t spicey_ac_mc_draw_device(int32_t device, int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C,
                                            const double *d_L, const double *tol, const double *icdf, const SpiceyAcMcReq *req, double *d_Rinv_out,
                                            double *d_C_out, double *d_L_out, void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyMcDrawArgs A;
  if (!spicey_mc_draw_judge(n_inst, nR, nC, nL, d_R, d_C, d_L, tol, icdf, req, d_Rinv_out, d_C_out, d_L_out, d_work != nullptr, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_mc_draw", [&]() { return spicey_launch_mc_draw(device, A, tol, icdf, d_work, (hipStream_t)stream); });
}

extern "C" int32_t spicey_ac_mc_reduce_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const uint8_t *valid,
                                              const double *lo, const double *hi, const int64_t *ranks, int32_t n_rank, const SpiceyAcMcReq *req,
                                              int64_t *d_sample, double *d_freq, void *d_work, int64_t work_bytes, void *stream) {
  SpiceyMcReduceArgs A;
  if (!spicey_mc_reduce_judge(n_inst, n_freq, d_v, n_v, valid, ranks, n_rank, req, d_sample && d_freq && d_work, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_mc_reduce",
                          [&]() { return spicey_launch_mc_reduce(device, A, valid, lo, hi, ranks, d_sample, d_freq, d_work, (hipStream_t)stream); });
}

// Monte Carlo of transient runs (include/spicey_hip.h): the draw and the reduction of tran_mc.hip on any device buffers, no handle.
extern "C" int64_t spicey_tran_mc_workspace_bytes(int32_t n_inst, int32_t n_scalar, int32_t nE, int32_t log2K, int32_t n_prob) {
  return spicey_tmc_workspace_bytes(n_inst, n_scalar, nE, log2K, n_prob);
}

extern "C" int32_t spicey_tran_mc_draw_device(int32_t device, int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C,
                                              const double *d_L, const double *tol, const double *icdf, const SpiceyTranMcReq *req, double *d_R_out,
                                              double *d_C_out, double *d_L_out, void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyMcDrawArgs A;
  if (!spicey_tmc_draw_judge(n_inst, nR, nC, nL, d_R, d_C, d_L, tol, icdf, req, d_R_out, d_C_out, d_L_out, d_work != nullptr, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_tmc_draw", [&]() { return spicey_launch_tmc_draw(device, A, tol, icdf, d_work, (hipStream_t)stream); });
}

extern "C" int32_t spicey_tran_mc_reduce_device(int32_t device, int32_t n_inst, const SpiceyMcRows *rows, const SpiceyMcScalar *scalars, int32_t n_scalar,
                                                const uint8_t *valid, const double *lo, const double *hi, const double *probs, int32_t n_prob, double *d_x,
                                                double *d_stat, int64_t *d_sample, void *d_work, int64_t work_bytes, void *stream) {
  SpiceyTmcArgs A;
  if (!spicey_tmc_reduce_judge(n_inst, rows, scalars, n_scalar, lo, hi, probs, n_prob, d_x && d_stat && d_sample && d_work, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_tmc_reduce", [&]() {
    return spicey_launch_tmc_reduce(device, A, scalars, valid, lo, hi, probs, d_x, d_stat, d_sample, d_work, (hipStream_t)stream);
  });
}

// Sensitivities and corners of transient measurements (include/spicey_hip.h): the design and the reduction of tran_sens.hip on any
// device buffers, no handle.
extern "C" int64_t spicey_tran_sens_workspace_bytes(int32_t n_inst, int32_t n_scalar, int32_t nE, int32_t nA) {
  return spicey_ts_workspace_bytes(n_inst, n_scalar, nE, nA);
}

extern "C" int32_t spicey_tran_sens_design_device(int32_t device, int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C,
                                                  const double *d_L, const SpiceyTranSensReq *req, const int32_t *act, const double *step, const int8_t *lvl,
                                                  const double *tol, double *d_R_out, double *d_C_out, double *d_L_out, void *d_work, int64_t work_bytes,
                                                  void *stream) {
  SpiceyTsDesignArgs A;
  if (!spicey_ts_design_judge(n_inst, nR, nC, nL, d_R, d_C, d_L, req, -1, act, step, lvl, tol, d_R_out, d_C_out, d_L_out, d_work != nullptr, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_ts_design", [&]() { return spicey_launch_ts_design(device, A, act, step, lvl, tol, d_work, (hipStream_t)stream); });
}

extern "C" int32_t spicey_tran_sens_reduce_device(int32_t device, int32_t n_inst, const SpiceyMcRows *rows, const SpiceyMcScalar *scalars, int32_t n_scalar,
                                                  const uint8_t *valid, const double *step, const double *tol_act, int32_t nA, double *d_x, double *d_sens,
                                                  int8_t *d_sign, double *d_bound, void *d_work, int64_t work_bytes, void *stream) {
  SpiceyTmcArgs T;
  SpiceyTsReduceArgs A;
  if (!spicey_ts_reduce_judge(n_inst, rows, scalars, n_scalar, step, tol_act, nA, d_x && d_sens && d_sign && d_bound && d_work, work_bytes, T, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_ts_reduce", [&]() {
    return spicey_launch_ts_reduce(device, T, A, scalars, valid, step, tol_act, d_x, d_sens, d_sign, d_bound, d_work, (hipStream_t)stream);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// Several devices behind one handle: instance shards, one SpiceyHandle per shard, host threads around the blocking runs.
#include <thread>

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
