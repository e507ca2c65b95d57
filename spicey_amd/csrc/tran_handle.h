// tran_handle.h — what the sources of the transient C-ABI share (spicey_abi.cpp: the handle's life, uploads, runs and state;
// reduced_abi.cpp: the reduced-run driver behind spicey_run_measure* / spicey_run_reduced / spicey_run_mc / spicey_run_sens /
// spicey_run_levels; device_abi.cpp: the handle-less spicey_*_device entry points): the handle, the device side of a run on host
// buffers, the roctx ranges, a call's own event pair, and the run plumbing of spicey_abi.cpp the driver goes through.  Private.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <dlfcn.h>
#include <string>
#include <vector>

#include "../../include/spicey_hip.h"
#include "devbuf.h"
#include "exact_plan.h"
#include "kernels.h"
#include "launch_plan.h"
#include "symbolic.h"

// The instance state a transient step carries: C_vprev, L_iprev, D_vdprev, S_ison ([n_inst][nC | nL | nD | nS] each).
struct StatePtrs { double *Cv, *Li, *Dv; int32_t *Son; };
struct StateBufs {
  DevBuf<double> Cv, Li, Dv;
  DevBuf<int32_t> Son;
  StatePtrs ptrs() const { return {Cv, Li, Dv, Son}; }
};

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
  double last_pss_ms = 0.0, last_pss_tran_ms = 0.0;  // the last spicey_run_pss: its designs and updates, its transients, summed over the iterations
  double last_fit_ms = 0.0, last_fit_tran_ms = 0.0;  // the last spicey_run_fit: its designs and updates, its transients, summed over the iterations
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

// (C++ linkage, kept out of the library's dynamic symbols)
#define SPICEY_PRIVATE __attribute__((visibility("hidden")))
SPICEY_PRIVATE extern thread_local std::string g_err;  // message of the calling thread's last failed call that has no handle to hang it on
// spicey_abi.cpp: a new run begins; the refusals of every transient entry point, in their order; the body of spicey_run_device_src
SPICEY_PRIVATE void forget_last_run(SpiceyHandle *h);
SPICEY_PRIVATE int32_t check_run_args(SpiceyHandle *h, int64_t steps, const void *out, const void *src, int32_t src_per_inst);
SPICEY_PRIVATE int32_t check_structure(SpiceyHandle *h);
SPICEY_PRIVATE int32_t run_device_src(SpiceyHandle *h, int64_t steps, double dt, const double *d_src_table, int32_t src_per_inst, double *d_out_v, double *d_out_i,
                                      int32_t *d_iters, void *stream, const double *const *vals);

// roctx ranges around the host-side phases (SURVEY §5 tracing hook): `rocprofv3 --marker-trace` shows symbolic phase, uploads,
// kernel and result copies as named ranges.  The marker library is looked up at run time (no link dependency: without it,
// or outside a profiler, the ranges cost one null check).
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

struct EventPair {  // (a call's own pair of timing events)
  hipEvent_t a = nullptr, b = nullptr;
  EventPair() = default;
  EventPair(const EventPair &) = delete;
  ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  hipError_t create() { const hipError_t e = hipEventCreate(&a); return e != hipSuccess ? e : hipEventCreate(&b); }
};
