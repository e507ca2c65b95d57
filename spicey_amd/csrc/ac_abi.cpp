// ac_abi.cpp — the AC half of the C-ABI (spicey_ac_* of include/spicey_hip.h).  Host code only; the kernels and their
// launchers are in ac.hip, ac_exact.hip and ac_measure.hip.  (hip_runtime.h: the run structs SpiceyAcRun and
// SpiceyAcExactRun are defined beside the device code of ac_exec.h / ac_exact_exec.h.)
//
// One SpiceyAcHandle serves both engines: it owns the device, the dimensions, the stream and its events, 1/R, C and L on
// the device, the error text, the per-instance status and the timings, and ac_sweep() stages, times and finishes every
// sweep.  An engine (AcEngine) contributes its plan and program, its run struct and the launch of a range of slots:
//   AcSparse   the level-scheduled sparse LU of the transient program in complex arithmetic (ac_exec.h): one workgroup per
//              (instance, frequency) slot, or the resident sweep for batches that outnumber the CUs; slots whose static
//              pivot order fails are re-solved dense with partial pivoting
//   AcExact    SpiceyOptions.interpreter = 3: the reference's own dense solve, bit for bit (ac_exact_exec.h)
// No CPU path: without a HIP device spicey_ac_create returns SPICEY_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/spicey_hip.h"
#include "ac_exact_exec.h"
#include "ac_measure.h"
#include "ac_measure_exec.h"
#include "ac_sweep.h"
#include "devbuf.h"
#include "kernels.h"
#include "mc.h"
#include "noise.h"
#include "sens.h"
#include "symbolic.h"

struct AcDims { int32_t n_inst = 0, n_out = 0, n_cur = 0, n_v = 0; };

// The device buffers of one sweep, as both run structs name them.
struct AcBuffers {
  const double *R_inv, *C_val, *L_val, *freqs, *vph;
  double *out_v, *out_i;
  void *gW;  // [slots of a launch][slot_ws_bytes()], or null
  int32_t *status;
  int64_t n_freq;
};

struct AcEngine {
  virtual ~AcEngine() = default;
  // the descriptor and option checks that need no device, the host program, the dimensions
  virtual int32_t plan(const SpiceyDesc *desc, const SpiceyOptions &opt, AcDims &dims, std::string &err) = 0;
  // with the device open: what is left to refuse, then the program into device memory
  virtual int32_t upload(SpiceyAcHandle *h, const SpiceyDesc *desc) = 0;
  virtual bool structurally_singular() const { return false; }
  // slots per launch of a sweep over `slots`, and the bytes of global workspace each of them needs (0: LDS)
  virtual int64_t chunk(const SpiceyAcHandle *h, int64_t slots, int64_t n_freq) = 0;
  virtual size_t slot_ws_bytes() const = 0;
  // the current injection of the next sweep (null: none), as node ids already checked against the descriptor; an engine
  // without injection refuses
  virtual int32_t set_inject(const SpiceyAcInject *inj, std::string &err) {
    if (!inj) return SPICEY_OK;
    err = "inject: the reference-order engine (interpreter = 3) takes no current injection";
    return SPICEY_ERR_BAD_DESC;
  }
  virtual int32_t bind(SpiceyAcHandle *h, const AcBuffers &b, hipStream_t st) = 0;  // the run struct of this sweep
  virtual hipError_t launch(int64_t base, int64_t count, hipStream_t st) = 0;
  // after the sweep (o.status on the host, the stream idle): what the engine adds
  virtual int32_t finish(SpiceyAcHandle *, SpiceyAcSweep &, hipStream_t) { return SPICEY_OK; }
  virtual void info(const SpiceyAcHandle *h, SpiceyInfo *info) const = 0;
};

struct SpiceyAcHandle {
  SpiceyOptions opt{};
  int device = 0, ncu = 256;
  AcDims dims;
  std::unique_ptr<AcEngine> eng;
  DevBuf<double> d_R, d_C, d_L;  // 1 / R, C, L [n_inst][n<kind>]
  int32_t n_nodes = 0, nR = 0, nC = 0, nL = 0;
  std::vector<double> R_host;    // R [n_inst][nR] in ohms, and on the device from the first noise pass on
  DevBuf<double> d_Rohm;
  bool have_Rohm = false;
  double last_noise_ms = 0.0, last_sens_ms = 0.0, last_mc_ms = 0.0, last_mc_draw_ms = 0.0;
  int64_t last_slots = 0;        // (instance, frequency) slots of the last sweep
  double last_ms = 0.0, last_measure_ms = 0.0;
  SpiceyAcInstStatus ist;        // per instance of the last sweep (spicey_ac_last_inst_status)
  std::string err;
  StreamTimers q;                // (last: events and stream go before the device buffers)
};

namespace {

struct AcSparse : AcEngine {
  HostProgram hp;
  HostResident hres;  // resident layout of the 16-bit records (batched sweeps)
  SpiceyProg dprog{};
  SpiceyResident dres{};
  DevBuf<uint8_t> d_blob, d_res;
  bool resident_ok = false, lds = true;
  int T = 256, Tres = 512;  // threads of a workgroup, and of the resident sweep's
  size_t lds_bytes = 0;
  int last_mode = 0;        // 1 = one workgroup per (instance, frequency), 2 = resident sweep
  int n_chunk = 1;          // resident sweep: workgroups per instance
  int64_t last_dense = 0;   // solves of the last run that went through the dense partial-pivoting fallback
  int32_t inj_p = 0, inj_n = 0;  // SpiceyAcRun::inj_* of the next sweep
  double inj_re = 0.0, inj_im = 0.0;
  SpiceyAcRun R{};

  int32_t plan(const SpiceyDesc *desc, const SpiceyOptions &, AcDims &dims, std::string &err) override {
    SpiceyDesc d = *desc;  // simulateAC.ts:38-59 stamps R, C, L and V only
    d.nS = 0;
    d.nD = 0;
    // (task records for every level: the real-valued cyclic reduction of a tridiagonal top is the transient kernel's)
    const int32_t rc = spicey_build_program(&d, hp, err, true, 0, false);
    const SpiceyProg &P = hp.hdr;
    dims = {desc->n_inst, P.nOut, P.nR + P.nC + P.nL + P.nV, P.nV};
    return rc;
  }

  int32_t upload(SpiceyAcHandle *h, const SpiceyDesc *) override {
    const SpiceyProg &P = hp.hdr;
    lds_bytes = (size_t)P.nW * sizeof(SpiceyCx);
    lds = !h->opt.force_global && lds_bytes + 64 <= SPICEY_LDS_MAX;
    const int n = P.n;
    // measured on rc_ladder(1000) x 201 frequencies: 256 / 512 / 1024 threads = 62 / 43 / 35 us per sweep (one wave of workgroups)
    T = h->opt.threads > 0 ? h->opt.threads : (n <= 48 ? 64 : n <= 160 ? 128 : n <= 400 ? 256 : 1024);
    if (T > 1024 || (T & 63) || T < 64) { h->err = "threads must be a multiple of 64 in [64, 1024]"; return SPICEY_ERR_BAD_DESC; }
    if (dev_upload(d_blob, hp.blob.size(), hp.blob.data()) != hipSuccess) { h->err = "upload of the program failed"; return SPICEY_ERR_HIP; }
    dprog = hp.bind(d_blob);
    // resident sweep for batches that outnumber the CUs: needs the LDS workspace, 16-bit records, and every entry in the
    // NSE register slots of a thread
    Tres = std::min(T, 512);
    if (lds && P.has16 && P.nLU <= SPICEY_AC_NSE * Tres && (int)hp.ph_cnt.size() <= 254) {
      spicey_build_resident(hp, Tres, SPICEY_AC_RMAX, hres, 0, false);  // (the complex executor knows generic records only)
      if (dev_upload(d_res, hres.blob.size(), hres.blob.data()) == hipSuccess) {
        dres = hres.bind(d_res);
        resident_ok = true;
      }
    }
    return SPICEY_OK;
  }

  bool structurally_singular() const override { return hp.structurally_singular; }

  // The right-hand-side row of a node is the pivot position of its ROW, HostProgram::rpos — not that of its column (out_x):
  // the source <-> node matching may permute the two differently.
  int32_t set_inject(const SpiceyAcInject *inj, std::string &) override {
    inj_p = inj_n = 0;
    inj_re = inj_im = 0.0;
    if (!inj) return SPICEY_OK;
    const int32_t nLU = hp.hdr.nLU;
    if (inj->node_p > 0) inj_p = 1 + nLU + hp.rpos[(size_t)inj->node_p - 1];
    if (inj->node_n > 0) inj_n = 1 + nLU + hp.rpos[(size_t)inj->node_n - 1];
    inj_re = inj->re; inj_im = inj->im;
    return SPICEY_OK;
  }

  int64_t chunk(const SpiceyAcHandle *h, int64_t slots, int64_t n_freq) override {
    // batches that outnumber the CUs (one workgroup per CU at this LDS size): persistent workgroups, ~2 per CU, each
    // keeping its share of the program in registers across its frequencies — one launch
    const int64_t ni = h->dims.n_inst;
    const bool resident = resident_ok && !(h->opt.debug & 16) && slots > (int64_t)2 * h->ncu;
    last_mode = resident ? 2 : 1;
    n_chunk = (int)std::min<int64_t>(n_freq, std::max<int64_t>(1, ((int64_t)2 * h->ncu + ni - 1) / ni));
    // global workspace: one slice per workgroup of a launch; sweeps whose slices would exceed 16 GiB run in chunks
    return lds ? slots : std::min<int64_t>(slots, std::max<int64_t>(1, (int64_t)(((size_t)16 << 30) / lds_bytes)));
  }
  size_t slot_ws_bytes() const override { return lds ? 0 : lds_bytes; }

  int32_t bind(SpiceyAcHandle *h, const AcBuffers &b, hipStream_t) override {
    R = SpiceyAcRun{};
    R.R_inv = b.R_inv; R.C_val = b.C_val; R.L_val = b.L_val;
    R.freqs = b.freqs; R.vph = b.vph; R.out_v = b.out_v; R.out_i = b.out_i; R.gW = (double *)b.gW; R.status = b.status;
    R.n_freq = b.n_freq; R.n_inst = h->dims.n_inst;
    R.inj_p = inj_p; R.inj_n = inj_n; R.inj_re = inj_re; R.inj_im = inj_im;  // (every chunk of the sweep launches this struct)
    return SPICEY_OK;
  }

  hipError_t launch(int64_t base, int64_t count, hipStream_t st) override {
    R.slot_base = base;
    if (last_mode == 2) return spicey_launch_ac_resident(dprog, dres, R, n_chunk, Tres, lds_bytes, st);
    return spicey_launch_ac(dprog, R, (int)count, T, lds ? lds_bytes : 0, st);
  }

  // Solves that tripped a pivot guard of the static order (a diagonal cancelling at a resonance) are repeated with
  // partial pivoting, dense, the way the reference solves every frequency; whatever fails there fails in the reference
  // too.  (diagnostics: SpiceyOptions.debug bit 7 = off; circuits beyond 4096 unknowns keep the error)
  int32_t finish(SpiceyAcHandle *h, SpiceyAcSweep &o, hipStream_t st) override {
    const SpiceyProg &P = hp.hdr;
    last_dense = 0;
    if (((h->opt.debug >> 7) & 1) || P.n > 4096) return SPICEY_OK;
    std::vector<int64_t> bad;
    for (size_t s = 0; s < o.status.size(); s++)
      if (o.status[s] != 0) bad.push_back((int64_t)s);
    if (bad.empty()) return SPICEY_OK;
    const size_t per = (size_t)P.n * ((size_t)P.n + 1) * sizeof(SpiceyCx);
    const size_t nb = std::min(bad.size(), std::max<size_t>(1, ((size_t)1 << 30) / per));
    DevBuf<int64_t> d_slots;
    DevBuf<SpiceyCx> d_A, d_Ws;
    DevBuf<SpiceyProg> d_P;
    DevBuf<SpiceyAcRun> d_run;
    if (d_slots.alloc(nb) != hipSuccess || d_A.alloc(nb * per / sizeof(SpiceyCx)) != hipSuccess || d_Ws.alloc(nb * (size_t)P.nW) != hipSuccess ||
        dev_upload(d_P, 1, &dprog) != hipSuccess || dev_upload(d_run, 1, &R) != hipSuccess) {
      h->err = "allocation of the dense fallback workspace failed";
      return SPICEY_ERR_HIP;
    }
    hipError_t e = hipSuccess;
    for (size_t b0 = 0; b0 < bad.size() && e == hipSuccess; b0 += nb) {
      const size_t cnt = std::min(nb, bad.size() - b0);
      e = hipMemcpyAsync(d_slots, bad.data() + b0, cnt * sizeof(int64_t), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = spicey_launch_ac_dense(d_P, d_run, P.n, d_slots, (int)cnt, d_Ws, d_A, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) { h->err = std::string("dense fallback: ") + hipGetErrorString(e); return SPICEY_ERR_HIP; }
    last_dense = (int64_t)bad.size();
    HIPCHK(h, hipMemcpyAsync(o.status.data(), R.status, o.status.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return SPICEY_OK;
  }

  void info(const SpiceyAcHandle *, SpiceyInfo *info) const override {
    info->n_var = hp.hdr.n;
    info->nnz_a = hp.nnzA;
    info->nnz_lu = hp.hdr.nLU;
    info->n_levels = hp.hdr.nLevels;
    info->threads = T;
    info->lds_bytes = lds ? (int32_t)lds_bytes : 0;
    info->interpreter = last_mode == 2 ? 2 : 1;  // 2 = the last run used the resident sweep
    info->resident_slots = resident_ok ? SPICEY_AC_RMAX : 0;
    info->resident_tasks = hres.resident_tasks;
    info->streamed_tasks = hres.streamed_tasks;
    info->program_bytes = (int64_t)hp.blob.size();
    info->tail_levels = (int32_t)last_dense;  // (AC handles: solves of the last run repeated with partial pivoting)
  }
};

// (no sparse program, no structural pre-check)
struct AcExact : AcEngine {
  AcExactPlan xplan;
  HostAcExactProg xp;
  DevBuf<uint8_t> d_blob;
  DevBuf<SpiceyAcExactProg> d_P;
  DevBuf<SpiceyAcExactRun> d_run;  // (the kernel reads its run struct from device memory)

  int32_t plan(const SpiceyDesc *desc, const SpiceyOptions &opt, AcDims &dims, std::string &err) override {
    const int32_t rc = spicey_ac_exact_plan(desc, opt, xplan, err);
    if (rc != SPICEY_OK) return rc;
    SpiceyDesc d = *desc;  // (R, C, L and V only)
    d.nS = 0;
    d.nD = 0;
    spicey_build_ac_exact(d, xplan.ws, xp);
    dims = {desc->n_inst, xp.hdr.nOut, xp.hdr.nCur, xp.hdr.nV};
    return SPICEY_OK;
  }

  int32_t upload(SpiceyAcHandle *h, const SpiceyDesc *) override {
    if (dev_upload(d_blob, xp.blob.size() * sizeof(uint32_t), reinterpret_cast<const uint8_t *>(xp.blob.data())) != hipSuccess) {
      h->err = "upload of the stamp lists failed";
      return SPICEY_ERR_HIP;
    }
    const SpiceyAcExactProg P = xp.bind(d_blob);
    if (dev_upload(d_P, 1, &P) != hipSuccess) { h->err = "upload of the program header failed"; return SPICEY_ERR_HIP; }
    return SPICEY_OK;
  }

  int64_t chunk(const SpiceyAcHandle *, int64_t slots, int64_t) override { return spicey_ac_exact_chunk(xplan, slots); }
  size_t slot_ws_bytes() const override { return xplan.lds ? 0 : (size_t)xp.hdr.ws_cx * sizeof(SpiceyCx); }

  int32_t bind(SpiceyAcHandle *h, const AcBuffers &b, hipStream_t st) override {
    SpiceyAcExactRun R{};
    R.R_inv = b.R_inv; R.C_val = b.C_val; R.L_val = b.L_val;
    R.freqs = b.freqs; R.vph = b.vph; R.out_v = b.out_v; R.out_i = b.out_i; R.gW = (SpiceyCx *)b.gW; R.status = b.status; R.skipped = nullptr;
    R.n_freq = b.n_freq; R.n_inst = h->dims.n_inst;
    HIPCHK(h, d_run.alloc(1));
    HIPCHK(h, hipMemcpyAsync(d_run, &R, sizeof(R), hipMemcpyHostToDevice, st));  // (pageable source: staged before the call returns)
    return SPICEY_OK;
  }

  hipError_t launch(int64_t base, int64_t count, hipStream_t st) override {
    return spicey_launch_ac_exact(d_P, d_run, base, (int)count, xplan.T, xplan.lds_bytes, st);
  }

  void info(const SpiceyAcHandle *h, SpiceyInfo *info) const override {
    info->n_var = xp.hdr.n;
    info->threads = xplan.T;
    info->lds_bytes = xplan.lds ? (int32_t)xplan.lds_bytes : 0;
    info->n_workgroups = (int32_t)h->last_slots;
    info->interpreter = 3;
    info->program_bytes = (int64_t)(xp.blob.size() * sizeof(uint32_t));
  }
};

thread_local std::string g_ac_err;  // message of the calling thread's last failed spicey_ac_create

}  // namespace

extern "C" const char *spicey_ac_last_error(SpiceyAcHandle *h) { return h ? h->err.c_str() : g_ac_err.c_str(); }

extern "C" void spicey_ac_destroy(SpiceyAcHandle *h) { delete h; }  // (events and stream, then every device buffer)

static int32_t ac_allocate(SpiceyAcHandle *h, const SpiceyDesc *desc) {
  int32_t rc = h->eng->plan(desc, h->opt, h->dims, h->err);
  if (rc == SPICEY_OK) rc = spicey_open_device(h->device, &h->ncu, h->err);
  if (rc == SPICEY_OK) rc = h->eng->upload(h, desc);
  if (rc != SPICEY_OK) return rc;
  const size_t ni = (size_t)h->dims.n_inst;
  h->n_nodes = desc->n_nodes;
  h->nR = desc->nR;
  h->nC = desc->nC;
  h->nL = desc->nL;
  h->R_host.assign(desc->R_val, desc->R_val + ni * (size_t)desc->nR);
  std::vector<double> rinv(ni * (size_t)desc->nR);
  for (size_t i = 0; i < rinv.size(); i++) rinv[i] = 1.0 / desc->R_val[i];  // (1 / R in simulateAC.ts:39-41, the same quotient)
  if (dev_upload(h->d_R, rinv.size(), rinv.data()) != hipSuccess || dev_upload(h->d_C, ni * desc->nC, desc->C_val) != hipSuccess ||
      dev_upload(h->d_L, ni * desc->nL, desc->L_val) != hipSuccess) {
    h->err = "upload of the element values failed";
    return SPICEY_ERR_HIP;
  }
  return h->q.create(h);
}

extern "C" int32_t spicey_ac_create(const SpiceyDesc *desc, const SpiceyOptions *opt, SpiceyAcHandle **out) {
  if (!out) { g_ac_err = "null out pointer"; return SPICEY_ERR_BAD_DESC; }
  *out = nullptr;
  if (!desc) { g_ac_err = "null descriptor"; return SPICEY_ERR_BAD_DESC; }
  SpiceyAcHandle *h = new SpiceyAcHandle();
  if (opt) h->opt = *opt;
  h->device = h->opt.device;
  if (h->opt.interpreter == 3) h->eng.reset(new AcExact());
  else h->eng.reset(new AcSparse());
  const int32_t rc = ac_allocate(h, desc);
  if (rc != SPICEY_OK) {
    g_ac_err = h->err;
    spicey_ac_destroy(h);
    return rc;
  }
  *out = h;
  return SPICEY_OK;
}

extern "C" int32_t spicey_ac_get_info(SpiceyAcHandle *h, SpiceyInfo *info) {
  if (!h || !info) return SPICEY_ERR_BAD_DESC;
  memset(info, 0, sizeof(*info));
  info->inst_per_wg = 1;
  info->wgs_per_inst = 1;
  info->n_cur = h->dims.n_cur;
  info->n_out = h->dims.n_out;
  h->eng->info(h, info);
  return SPICEY_OK;
}

extern "C" double spicey_ac_last_kernel_ms(SpiceyAcHandle *h) { return h ? h->last_ms : 0.0; }

// The refusals of an injection that need no engine (text in h->err).
static bool ac_judge_inject(SpiceyAcHandle *h, const SpiceyAcInject *inj) {
  const char *what = nullptr;
  if (inj->struct_bytes != (int64_t)sizeof(SpiceyAcInject)) what = "struct_bytes is not sizeof(SpiceyAcInject)";
  else if (inj->node_p < 0 || inj->node_p > h->n_nodes || inj->node_n < 0 || inj->node_n > h->n_nodes) what = "node outside [0, n_nodes]";
  else if (inj->node_p == inj->node_n) what = "node_p == node_n: nothing is injected";
  else if (!std::isfinite(inj->re) || !std::isfinite(inj->im)) what = "the amplitude must be finite";
  if (what) h->err = std::string("inject: ") + what;
  return !what;
}

// What spicey_ac_run and spicey_ac_run_measure share: the argument checks, then ONE sweep into `o` — staged, timed,
// launched through the engine, o.status on the host, the stream idle.  The caller copies out or reduces.
// *done: the call is answered without a sweep (nothing to do, or structurally singular).
// inj: the current injection of this sweep (null: none; with one, a null vph means every phasor zero).
// vals: three device arrays {1 / R, C, L} [n_inst][n<kind>] the sweep reads instead of the handle's (null: the handle's).
static int32_t ac_sweep(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, bool have_out, bool want_i, SpiceyAcSweep &o, bool *done,
                        const SpiceyAcInject *inj = nullptr, DevBuf<double> *keep_freqs = nullptr, const double *const *vals = nullptr) {
  *done = true;
  h->ist.forget();
  const AcDims &d = h->dims;
  if (n_freq < 0 || (n_freq > 0 && (!freqs || !have_out)) || (d.n_v > 0 && !vph && !inj)) { h->err = "bad run arguments"; return SPICEY_ERR_BAD_DESC; }
  if (inj && !ac_judge_inject(h, inj)) return SPICEY_ERR_BAD_DESC;
  if (const int32_t rc = h->eng->set_inject(inj, h->err); rc != SPICEY_OK) return rc;
  if (n_freq == 0) {
    h->ist.fill(d.n_inst, 0, -1);
    return SPICEY_OK;
  }
  if (h->eng->structurally_singular()) {
    h->err = "Singular matrix (complex): structurally singular";
    h->ist.fill(d.n_inst, SPICEY_ERR_SINGULAR, 0);
    return SPICEY_ERR_SINGULAR;
  }
  *done = false;
  const int64_t slots = (int64_t)d.n_inst * n_freq;
  if (slots > 0x7fffffffll) { h->err = "n_inst * n_freq exceeds the grid limit"; return SPICEY_ERR_BAD_DESC; }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->q.stream;
  o.status.assign((size_t)slots, 0);
  const int64_t chunk = h->eng->chunk(h, slots, n_freq);
  const size_t ws_bytes = (size_t)chunk * h->eng->slot_ws_bytes();
  DevBuf<double> d_f_own, d_ph;
  DevBuf<double> &d_f = keep_freqs ? *keep_freqs : d_f_own;  // (a caller that reduces behind the sweep keeps the frequencies)
  DevBuf<uint8_t> d_gW;
  DevBuf<int32_t> d_status;
  HIPCHK(h, d_f.alloc((size_t)n_freq));
  HIPCHK(h, d_ph.alloc(std::max<size_t>(1, (size_t)d.n_inst * d.n_v * 2)));
  HIPCHK(h, o.d_ov.alloc(std::max<size_t>(1, (size_t)slots * d.n_out * 2)));
  if (want_i) HIPCHK(h, o.d_oi.alloc(std::max<size_t>(1, (size_t)slots * d.n_cur * 2)));
  HIPCHK(h, d_status.alloc((size_t)slots));
  if (ws_bytes && d_gW.alloc(ws_bytes) != hipSuccess) {
    h->err = "allocation of the global slab failed (" + std::to_string(ws_bytes) + " bytes)";
    return SPICEY_ERR_HIP;
  }
  HIPCHK(h, hipMemcpyAsync(d_f, freqs, (size_t)n_freq * sizeof(double), hipMemcpyHostToDevice, st));
  if (d.n_v > 0 && vph) HIPCHK(h, hipMemcpyAsync(d_ph, vph, (size_t)d.n_inst * d.n_v * 2 * sizeof(double), hipMemcpyHostToDevice, st));
  else if (d.n_v > 0) HIPCHK(h, hipMemsetAsync(d_ph, 0, (size_t)d.n_inst * d.n_v * 2 * sizeof(double), st));
  const AcBuffers b{vals ? vals[0] : h->d_R, vals ? vals[1] : h->d_C, vals ? vals[2] : h->d_L, d_f, d_ph, o.d_ov, o.d_oi, d_gW, d_status, n_freq};
  if (const int32_t rc = h->eng->bind(h, b, st); rc != SPICEY_OK) return rc;
  HIPCHK(h, hipEventRecord(h->q.ev0, st));
  for (int64_t base = 0; base < slots; base += chunk) HIPCHK(h, h->eng->launch(base, std::min(chunk, slots - base), st));
  HIPCHK(h, hipEventRecord(h->q.ev1, st));
  HIPCHK(h, hipMemcpyAsync(o.status.data(), d_status, (size_t)slots * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  StreamTimers::elapsed(h->q.ev0, h->q.ev1, &h->last_ms);
  h->last_slots = slots;
  return h->eng->finish(h, o, st);
}

static int32_t ac_run(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, const SpiceyAcInject *inj, double *out_v, double *out_i) {
  SpiceyAcSweep o;
  bool done = false;
  const int32_t rc = ac_sweep(h, n_freq, freqs, vph, out_v != nullptr, out_i != nullptr, o, &done, inj);
  if (rc != SPICEY_OK || done) return rc;
  const AcDims &d = h->dims;
  const size_t slots = (size_t)d.n_inst * (size_t)n_freq;
  hipStream_t st = h->q.stream;
  // (also when a slot failed: the rows of the instances that are fine are complete, spicey_ac_last_inst_status names them)
  HIPCHK(h, hipMemcpyAsync(out_v, o.d_ov, slots * (size_t)d.n_out * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (out_i) HIPCHK(h, hipMemcpyAsync(out_i, o.d_oi, slots * (size_t)d.n_cur * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return h->ist.from_slots(o.status, d.n_inst, n_freq, h->err);
}

extern "C" int32_t spicey_ac_run(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, double *out_v, double *out_i) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  return ac_run(h, n_freq, freqs, vph, nullptr, out_v, out_i);
}

extern "C" int32_t spicey_ac_run_inject(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, const SpiceyAcInject *inj, double *out_v,
                                        double *out_i) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  if (!inj) { h->ist.forget(); h->err = "inject: null injection"; return SPICEY_ERR_BAD_DESC; }
  return ac_run(h, n_freq, freqs, vph, inj, out_v, out_i);
}

extern "C" int32_t spicey_ac_last_inst_status(SpiceyAcHandle *h, int32_t *status, int64_t *first_freq) {
  if (!h || !status || !h->ist.valid) return -1;
  int32_t bad = 0;
  for (size_t i = 0; i < h->ist.code.size(); i++) {
    status[i] = h->ist.code[i];
    if (first_freq) first_freq[i] = h->ist.first[i];
    bad += h->ist.code[i] != 0;
  }
  return bad;
}

extern "C" int32_t spicey_ac_run_measure(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, const SpiceyAcMeasReq *reqs,
                                         int32_t n_req, double *meas) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  h->ist.forget();
  h->last_measure_ms = 0.0;
  const AcDims &d = h->dims;
  // (a refused request list runs nothing; the buffers are this call's own)
  const int64_t work_bytes = spicey_acm_workspace_bytes(d.n_inst, n_freq, n_req);
  std::vector<SpiceyAcMeasDevReq> table;
  if (const int32_t rc = spicey_judge_measure("ac measure", spicey_acm_plan, spicey_acm_workspace_bytes, d.n_inst, n_freq, true, d.n_out, true, d.n_cur, reqs,
                                              n_req, true, work_bytes, table, h->err); rc != SPICEY_OK)
    return rc;
  bool need_i = false;
  for (const SpiceyAcMeasDevReq &q : table) need_i = need_i || q.num_signal == 1 || q.den_signal == 1;
  SpiceyAcSweep o;
  bool done = false;
  const int32_t rc = ac_sweep(h, n_freq, freqs, vph, meas != nullptr, need_i, o, &done);
  if (rc != SPICEY_OK || done) return rc;
  hipStream_t st = h->q.stream;
  HIPCHK(h, h->q.want_pass_events(PASS_MEASURE));
  const hipEvent_t *ev = h->q.pass_ev[PASS_MEASURE];
  DevBuf<double> d_meas;
  DevBuf<uint8_t> d_work;
  const size_t n_meas = (size_t)d.n_inst * (size_t)n_req * 8;
  HIPCHK(h, d_meas.alloc(n_meas));
  HIPCHK(h, d_work.alloc((size_t)work_bytes));
  HIPCHK(h, hipEventRecord(ev[0], st));
  HIPCHK(h, spicey_launch_ac_measure(h->device, d.n_inst, n_freq, o.d_ov, d.n_out, o.d_oi, d.n_cur, table.data(), n_req, d_meas, d_work, st));
  HIPCHK(h, hipEventRecord(ev[1], st));
  HIPCHK(h, hipMemcpyAsync(meas, d_meas, n_meas * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  StreamTimers::elapsed(ev[0], ev[1], &h->last_measure_ms);
  return h->ist.from_slots(o.status, d.n_inst, n_freq, h->err);
}

extern "C" double spicey_ac_last_measure_ms(SpiceyAcHandle *h) { return h ? h->last_measure_ms : 0.0; }

// The injected sweep of spicey_ac_run_inject with its buffers left on the device and the noise pass of noise.hip behind it.
extern "C" int32_t spicey_ac_run_noise(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, const SpiceyAcInject *inj,
                                       const SpiceyAcNoiseReq *req, double *spec, double *contrib, double *total, double *gain) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  h->ist.forget();
  h->last_noise_ms = 0.0;
  const AcDims &d = h->dims;
  if (!inj) { h->err = "inject: null injection"; return SPICEY_ERR_BAD_DESC; }
  // (a refused request runs nothing: judged on placeholder buffers first, the sweep's own are bound below)
  const int64_t work_bytes = spicey_noise_workspace_bytes(d.n_inst, n_freq, h->nR);
  const double *some = h->d_R;  // (any non-null pointer: the judge looks at null-ness only)
  SpiceyNoiseArgs A;
  if (!spicey_noise_judge(d.n_inst, n_freq, some, d.n_out, some, d.n_cur, some, h->nR, some, req, spec && contrib && total, work_bytes, A, h->err))
    return SPICEY_ERR_BAD_DESC;
  SpiceyAcSweep o;
  DevBuf<double> d_f;
  bool done = false;
  const int32_t rc = ac_sweep(h, n_freq, freqs, vph, true, true, o, &done, inj, &d_f);
  if (rc != SPICEY_OK || done) return rc;
  hipStream_t st = h->q.stream;
  if (!h->have_Rohm) {
    if (dev_upload(h->d_Rohm, h->R_host.size(), h->R_host.data()) != hipSuccess) { h->err = "upload of the resistances failed"; return SPICEY_ERR_HIP; }
    h->have_Rohm = true;
  }
  HIPCHK(h, h->q.want_pass_events(PASS_MEASURE));
  const hipEvent_t *ev = h->q.pass_ev[PASS_MEASURE];
  const size_t n_spec = (size_t)d.n_inst * (size_t)n_freq * SPICEY_NOISE_SPEC, n_con = (size_t)d.n_inst * (size_t)h->nR, n_tot = (size_t)d.n_inst * 2;
  DevBuf<double> d_spec, d_con, d_tot;
  DevBuf<uint8_t> d_work;
  HIPCHK(h, d_spec.alloc(n_spec));
  HIPCHK(h, d_con.alloc(n_con));
  HIPCHK(h, d_tot.alloc(n_tot));
  HIPCHK(h, d_work.alloc((size_t)work_bytes));
  A.d_i = o.d_oi; A.d_v = o.d_ov; A.R = h->d_Rohm; A.freqs = d_f;
  HIPCHK(h, hipEventRecord(ev[0], st));
  HIPCHK(h, spicey_launch_noise(h->device, A, d_spec, d_con, d_tot, d_work, st));
  HIPCHK(h, hipEventRecord(ev[1], st));
  HIPCHK(h, hipMemcpyAsync(spec, d_spec, n_spec * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(contrib, d_con, n_con * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(total, d_tot, n_tot * sizeof(double), hipMemcpyDeviceToHost, st));
  if (gain && A.in_col >= 0)  // (the one column of out_i the host wants whole: a strided copy of 16 bytes per slot)
    HIPCHK(h, hipMemcpy2DAsync(gain, 2 * sizeof(double), (const double *)o.d_oi + (size_t)A.in_col * 2, (size_t)d.n_cur * 2 * sizeof(double), 2 * sizeof(double),
                               (size_t)d.n_inst * (size_t)n_freq, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  StreamTimers::elapsed(ev[0], ev[1], &h->last_noise_ms);
  return h->ist.from_slots(o.status, d.n_inst, n_freq, h->err);
}

extern "C" double spicey_ac_last_noise_ms(SpiceyAcHandle *h) { return h ? h->last_noise_ms : 0.0; }

// Sweep D (vph, no injection) and sweep X (inj, every phasor zero) of ac_sweep, both left on the device, and the sensitivity
// pass of sens.hip behind them.
extern "C" int32_t spicey_ac_run_sens(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, const SpiceyAcInject *inj,
                                      const SpiceyAcSensReq *req, const double *tol, double *spec, double *peak, double *full) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  h->ist.forget();
  h->last_sens_ms = 0.0;
  const AcDims &d = h->dims;
  const int32_t nE = h->nR + h->nC + h->nL;
  if (!inj) { h->err = "inject: null injection"; return SPICEY_ERR_BAD_DESC; }
  // (a refused request, tolerance list or injection runs nothing: judged on placeholder buffers first, the sweeps' own are
  // bound below; the engine is asked for the injection before sweep D, which then clears it)
  const int64_t work_bytes = spicey_sens_workspace_bytes(d.n_inst, n_freq, nE);
  const double *some = h->d_R;  // (any non-null pointer: the judge looks at null-ness only)
  SpiceySensArgs A;
  if (!spicey_sens_judge(d.n_inst, n_freq, some, d.n_out, some, some, d.n_cur, some, some, some, tol, some, req, spec && peak, work_bytes, A, h->err))
    return SPICEY_ERR_BAD_DESC;
  if (req->nR != h->nR || req->nC != h->nC || req->nL != h->nL) { h->err = "sens: nR, nC, nL are not the handle's"; return SPICEY_ERR_BAD_DESC; }
  if (!ac_judge_inject(h, inj)) return SPICEY_ERR_BAD_DESC;
  if (const int32_t rc = h->eng->set_inject(inj, h->err); rc != SPICEY_OK) return rc;
  SpiceyAcSweep dir, adj;
  DevBuf<double> d_f;
  bool done = false;
  int32_t rc = ac_sweep(h, n_freq, freqs, vph, true, true, dir, &done, nullptr, &d_f);
  if (rc != SPICEY_OK || done) return rc;
  const double dir_ms = h->last_ms;
  rc = ac_sweep(h, n_freq, freqs, nullptr, true, true, adj, &done, inj);
  if (rc != SPICEY_OK || done) return rc;
  h->last_ms += dir_ms;
  for (size_t s = 0; s < dir.status.size(); s++)
    if (dir.status[s] == 0) dir.status[s] = adj.status[s];
  hipStream_t st = h->q.stream;
  if (!h->have_Rohm) {
    if (dev_upload(h->d_Rohm, h->R_host.size(), h->R_host.data()) != hipSuccess) { h->err = "upload of the resistances failed"; return SPICEY_ERR_HIP; }
    h->have_Rohm = true;
  }
  HIPCHK(h, h->q.want_pass_events(PASS_MEASURE));
  const hipEvent_t *ev = h->q.pass_ev[PASS_MEASURE];
  const size_t slots = (size_t)d.n_inst * (size_t)n_freq;
  const size_t n_spec = slots * SPICEY_SENS_SPEC, n_peak = (size_t)d.n_inst * (size_t)nE * SPICEY_SENS_PEAK, n_full = slots * (size_t)nE * 2;
  DevBuf<double> d_spec, d_peak, d_full;
  DevBuf<uint8_t> d_work;
  HIPCHK(h, d_spec.alloc(n_spec));
  HIPCHK(h, d_peak.alloc(n_peak));
  if (full) HIPCHK(h, d_full.alloc(n_full));
  HIPCHK(h, d_work.alloc((size_t)work_bytes));
  // (h->d_C and h->d_L hold farads and henries as the descriptor gave them; 1 / R is the sweep's, ohms are uploaded once)
  A.d_v = dir.d_ov; A.d_id = dir.d_oi; A.d_ix = adj.d_oi; A.R = h->d_Rohm; A.C = h->d_C; A.L = h->d_L; A.freqs = d_f;
  HIPCHK(h, hipEventRecord(ev[0], st));
  HIPCHK(h, spicey_launch_sens(h->device, A, tol, d_spec, d_peak, full ? (double *)d_full : nullptr, d_work, st));
  HIPCHK(h, hipEventRecord(ev[1], st));
  HIPCHK(h, hipMemcpyAsync(spec, d_spec, n_spec * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(peak, d_peak, n_peak * sizeof(double), hipMemcpyDeviceToHost, st));
  if (full) HIPCHK(h, hipMemcpyAsync(full, d_full, n_full * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  StreamTimers::elapsed(ev[0], ev[1], &h->last_sens_ms);
  return h->ist.from_slots(dir.status, d.n_inst, n_freq, h->err);
}

extern "C" double spicey_ac_last_sens_ms(SpiceyAcHandle *h) { return h ? h->last_sens_ms : 0.0; }

// The draw of mc.hip into scratch value arrays, ONE sweep of ac_sweep bound to them and left on the device, and the reduction
// across the instances behind it.
extern "C" int32_t spicey_ac_run_mc(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, const SpiceyAcMcReq *req, const double *tol,
                                    const double *icdf, const double *lo, const double *hi, const double *probs, int32_t n_prob, double *freq_stats,
                                    int64_t *sample, double *nominal) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  h->ist.forget();
  h->last_mc_ms = h->last_mc_draw_ms = 0.0;
  const AcDims &d = h->dims;
  const int32_t nE = h->nR + h->nC + h->nL;
  // (a refused request, tolerance list, table or probability runs nothing: judged on placeholder buffers first, the scratch
  // arrays and the sweep's own are bound below; the ranks follow from n_valid, which only the sweep tells)
  if (n_prob < 0 || n_prob > (1 << 20) || (n_prob && !probs)) { h->err = "mc: bad probabilities (n_prob >= 0, a list)"; return SPICEY_ERR_BAD_DESC; }
  for (int32_t j = 0; j < n_prob; j++)
    if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) { h->err = "mc: a probability outside [0, 1]"; return SPICEY_ERR_BAD_DESC; }
  const int32_t n_rank = 2 * n_prob;
  const int64_t draw_bytes = req ? spicey_mc_draw_bytes(nE, req->log2K) : 0, red_bytes = spicey_mc_reduce_bytes(d.n_inst, n_freq, n_rank);
  double *some = h->d_R;  // (any non-null pointer: the judges look at null-ness only)
  SpiceyMcDrawArgs D;
  SpiceyMcReduceArgs A;
  if (!spicey_mc_draw_judge(d.n_inst, h->nR, h->nC, h->nL, some, some, some, tol, icdf, req, some, some, some, true, draw_bytes, D, h->err) ||
      !spicey_mc_reduce_judge(d.n_inst, n_freq, some, d.n_out, nullptr, nullptr, 0, req, freq_stats && sample, red_bytes, A, h->err))
    return SPICEY_ERR_BAD_DESC;
  if (!freqs || (d.n_v > 0 && !vph)) { h->err = "bad run arguments"; return SPICEY_ERR_BAD_DESC; }
  if (h->eng->structurally_singular()) {
    h->err = "Singular matrix (complex): structurally singular";
    h->ist.fill(d.n_inst, SPICEY_ERR_SINGULAR, 0);
    return SPICEY_ERR_SINGULAR;
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->q.stream;
  if (!h->have_Rohm) {
    if (dev_upload(h->d_Rohm, h->R_host.size(), h->R_host.data()) != hipSuccess) { h->err = "upload of the resistances failed"; return SPICEY_ERR_HIP; }
    h->have_Rohm = true;
  }
  const size_t ni = (size_t)d.n_inst;
  DevBuf<double> d_sR, d_sC, d_sL;
  DevBuf<uint8_t> d_work;
  HIPCHK(h, d_sR.alloc(std::max<size_t>(1, ni * (size_t)h->nR)));
  HIPCHK(h, d_sC.alloc(std::max<size_t>(1, ni * (size_t)h->nC)));
  HIPCHK(h, d_sL.alloc(std::max<size_t>(1, ni * (size_t)h->nL)));
  HIPCHK(h, d_work.alloc((size_t)std::max(draw_bytes, red_bytes)));
  D.R = h->d_Rohm; D.C = h->d_C; D.L = h->d_L; D.oR = d_sR; D.oC = d_sC; D.oL = d_sL;
  HIPCHK(h, hipEventRecord(h->q.ev0, st));
  HIPCHK(h, spicey_launch_mc_draw(h->device, D, tol, icdf, d_work, st));
  HIPCHK(h, hipEventRecord(h->q.ev1, st));
  HIPCHK(h, hipStreamSynchronize(st));  // (ac_sweep records the same pair again)
  StreamTimers::elapsed(h->q.ev0, h->q.ev1, &h->last_mc_draw_ms);
  const double *vals[3] = {d_sR, d_sC, d_sL};
  SpiceyAcSweep o;
  bool done = false;
  const int32_t rc = ac_sweep(h, n_freq, freqs, vph, true, false, o, &done, nullptr, nullptr, vals);
  if (rc != SPICEY_OK || done) return rc;
  std::vector<uint8_t> valid(ni, 1);
  int64_t n_valid = 0;
  for (size_t s = 0; s < ni; s++) {
    for (int64_t k = 0; k < n_freq && valid[s]; k++) valid[s] = o.status[s * (size_t)n_freq + (size_t)k] == 0;
    n_valid += valid[s];
  }
  const int32_t sweep_rc = h->ist.from_slots(o.status, d.n_inst, n_freq, h->err);
  if (n_valid == 0) {
    if (sweep_rc == SPICEY_OK) { h->err = "mc: no valid sample"; return SPICEY_ERR_SINGULAR; }
    h->err += " (mc: no valid sample, nothing reduced)";
    return sweep_rc;
  }
  std::vector<int64_t> ranks((size_t)n_rank);
  for (int32_t j = 0; j < n_prob; j++) {
    const int64_t r = (int64_t)std::floor(probs[j] * (double)(n_valid - 1));
    ranks[2 * (size_t)j] = r;
    ranks[2 * (size_t)j + 1] = std::min<int64_t>(r + 1, n_valid - 1);
  }
  std::string why;
  if (!spicey_mc_reduce_judge(d.n_inst, n_freq, o.d_ov, d.n_out, valid.data(), ranks.data(), n_rank, req, true, red_bytes, A, why)) {
    h->err = why;
    return SPICEY_ERR_BAD_DESC;
  }
  HIPCHK(h, h->q.want_pass_events(PASS_MEASURE));
  const hipEvent_t *ev = h->q.pass_ev[PASS_MEASURE];
  const size_t n_fs = (size_t)n_freq * (size_t)(SPICEY_MC_FREQ_HEAD + n_rank);
  DevBuf<double> d_fs;
  DevBuf<int64_t> d_sample;
  HIPCHK(h, d_fs.alloc(n_fs));
  HIPCHK(h, d_sample.alloc(ni * 2));
  HIPCHK(h, hipEventRecord(ev[0], st));
  HIPCHK(h, spicey_launch_mc_reduce(h->device, A, n_valid == (int64_t)ni ? nullptr : valid.data(), lo, hi, ranks.data(), d_sample, d_fs, d_work, st));
  HIPCHK(h, hipEventRecord(ev[1], st));
  HIPCHK(h, hipMemcpyAsync(freq_stats, d_fs, n_fs * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(sample, d_sample, ni * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  std::vector<double> col_p, col_n;
  const bool want_nom = nominal && req->keep_first;
  if (want_nom) {  // (sample 0's columns of the pair: a strided copy of 16 bytes per frequency each, as the noise pass's gain)
    for (int side = 0; side < 2; side++) {
      const int32_t col = side ? req->out_n : req->out_p;
      std::vector<double> &dst = side ? col_n : col_p;
      if (col < 0) continue;
      dst.resize((size_t)n_freq * 2);
      HIPCHK(h, hipMemcpy2DAsync(dst.data(), 2 * sizeof(double), (const double *)o.d_ov + (size_t)col * 2, (size_t)d.n_out * 2 * sizeof(double), 2 * sizeof(double),
                                 (size_t)n_freq, hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHK(h, hipStreamSynchronize(st));
  StreamTimers::elapsed(ev[0], ev[1], &h->last_mc_ms);
  if (want_nom)
    for (size_t i = 0; i < (size_t)n_freq * 2; i++) {  // (H as spicey_mc_q forms it: one subtraction per part)
      double x = 0.0;
      if (!col_p.empty()) x = col_p[i];
      if (!col_n.empty()) x = x - col_n[i];
      nominal[i] = x;
    }
  return sweep_rc;
}

extern "C" double spicey_ac_last_mc_ms(SpiceyAcHandle *h) { return h ? h->last_mc_ms : 0.0; }
extern "C" double spicey_ac_last_mc_draw_ms(SpiceyAcHandle *h) { return h ? h->last_mc_draw_ms : 0.0; }
