/*
 * spicey_hip.h — C-ABI of the MI355X-native transient MNA solver that replaces the body of
 * spicey's simulateTRAN().
 *
 * Boundary: the reference has no plugin/FFI layer; the boundary is cut INSIDE
 *   simulateTRAN(ckt)            /root/reference/lib/analysis/simulateTRAN.ts:130-252
 * The host (TypeScript via bun:ffi, or the Python mirror in spicey_amd/) keeps parsing,
 * computeEffectiveTimeStep (:14-19), waveform pre-evaluation (:67, closures cannot cross FFI),
 * flattening ParsedCircuit (parseNetlist.ts:85-105) into the POD arrays below, result re-keying
 * and state write-back.  The native side runs the whole `for step … for iter …` nest
 * (:146-238): stamping (:25-102, lib/stamping/stamp{Admittance,Current,VoltageSource}Real.ts), the linear solve that replaces
 * solveReal (lib/math/solveReal.ts:3-73), the switch iteration (:108-128,:151-162), result
 * recording (:164-219) and the state update (:221-237).
 *
 * Everything is plain C: POD structs, raw pointers and sizes, int32 status codes; no torch or
 * C++ types.  A handle owns its device memory and is not thread-safe; distinct handles may be
 * used from distinct threads.  The library never calls abort()/exit().
 *
 * Launch admission (one rule per DEVICE, enforced inside the library).  A large instance may run on several cooperating
 * workgroups that wait for one another inside the kernel ("group mode", SpiceyInfo.wgs_per_inst > 1): such a launch only
 * makes progress while ALL its workgroups are resident, one per CU.  Therefore (a) a group is sized from the runtime's
 * occupancy answer for the very kernel and LDS size it launches, at most one workgroup per CU; (b) a group-mode launch
 * starts only after every transient launch this library has enqueued on that device before it has finished, and no
 * later transient launch of the library starts before the group-mode launch has finished — whatever handles, streams
 * and host threads they come from (stream-ordered event waits, nothing blocks on the host; launches that are not
 * group-mode stay concurrent with each other); (c) every cross-workgroup wait is bounded in time
 * (SpiceyOptions.group_timeout_ms): a launch whose wait runs out aborts as a whole with SPICEY_ERR_HIP and the waiter's
 * position in spicey_last_error() — it never hangs.  What the library cannot see are kernels of OTHER code on the same
 * device: keep long-running foreign kernels off the device while a group-mode run is in flight, or raise the timeout.
 *
 * Conventions
 *   node ids      0 = ground, 1..n_nodes = non-ground nodes (NodeIndex.ts:28-31: row = id-1)
 *   unknowns      x[0..n_nodes-1] node voltages, x[n_nodes+k] = branch current of source k
 *                 (parseNetlist.ts:455-460)
 *   instances     n_inst circuits sharing ONE topology (node ids, element order) with
 *                 per-instance element values and state: every `double` array below is
 *                 instance-major, [n_inst][n<kind>]
 *   outputs       step-major: out_v[inst][step][n_out], out_i[inst][step][n_cur] with
 *                 n_cur = nR+nC+nL+nV+nS+nD in the reference's recording order R,C,L,V,S,D
 *                 (simulateTRAN.ts:173-219)
 */
#ifndef SPICEY_HIP_H
#define SPICEY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPICEY_ABI_VERSION 2 /* 2: SpiceyOptions grew (group_retry, group_timeout_ms, diagnostics) */

/* status codes (SURVEY.md §8(b) "Errors") */
#define SPICEY_OK 0
#define SPICEY_ERR_SINGULAR 1 /* host maps to Error("Singular matrix (real)"), solveReal.ts:28 */
#define SPICEY_ERR_BAD_DESC 2
#define SPICEY_ERR_HIP 3
#define SPICEY_ERR_NO_DEVICE 4 /* the product path has no CPU fallback: no GPU -> this error */
#define SPICEY_ERR_COMPLEX_DIV 5 /* AC only: host maps to Error("Complex divide by ~0"), math/Complex.ts:40-42 */

/* Flat circuit descriptor: the ParsedCircuit of parseNetlist.ts:85-105 as SoA arrays.
 * All pointers are HOST pointers, read during spicey_create only. */
typedef struct SpiceyDesc {
  int32_t abi_version; /* SPICEY_ABI_VERSION */
  int32_t n_nodes;     /* ckt.nodes.count() - 1 */
  int32_t n_inst;      /* >= 1 */
  int32_t nR, nC, nL, nV, nS, nD;

  /* resistors  (ParsedResistor, parseNetlist.ts:12) */
  const int32_t *R_n1, *R_n2; /* [nR] */
  const double *R_val;        /* [n_inst][nR] ohms */
  /* capacitors (ParsedCapacitor :13-19); C_vprev = state entering the run (vPrev) */
  const int32_t *C_n1, *C_n2;
  const double *C_val, *C_vprev; /* [n_inst][nC] */
  /* inductors (ParsedInductor :20-26); L_iprev = iPrev */
  const int32_t *L_n1, *L_n2;
  const double *L_val, *L_iprev; /* [n_inst][nL] */
  /* independent voltage sources (ParsedVoltageSource :34-43); values come per step in src_table */
  const int32_t *V_n1, *V_n2; /* [nV] */
  /* voltage-controlled switches (ParsedSwitch :63-72 + ParsedVSwitchModel :45-51) */
  const int32_t *S_n1, *S_n2, *S_cp, *S_cn;          /* [nS] */
  const double *S_ron, *S_roff, *S_von, *S_voff;     /* [n_inst][nS] */
  const int32_t *S_ison;                             /* [n_inst][nS] 0/1, state entering the run */
  /* diodes (ParsedDiode :53-61 + ParsedDiodeModel :28-32); D_vdprev = vdPrev */
  const int32_t *D_np, *D_nm;                        /* [nD] */
  const double *D_is, *D_n, *D_vdprev;               /* [n_inst][nD] */

  /* recorded node voltages: out_nodes[n_out] are node ids (1-based); n_out = 0 / NULL -> all
   * nodes in id order (simulateTRAN.ts:164-171; .PRINT filtering :240-249 done before writing) */
  int32_t n_out;
  const int32_t *out_nodes;
} SpiceyDesc;

typedef struct SpiceyOptions {
  int32_t device;        /* HIP device ordinal */
  int32_t threads;       /* workgroup size, 0 = auto (a circuit that takes the hybrid workspace, SpiceyInfo.hybrid_entries > 0, runs on
                            1024 threads; 512 selects the 512-thread build of that kernel: the same results bit for bit) */
  int32_t inst_per_wg;   /* instances interleaved in one workgroup's LDS, 0 = auto */
  int32_t want_currents; /* 1: record element currents (out_i) */
  int32_t force_global;  /* 1: keep the LU workspace in HBM/L2 even if it fits LDS (testing) */
  int32_t profile;       /* 1: accumulate per-phase shader-clock cycles (spicey_debug_phase_cycles) */
  int32_t interpreter;   /* 0 auto; 1 = v1 (32-bit sliced task lists from L2); 2 = v2 (register-resident 16-bit records);
                            3 = reference order: the reference's own algorithm (fresh dense stamp in element order, solveReal
                            with partial pivoting and its |f| < EPS row-update skip, back substitution in its order), one
                            workgroup per instance — every result bit, the end state and SPICEY_ERR_SINGULAR exactly where
                            the reference has them.  A | b in LDS up to n ~ 138 unknowns, else an n x (n + 1) slab per
                            instance in global memory (force_global = 1: always).  threads: 0 = 64 for n <= 64, else 256;
                            64..1024 honoured (same bits).  inst_per_wg > 1, geometry != 0, front_cut > 0, wgs_per_inst > 1
                            and profile are refused (SPICEY_ERR_BAD_DESC).  diagnostics bit 0 then counts the nonzero
                            multipliers the skip dropped (spicey_last_skip_risk), bit 1 records lin_err as for the others.
                            Never chosen automatically. */
  int32_t geometry;      /* v2 only. 0 auto; 1 = latency: one workgroup per CU, whole program in registers;
                            2 = throughput: two 512-thread workgroups per CU (<= 128 VGPRs, wide levels streamed) */
  int32_t debug;         /* diagnostics: bit 0 = no tail merge; bit 1 = refactor every step even for linear circuits;
                            bit 2 = plain CSR numbering of the L+U entries (no LDS-bank-aware slot-major numbering);
                            bit 3 = dense fronts above 64 rows take the staged (global-memory) path even if they fit LDS;
                            bit 4 = AC: never use the resident sweep (one workgroup per (instance, frequency) always);
                            bit 5 = no tridiagonal top (interpreter 2 keeps its task lists for the top levels of a chain);
                            bit 6 = no row records (streamed factor levels of a chain keep one task per target entry);
                            bit 7 = AC: no dense partial-pivoting fallback (a solve whose static pivot order hits a cancelled
                                    diagonal reports "Complex divide by ~0" / "Singular matrix (complex)" instead);
                            bits 8.. = extra empty phases per solve */
  int32_t wgs_per_inst;  /* global-workspace path: workgroups (CUs) cooperating on one instance; 0 auto, 1 = none */
  int32_t front_cut;     /* dense fronts (large instances): pivots of elimination-tree level >= front_cut are factored as
                            dense supernodal fronts (LDS-staged panels, MFMA trailing updates) instead of one
                            barrier-separated level per pivot.  0 = auto (large nonlinear circuits), -1 = never, > 0 = this level */
  int32_t group_retry;   /* group mode: 1 = a launch that ends in the bounded-wait abort is repeated ONCE from the state it
                            started with (spicey_sync); 0 (default) = the abort is reported as SPICEY_ERR_HIP */
  int32_t group_timeout_ms; /* group mode: longest single cross-workgroup wait before the launch aborts; 0 = 5000 */
  int32_t diagnostics;   /* bit 0: count the solves whose stamped matrix has a column with 0 < |a_ik| < 1e-15 max_j |a_jk| — the
                                   situation in which the reference's `if (Math.abs(f) < EPS) continue` (solveReal.ts:46) drops a
                                   row update that this library performs (spicey_last_skip_risk);
                            bit 1: record per step the one-shot linearisation error max_d |vd_new - vd_lin| over the diodes
                                   (spicey_get_lin_err); diagnostic only, never changes an iteration count */
} SpiceyOptions;

typedef struct SpiceyInfo {
  int32_t n_var;       /* n_nodes + nV */
  int32_t nnz_a;       /* structural nonzeros of A */
  int32_t nnz_lu;      /* nonzeros of L+U (incl. fill) under the chosen ordering */
  int32_t n_levels;    /* elimination-tree height = barrier-separated factor phases */
  int32_t threads;
  int32_t inst_per_wg;
  int32_t lds_bytes;   /* dynamic LDS per workgroup; 0 = global workspace */
  int32_t n_cur;       /* element-current columns */
  int32_t n_out;       /* recorded node-voltage columns */
  int32_t n_workgroups;
  int32_t interpreter;      /* 1, 2 or 3, see SpiceyOptions (3: n_workgroups = n_inst, inst_per_wg = wgs_per_inst = 1, lds_bytes 0 on
                               the global slab, the fields of the sparse program 0) */
  int32_t geometry;         /* 1 or 2 (v2), see SpiceyOptions */
  int32_t tail_levels;      /* v2: elimination-tree levels merged into the single-wave tail phase */
  int32_t wgs_per_inst;     /* workgroups cooperating on one instance (group mode), else 1 */
  int32_t resident_slots;   /* v2: 16-byte task records per thread kept in VGPRs */
  int64_t resident_tasks;   /* v2: factor/backward tasks held in registers */
  int64_t streamed_tasks;   /* v2: tasks still fetched from L2 every step */
  int64_t program_bytes;            /* device-side schedule ("program") size */
  int64_t algorithmic_bytes_solve;  /* SURVEY.md §8(d) formula */
  int32_t factor_reuse;     /* 1: no diodes / switches -> the factors of step 0 are reused, later steps solve only */
  int32_t n_fronts;         /* dense fronts of the upper elimination tree (0 = none) */
  int32_t front_cut;        /* first elimination-tree level handled by fronts (0 = none) */
  int32_t max_front;        /* rows of the largest front (padded to 16) */
  int64_t front_ws_bytes;   /* front workspace per instance */
  int32_t pcr_rows;         /* interpreter 2: rows of the tridiagonal top solved by one wave with parallel cyclic reduction (0 = none) */
  int32_t pcr_level;        /* first elimination-tree level of that top */
  int32_t hybrid_entries;   /* interpreter 2, hybrid workspace: entries of L+U (those the leaves of the elimination tree own) kept in
                               global memory because the whole L+U does not fit the LDS of one CU; 0 = everything in LDS */
  int32_t operand_addr;     /* interpreter 2: 1 = the runs of this handle that take the ready-argument kernel take its operand-address
                               form (LDS operands addressed in one instruction: the packed fresh shape, a program whose descriptor
                               fields hold indices from the start of the workspace, SPICEY_NO_OPERAND_ADDR not set); 0 = no such form */
} SpiceyInfo;

typedef struct SpiceyHandle SpiceyHandle;

/* Symbolic phase (MNA pattern, zero-free-diagonal row matching, nested-dissection ordering,
 * symbolic LU, level schedule) + upload.  Replaces the per-iteration dense allocation and
 * pivot search of simulateTRAN.ts:152-153 / solveReal.ts:15-34. */
int32_t spicey_create(const SpiceyDesc *desc, const SpiceyOptions *opt, SpiceyHandle **out);

/* One transient run of `steps`+1 points (step = 0..steps inclusive, t = step*dt;
 * simulateTRAN.ts:146-147) for all instances, continuing from the handle's current state
 * (a second run continues like the reference does).
 *   src_table   [steps+1][nV] source values at t = step*dt, shared by all instances
 *   out_v       [n_inst][steps+1][n_out]
 *   out_i       [n_inst][steps+1][n_cur] or NULL
 *   iters       [n_inst][steps+1] iterations executed per step (1..20) or NULL
 * HOST buffers; blocking. */
int32_t spicey_run(SpiceyHandle *h, int64_t steps, double dt, const double *src_table,
                   double *out_v, double *out_i, int32_t *iters);

/* Same with DEVICE buffers, enqueued on `stream` (a hipStream_t, NULL = default stream) without
 * synchronising: the error word is checked by spicey_sync(). */
int32_t spicey_run_device(SpiceyHandle *h, int64_t steps, double dt, const double *d_src_table,
                          double *d_out_v, double *d_out_i, int32_t *d_iters, void *stream);

/* Batched sweeps whose instances differ in their stimulus (a supply corner, an input amplitude, one PWL vector each):
 * src_per_inst = 0: src_table [steps+1][nV], shared by all instances (exactly spicey_run);
 *                1: src_table [n_inst][steps+1][nV], instance i reads block i.  Other values: SPICEY_ERR_BAD_DESC.
 * Every interpreter, workspace layout, K and group mode honours the layout.  Unlike spicey_run, the output buffers are
 * also filled when the call returns SPICEY_ERR_SINGULAR: the rows of every instance whose spicey_last_inst_status entry
 * is 0 are complete, the others are undefined. */
int32_t spicey_run_src(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst,
                       double *out_v, double *out_i, int32_t *iters);
/* The same with DEVICE buffers, enqueued on `stream` without synchronising (as spicey_run_device). */
int32_t spicey_run_device_src(SpiceyHandle *h, int64_t steps, double dt, const double *d_src_table, int32_t src_per_inst,
                              double *d_out_v, double *d_out_i, int32_t *d_iters, void *stream);
/* Per instance of the last run (after spicey_run* / spicey_sync), status[n_inst]: 0 = reached its last step;
 * SPICEY_ERR_SINGULAR = its own solve was singular (where the reference throws); -1 = stopped unfinished because another
 * instance in its workgroup failed (only when SpiceyInfo.inst_per_wg > 1); SPICEY_ERR_HIP = its launch aborted (group
 * mode).  A workgroup has one error flag, so the first singular solve stops all of its instances; the status words name
 * only that one.  The device state of an instance that did not reach its last step is undefined (some paths write state
 * during the run, e.g. capacitors beyond the register-resident ones): run it again from the state it entered with.  Returns
 * the number of nonzero entries; -1 without a handle or a buffer, before any run, and when the last run was refused or
 * failed before its launch finished (a structurally singular descriptor is answered: every instance SPICEY_ERR_SINGULAR). */
int32_t spicey_last_inst_status(SpiceyHandle *h, int32_t *status /* [n_inst] */);
/* Wait for enqueued runs; returns SPICEY_ERR_SINGULAR etc. like spicey_run.
 * Group mode (several workgroups per instance): every cross-workgroup wait is bounded in time; a launch whose wait runs
 * out aborts as a whole (nothing of it is kept): SPICEY_ERR_HIP with the first waiter's position (which wait, which
 * workgroup on which XCD, the value it waited for and the value it saw) in spicey_last_error() and on stderr.  Only with
 * SpiceyOptions.group_retry = 1 is the launch repeated ONCE from the state it started with, on the same stream; the
 * text of the aborted attempt then stays in spicey_last_error() (prefixed "recovered: ") although the call returns OK. */
int32_t spicey_sync(SpiceyHandle *h);
/* Number of launches this handle has repeated that way (0 in a healthy run; each is also reported on stderr). */
int32_t spicey_group_retries(const SpiceyHandle *h);
/* Group mode, summed over this handle's launches: waits that only the read-modify-write poll saw satisfied, i.e. where the
 * plain sc1 load poll kept returning an older value (kernels.hip, spin_until).  0 in a healthy run. */
int64_t spicey_group_stale_polls(const SpiceyHandle *h);

/* Final state after the last run (write-back to ckt: simulateTRAN.ts:221-237,122-124).
 * Any pointer may be NULL.  Arrays are [n_inst][n<kind>]. */
int32_t spicey_get_state(SpiceyHandle *h, double *C_vprev, double *L_iprev, double *D_vdprev,
                         int32_t *S_ison);

/* State entering the NEXT run (the counterpart of spicey_get_state; the reference keeps this state on the caller's
 * `ckt`, parseNetlist.ts:316,327,439,422, and a caller may rewrite it between two simulateTRAN calls).  HOST arrays
 * [n_inst][n<kind>]; a NULL pointer leaves that kind as it is.  Blocking. */
int32_t spicey_set_state(SpiceyHandle *h, const double *C_vprev, const double *L_iprev, const double *D_vdprev,
                         const int32_t *S_ison);
/* Back to the state the descriptor of spicey_create carried (kept in device memory): enqueued on `stream` (a
 * hipStream_t, NULL = default stream) as device-to-device copies, no synchronisation — every spicey_run_device after
 * it repeats the same transient instead of continuing the previous one. */
int32_t spicey_reset_state(SpiceyHandle *h, void *stream);

/* Total solves (= sum of iterations) executed by the last run, all instances. */
int64_t spicey_last_solve_count(SpiceyHandle *h);
/* Diagnostics (SpiceyOptions.diagnostics bit 0).  The reference eliminates with partial pivoting and skips a row update whose
 * multiplier a_ik / pivot is below 1e-15 (`if (Math.abs(f) < EPS) continue`, solveReal.ts:46): a nonzero coupling dropped —
 * floor conductances (diode gd 1e-12 S, switch 1/Roff) next to a clamped diode, a milliohm resistor or a large C/dt.  A sparse
 * static pivot order cannot reproduce that entry for entry; this library PERFORMS those updates (the physically consistent
 * answer) and says when the situation occurs: the number of (solve, column) pairs of the last run in which the stamped
 * matrix column held a nonzero entry below 1e-15 x the column's largest magnitude (per instance in per_inst[n_inst] if not
 * NULL; the return value is the sum; -1 without the option).  0 means the reference took no such shortcut on the stamped
 * matrix and the two results agree to the 1e-9 parity bar; > 0 means the reference's own result may differ from this one by
 * up to |v_k| * |a_ik| / a_ii per flagged coupling ("Where the reference skips row updates").
 * With SpiceyOptions.interpreter = 3 (reference order) the count is exact instead: the nonzero multipliers the skip dropped in
 * the run's completed solves, per instance. */
int64_t spicey_last_skip_risk(SpiceyHandle *h, int64_t *per_inst);
/* Diagnostics (SpiceyOptions.diagnostics bit 1): out[n_inst][steps+1] = per step the largest |vd(x) - vd_lin| over the diodes,
 * vd_lin being the junction voltage the step's LAST solve was linearised at (vdPrev on iteration 0, the previous iterate
 * afterwards: simulateTRAN.ts:81-85).  The reference iterates only on switch flips and never looks at this quantity; it is
 * reported, not acted on: iteration counts and results are identical with and without the option. */
int32_t spicey_get_lin_err(SpiceyHandle *h, double *out);
/* Duration in ms of the last run's kernel, measured with HIP events on the launch stream. */
double spicey_last_kernel_ms(SpiceyHandle *h);

int32_t spicey_get_info(SpiceyHandle *h, SpiceyInfo *info);
/* Interpreter 2: 1 = a run of `steps` steps on this handle takes the operand-address kernel whose tridiagonal top exchanges
 * its rows between the lanes' registers instead of through LDS (the packed fresh shape, SpiceyInfo.operand_addr = 1 and the
 * run within the ready-argument kernel's step range, a top of 2 .. 64 rows, SPICEY_NO_TOP_REGS not set when the handle was
 * created); 0 = it takes another kernel, or there is no handle.  The results are the same bits either way. */
int32_t spicey_top_regs_form(const SpiceyHandle *h, int64_t steps);
/* Interpreter 2: 1 = a run of `steps` steps on this handle takes the form of that kernel which keeps the row record of factor
 * level 0 in registers for the whole run (spicey_top_regs_form says 1, level 0 is streamed as row records, at most one per
 * thread and nothing else, the circuit is not linear, SPICEY_NO_U0_RESIDENT not set when the handle was created); 0 = it
 * takes another kernel, or there is no handle.  The results are the same bits either way. */
int32_t spicey_u0_resident_form(const SpiceyHandle *h, int64_t steps);
/* Interpreter 2: 1 = a run of `steps` steps on this handle takes the form of that kernel in which the lanes of the tridiagonal
 * top run the factor level right below it themselves (spicey_u0_resident_form says 1, that level is row records of the top's
 * rows and nothing else, SPICEY_NO_TOP_FOLD not set when the handle was created); 0 = it takes another kernel, or there is
 * no handle.  The results are the same bits either way. */
int32_t spicey_top_fold_form(const SpiceyHandle *h, int64_t steps);
/* Interpreter 2: 1 = a run of `steps` steps on this handle takes the form of that kernel whose update phase stamps the next
 * step's matrix and right-hand side from registers, with no stamping phase in the time loop (spicey_top_fold_form says 1,
 * every stamped entry and every row draws on values of one thread — no switch, no inductor, nothing beyond the resident
 * capacity —, SPICEY_NO_STAMP_FUSE not set when the handle was created); 0 = it takes another kernel, or there is no
 * handle.  The results are the same bits either way. */
int32_t spicey_stamp_fuse_form(const SpiceyHandle *h, int64_t steps);
/* Interpreter 2: 1 = a run of `steps` steps on this handle takes the form of that kernel whose time loop is written out for
 * what the plan holds (spicey_stamp_fuse_form says 1, every phase but factor level 0 is resident, no resident record uses the
 * overflow list, the first backward phase runs in the top's wave, no empty diagnostics phases were asked for,
 * SPICEY_NO_FIXED_SCHEDULE not set when the handle was created); 0 = it takes another kernel, or there is no handle.  The
 * results are the same bits either way. */
int32_t spicey_fixed_schedule_form(const SpiceyHandle *h, int64_t steps);
/* Human-readable description of the last error ("singular at inst 0 step 3 iter 0", the
 * hipGetErrorString text, …).  Valid until the next call on the handle. NULL handle -> global. */
const char *spicey_last_error(SpiceyHandle *h);
void spicey_destroy(SpiceyHandle *h);

/* Diagnostics: shader-clock cycles spent per phase kind by workgroup 0 during the last run (needs
 * SpiceyOptions.profile = 1).  out[72]: [0] prologue, [1] B stamp+rhs, [2] S switches, [3] A re-linearise,
 * [4] Z record/next-eval, [8+l] factor level l, [40+l] backward level l.  Returns the slot count. */
int32_t spicey_debug_phase_cycles(SpiceyHandle *h, uint64_t *out, int32_t n);
/* The same slots of launched workgroup `wg` (group mode: wg = group * wgs_per_inst + index).  In group mode the slots hold
 * 100 MHz wall-clock ticks per SECTION of the step: [1] B, [8] factor levels below the front cut, [9] fronts forward,
 * [10] fronts backward, [11] publish + group barrier, [12..20] inside the fronts, [40] backward levels, [4] Z. */
int32_t spicey_debug_phase_cycles_wg(SpiceyHandle *h, int32_t wg, uint64_t *out, int32_t n);
/* Diagnostics (SpiceyOptions.profile, circuits with dense fronts): per front of group `grp` four event times of the last
 * run — forward: children assembled / done, backward: parent's unknowns there / done — in 100 MHz ticks since the owning
 * workgroup entered the forward sweep, SUMMED over the solves (out[f*4+e]); meta[f*4+{0,1,2,3}] = pivots, boundary rows,
 * parent front, owning workgroup.  Returns the number of fronts (0: nothing recorded / cap_fronts too small). */
int32_t spicey_debug_front_ticks(SpiceyHandle *h, int32_t grp, uint64_t *out, int32_t *meta, int32_t cap_fronts);

/* ---------------------------------------------------------------------------------------------------------------
 * Several devices behind one handle (SURVEY.md §8(b) "device ordinal(s)", §8(e)): the n_inst instances of the descriptor
 * are block-partitioned over the listed devices (instance i -> devices[floor(i * n_dev / n_inst)], the partition of
 * spicey_amd/dist.py), one SpiceyHandle + stream per device inside THIS process; spicey_run_multi launches every shard
 * from its own host thread and each shard's results land directly in its slice of the caller's single host buffers
 * (that is the gather).  No data-path exchange between devices: instances are independent (simulateTRAN.ts:130 is one
 * circuit, one thread).  A device may be listed more than once (it then gets several shards; shards in group mode then
 * run one after the other on it — "Launch admission" at the top of this file).  opt->device is ignored.
 *   devices   [n_dev] HIP device ordinals, n_dev >= 1; n_dev > n_inst leaves the surplus devices idle
 * Errors: the first failing shard's status; spicey_multi_last_error names the device. */
typedef struct SpiceyMulti SpiceyMulti;
int32_t spicey_create_multi(const SpiceyDesc *desc, const SpiceyOptions *opt, const int32_t *devices, int32_t n_dev, SpiceyMulti **out);
/* Same buffers as spicey_run, for ALL instances: out_v [n_inst][steps+1][n_out], out_i, iters likewise or NULL. Blocking. */
int32_t spicey_run_multi(SpiceyMulti *m, int64_t steps, double dt, const double *src_table, double *out_v, double *out_i, int32_t *iters);
/* With per-instance source tables (src_per_inst as for spicey_run_src): each shard gets its slice of the tables. */
int32_t spicey_run_multi_src(SpiceyMulti *m, int64_t steps, double dt, const double *src_table, int32_t src_per_inst,
                             double *out_v, double *out_i, int32_t *iters);
int32_t spicey_get_state_multi(SpiceyMulti *m, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison);
/* Shard `shard` (0 .. n_shards-1): its SpiceyInfo, first instance and instance count; returns SPICEY_ERR_BAD_DESC past the end. */
int32_t spicey_multi_get_shard(SpiceyMulti *m, int32_t shard, SpiceyInfo *info, int32_t *device, int32_t *first_inst, int32_t *n_inst);
int64_t spicey_multi_last_solve_count(SpiceyMulti *m);  /* all shards */
int32_t spicey_multi_group_retries(SpiceyMulti *m);      /* spicey_group_retries summed over the shards */
int64_t spicey_multi_group_stale_polls(SpiceyMulti *m);  /* spicey_group_stale_polls summed over the shards */
double spicey_multi_last_kernel_ms(SpiceyMulti *m);     /* the slowest shard's kernel */
const char *spicey_multi_last_error(SpiceyMulti *m);    /* NULL handle -> the calling thread's last failed create */
void spicey_destroy_multi(SpiceyMulti *m);

/* ---------------------------------------------------------------------------------------------------------------
 * Waveform measurements on the device (what SPICE users know as .meas): a reduction pass of its own over the step-major
 * waveform buffers a transient run wrote, stream-ordered behind it; only [n_inst][n_req][8] doubles leave the device.
 * One request = one signal, one window of steps, one kind:
 *   kind       0 = stats, 1 = crossings
 *   signal     0 = column of out_v, 1 = column of out_i
 *   col        the measured column; col_ref = -1: none, else the signal is x[col] - x[col_ref] of the same array (one
 *              rounded subtraction)
 *   step_from, step_to   inclusive window; step_to = -1: the last point
 *   level, dir crossings: the threshold, and +1 = rises, -1 = falls, 0 = both
 * Results, 8 doubles per (instance, request):
 *   stats      {min, max, step_min, step_max, sum, sumsq, first, last}.  step_min / step_max: the step of the FIRST
 *              occurrence of the extreme, as a double.  The extremes use the plain comparisons x < m and x > m: a NaN sample
 *              is ignored by them and propagates into the sums.
 *   crossings  {count, t_first, t_last, 0, 0, 0, 0, 0} over the intervals (k, k + 1) with both steps inside the window; rise:
 *              x_k < level && x_k+1 >= level, fall: x_k > level && x_k+1 <= level; the crossing time is
 *              ((double)k + (level - x_k) / (x_k+1 - x_k)) * dt; t_first = t_last = -1.0 when count = 0.
 * Every field is a function of the window's samples, dt and the request only (the summation order is fixed: chunks of 256
 * steps counted from step_from, sequential inside a chunk, chunk partials added in ascending order): it does not depend on
 * n_inst, on the other requests of the list or on the launch.  No FMA contraction. */
typedef struct SpiceyMeasReq {
  int32_t kind, signal, col, col_ref;
  int64_t step_from, step_to;
  double level;
  int32_t dir, reserved; /* reserved: 0 */
} SpiceyMeasReq;

/* Bytes of device workspace spicey_measure_device needs (request table + chunk partials); -1 for counts <= 0. */
int64_t spicey_measure_workspace_bytes(int32_t n_inst, int64_t n_points, int32_t n_req);
/* The reduction alone, on any DEVICE buffers d_v [n_inst][n_points][n_v] and d_i [n_inst][n_points][n_i] (or NULL):
 * needs no handle.  reqs is a HOST array; d_meas [n_inst][n_req][8] and d_work (work_bytes >=
 * spicey_measure_workspace_bytes) are DEVICE buffers.  Enqueued on `stream` (a hipStream_t, NULL = default stream)
 * without synchronising; the request table travels into the head of the workspace.  SPICEY_ERR_BAD_DESC, with a text in
 * spicey_last_error(NULL) and nothing launched, for: an unknown kind, signal or dir; a column out of range; signal = 1
 * with d_i == NULL; a window outside [0, n_points) or with step_from > step_to; a workspace that is too small;
 * n_req <= 0. */
int32_t spicey_measure_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v,
                              const double *d_i, int32_t n_i, const SpiceyMeasReq *reqs, int32_t n_req, double *d_meas,
                              void *d_work, int64_t work_bytes, void *stream);
/* One transient run (as spicey_run_src) whose waveforms stay on the device: out_v (and out_i only if a request has
 * signal = 1) are allocated there, reduced by spicey_measure_device on the handle's stream, and only
 * meas [n_inst][n_req][8] and iters [n_inst][steps+1] (or NULL) come back — also after SPICEY_ERR_SINGULAR, where the
 * rows of the instances whose spicey_last_inst_status entry is nonzero are undefined.  Columns are those of the handle
 * (SpiceyInfo.n_out, n_cur); n_points = steps + 1.  State, solve count, skip risk and kernel ms are queried as after
 * spicey_run. */
int32_t spicey_run_measure(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst,
                           const SpiceyMeasReq *reqs, int32_t n_req, double *meas, int32_t *iters);
/* Duration in ms of the last spicey_run_measure's reduction (both of its kernels), measured with HIP events. */
double spicey_last_measure_ms(SpiceyHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Harmonics of a transient's waveforms on the device (what SPICE users know as .four): a third reduction pass over the
 * same step-major buffers.  One request = one signal (signal, col, col_ref exactly as in SpiceyMeasReq), a fundamental
 * f0 in Hz, a harmonic count n_harm and a window of steps: the N = step_to - step_from samples step_from .. step_to - 1
 * enter the sums — the sample at step_to closes the last period and is left out (the rectangular rule, exact for a
 * waveform that is periodic in the window); step_to = -1: n_points - 1.
 * Results, 1 + 2 n_harm doubles per (instance, request) at the head of a row of out_stride doubles, the rest of the row 0:
 *   {C0, C1, S1, ..., CH, SH}   C0 = sum x_s,  C_h = sum x_s c(h, s),  S_h = sum x_s s(h, s)
 * over the ABSOLUTE step s (phases refer to t = 0, not to the window), with the twiddles
 *   r = (double)(h s) (f0 dt), the integer product in 64 bits;  r = r - floor(r);  a = 2 pi r;  c = cos(a), s = sin(a)
 * evaluated by the HOST's libm: the device reads a table the host built, one per basis (f0, step_from, step_to), uploaded
 * into the head of the workspace.  So a_h = 2 C_h / N, b_h = 2 S_h / N give the harmonic M cos(2 pi h f0 t + phi) with
 * M = hypot(a_h, b_h), phi = atan2(-b_h, a_h), and C0 / N is the mean.  A window that is no whole number of periods leaks;
 * that is the caller's business and not refused.
 * Every row is a function of the window's samples, dt and the request only (the summation order is that of the
 * measurements above: chunks of 256 steps counted from step_from, sequential inside a chunk with sums that start at 0.0,
 * chunk partials added in ascending order; every product and sum rounded on its own, no FMA contraction): it does not
 * depend on n_inst, on the other requests of the list or of its basis, or on the launch. */
#define SPICEY_FOUR_MAX_HARM 16
typedef struct SpiceyFourReq {
  int32_t signal, col, col_ref, n_harm; /* n_harm in 1..SPICEY_FOUR_MAX_HARM */
  int64_t step_from, step_to;           /* samples step_from .. step_to-1 are summed; step_to = -1: n_points-1 */
  double f0;                            /* Hz, > 0 and finite */
} SpiceyFourReq;

/* Bytes of device workspace spicey_fourier_device needs for this request list (request table, bases, twiddles, chunk
 * partials); -1 for a list whose windows, harmonic counts or fundamentals no launch accepts, and for counts <= 0. */
int64_t spicey_fourier_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyFourReq *reqs, int32_t n_req);
/* The reduction alone, on any DEVICE buffers d_v [n_inst][n_points][n_v] and d_i [n_inst][n_points][n_i] (or NULL):
 * needs no handle.  reqs is a HOST array; d_out [n_inst][n_req][out_stride] and d_work (work_bytes >=
 * spicey_fourier_workspace_bytes) are DEVICE buffers.  Enqueued on `stream` (a hipStream_t, NULL = default stream)
 * without synchronising.  SPICEY_ERR_BAD_DESC, with a text containing "fourier" in spicey_last_error(NULL), nothing
 * launched and the buffers untouched, for: an unknown signal; a column out of range; signal = 1 with d_i == NULL;
 * step_from < 0, step_to beyond the run or step_from >= step_to; n_harm outside 1..16; f0 or dt not finite or <= 0;
 * n_harm f0 dt > 0.5 (above Nyquist); out_stride < 1 + 2 max n_harm; a workspace that is too small; n_req <= 0; null
 * buffers. */
int32_t spicey_fourier_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v,
                              const double *d_i, int32_t n_i, const SpiceyFourReq *reqs, int32_t n_req, double *d_out,
                              int32_t out_stride, void *d_work, int64_t work_bytes, void *stream);
/* spicey_run_measure with the harmonics pass on the same stream behind the measurements: one transient run, currents
 * recorded only if a request of either list has signal = 1, both reductions over the same device waveforms; only meas
 * [n_inst][n_req][8] (n_req may be 0: meas may then be NULL and no measurement pass runs), four
 * [n_inst][n_four][four_stride] (n_four >= 1) and iters (or NULL) come back.  Everything else — SPICEY_ERR_SINGULAR, the
 * repeated launch of group_retry, the queries afterwards — is as for spicey_run_measure. */
int32_t spicey_run_measure_fourier(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst,
                                   const SpiceyMeasReq *reqs, int32_t n_req, double *meas, const SpiceyFourReq *freqs,
                                   int32_t n_four, double *four, int32_t four_stride, int32_t *iters);
/* Duration in ms of the last spicey_run_measure_fourier's harmonics pass (both of its kernels), measured with HIP events. */
double spicey_last_fourier_ms(SpiceyHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Edge timing on the device (propagation delay, rise time, settling time, pulse width, period): a fourth reduction pass
 * over the same step-major buffers.
 * An EDGE names one signal (signal, col, col_ref exactly as in SpiceyMeasReq: one rounded subtraction per sample), a
 * direction dir (+1 rise, -1 fall, 0 either), an occurrence n != 0 (n >= 1: the n-th crossing from the start of the edge's
 * search range, n <= -1: the |n|-th from its end) and a level:
 *   level_kind 0   absolute: L = level
 *   level_kind 1   L = lo + level * (hi - lo) with (lo, hi) = (min, max) of the same signal over the inclusive base window
 *                  [base_from, base_to] (base_to = -1: n_points - 1) of THAT instance
 *   level_kind 2   the same with (lo, hi) = (first, last) sample of the base window
 * the difference, the product and the sum each rounded on its own; `level` is then any finite fraction (1.02 is legal).  A
 * flat signal gives L = lo and no crossing.  base_from / base_to are not read for level_kind 0.
 * A crossing is that of SpiceyMeasReq's kind 1: a rise is x_k < L && x_k+1 >= L, a fall x_k > L && x_k+1 <= L; it lies in
 * interval k, at the time ((double)k + (L - x_k) / (x_k+1 - x_k)) * dt, evaluated in that order.  A NaN sample or level
 * never makes a crossing.
 * A REQUEST has a window [step_from, step_to] (step_to = -1: n_points - 1; the intervals with both ends inside), a targ
 * edge and, with has_trig = 1, a trig edge.  The trig's search range is the window.  So is the targ's (SPICE's rule, the
 * default); with targ_from_trig = 1 it is the window's intervals k >= k_trig.  All selection is by the integer interval
 * index; interpolated times are never compared, so a targ crossing in the trigger's own interval counts, even where its
 * interpolated time lies a fraction of a step before the trigger's.  With the same edge as trig and targ and
 * targ_from_trig = 1, n = 1 therefore finds the trigger's own crossing: a period is asked for as trig n = 1, targ n = 2
 * under the default rule.
 * Results, 8 doubles per (instance, request):
 *   {k_trig, t_trig, L_trig, k_targ, t_targ, L_targ, n_trig, n_targ}
 * k_* the selected interval as a double, -1.0 when not found (t_* = -1.0 then); L_* the level used in that instance; n_*
 * the number of crossings of that edge in its search range.  Without a trig: k_trig = t_trig = -1, L_trig = 0, n_trig = 0.
 * With targ_from_trig = 1 and no trig found the targ is not searched: k_targ = t_targ = -1, n_targ = 0, L_targ still the
 * level.
 * Every field has one value in any evaluation order (integer counts, min / max / first / last, two fixed formulas; no FMA
 * contraction), so a row is a function of the window's samples, dt and the request alone: it does not depend on n_inst,
 * the launch or the other requests of the list. */
typedef struct SpiceyTimingEdge {
  int32_t signal, col, col_ref, dir;
  int32_t n, level_kind;
  int64_t base_from, base_to;
  double level;
} SpiceyTimingEdge;
typedef struct SpiceyTimingReq {
  int64_t step_from, step_to;
  int32_t has_trig, targ_from_trig; /* 0 / 1 each */
  SpiceyTimingEdge trig, targ;      /* trig is not read when has_trig = 0 */
} SpiceyTimingReq;

/* Bytes of device workspace spicey_timing_device needs for this request list (edge and request tables, the base windows'
 * results and the measurement pass's workspace for them, chunk counts); -1 for counts <= 0 or a list no launch accepts. */
int64_t spicey_timing_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyTimingReq *reqs, int32_t n_req);
/* The reduction alone, on any DEVICE buffers d_v [n_inst][n_points][n_v] and d_i [n_inst][n_points][n_i] (or NULL):
 * needs no handle.  reqs is a HOST array; d_out [n_inst][n_req][8] and d_work (work_bytes >=
 * spicey_timing_workspace_bytes) are DEVICE buffers.  The base windows of the relative levels go through the kernels of
 * spicey_measure_device as stats requests into the workspace, then two kernels of this pass; all enqueued on `stream` (a
 * hipStream_t, NULL = default stream) without synchronising.  SPICEY_ERR_BAD_DESC, with a text containing "timing" in
 * spicey_last_error(NULL), nothing launched and the buffers untouched, for: an unknown signal, dir or level_kind; n = 0;
 * a level or fraction that is not finite; a column out of range; signal = 1 with d_i == NULL; a window or base window
 * outside the run or with from > to; a window of one point (no interval); targ_from_trig without has_trig (or either not
 * 0 / 1); dt not finite or <= 0; a workspace that is too small; n_req <= 0; null buffers. */
int32_t spicey_timing_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v,
                             const double *d_i, int32_t n_i, const SpiceyTimingReq *reqs, int32_t n_req, double *d_out,
                             void *d_work, int64_t work_bytes, void *stream);
/* spicey_run_measure_fourier with the timing pass behind the other two: one transient run, currents recorded only if a
 * request of any list has signal = 1, then the measurement pass (if n_req > 0), the harmonics pass (if n_four > 0) and
 * the timing pass (n_timing >= 1) on the handle's stream over the same device waveforms; only meas [n_inst][n_req][8],
 * four [n_inst][n_four][four_stride], timing [n_inst][n_timing][8] and iters (or NULL) come back — also after
 * SPICEY_ERR_SINGULAR.  meas / four may be NULL when their count is 0.  Everything else is as for spicey_run_measure. */
int32_t spicey_run_measure_timing(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst,
                                  const SpiceyMeasReq *reqs, int32_t n_req, double *meas, const SpiceyFourReq *freqs,
                                  int32_t n_four, double *four, int32_t four_stride, const SpiceyTimingReq *treqs,
                                  int32_t n_timing, double *timing, int32_t *iters);
/* Duration in ms of the last spicey_run_measure_timing's timing pass (the base windows' kernels included), measured with
 * HIP events. */
double spicey_last_timing_ms(SpiceyHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Spectrum of a transient's waveforms on the device (what SPICE users know as fft / spec / .meas ... FFT): a fifth pass
 * over the same step-major buffers, for the questions fourier() cannot answer because nobody knows f0.  Unlike the other
 * passes it is no streaming reduction but a batched FFT in LDS, one workgroup per (instance, request).
 * One request = one signal (signal, col, col_ref exactly as in SpiceyMeasReq: one rounded subtraction per sample), a first
 * step step_from, a length N = 2^log2n (3 <= log2n <= 13: N = 8 .. 8192), a window (0 rectangular, 1 periodic Hann), an
 * inclusive band of bins [bin_from, bin_to] inside [0, N/2] and a kind (0 bins, 1 dominant).  The N samples x_j =
 * signal at step step_from + j, j = 0 .. N-1, enter; they must lie inside the run.
 * The numbers, in this order, every product, sum and difference rounded on its own (no FMA contraction):
 *   1. y_j = x_j w_j, one rounded product (skipped for window 0), w_j = 0.5 - 0.5 cos((2.0 M_PI j) / N) from the HOST's
 *      libm, one table per distinct (N, window).
 *   2. Radix-2 decimation in time over N complex points (im = 0) on the bit-reversed input: for h = 1, 2, 4, ... N/2 and
 *      every pair (a, b) = (z[i], z[i+h]), i = 2h g + j, 0 <= j < h, with W = T[j N / (2h)]:
 *        tr = b.re W.re - b.im W.im,  ti = b.re W.im + b.im W.re,  z[i] = a + t,  z[i+h] = a - t.
 *      T[k] = (cos((2.0 M_PI k) / N), -sin((2.0 M_PI k) / N)), k < N/2, from the HOST's libm, T[0] = (1, 0) and T[N/4] =
 *      (0, -1) set exactly; one table per distinct N.  The device never evaluates a sine.
 *   3. P_k = re_k re_k + im_k im_k.
 * So X_k = sum_j y_j exp(-2 pi i j k / N): phases refer to the window's FIRST sample (fourier()'s refer to t = 0).
 * Results, at the head of a row of out_stride doubles per (instance, request), the rest of the row 0:
 *   kind 0   2 (bin_to - bin_from + 1) doubles {re, im} per bin of the band
 *   kind 1   8 doubles {k, re_k, im_k, P_k-1, P_k, P_k+1, 0, 0}: k the bin of the band with the largest P by the plain
 *            comparison P > best in ascending k from best = 0 (the first occurrence wins, a NaN never wins), as a double;
 *            k = -1 and the other fields 0 when no bin wins (an all-zero band).  The neighbours come from the bins
 *            0 .. N/2 whether or not they lie in the band; one that does not exist is -1.0.
 * A row is a function of the N samples and the request alone: not of n_inst, the launch, the workgroup size or the other
 * requests of the list. */
#define SPICEY_SPEC_MIN_LOG2N 3
#define SPICEY_SPEC_MAX_LOG2N 13
typedef struct SpiceySpecReq {
  int32_t signal, col, col_ref, kind;         /* kind: 0 bins, 1 dominant */
  int64_t step_from;                          /* samples step_from .. step_from + N - 1 */
  int32_t log2n, window, bin_from, bin_to;    /* N = 2^log2n; window: 0 rectangular, 1 periodic Hann */
} SpiceySpecReq;

/* Bytes of device workspace spicey_spectrum_device needs for this request list (request table, twiddle and window
 * tables); -1 for a list whose lengths, windows, bands or first steps no launch accepts, and for counts <= 0. */
int64_t spicey_spectrum_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceySpecReq *reqs, int32_t n_req);
/* The pass alone, on any DEVICE buffers d_v [n_inst][n_points][n_v] and d_i [n_inst][n_points][n_i] (or NULL): needs no
 * handle.  reqs is a HOST array; d_out [n_inst][n_req][out_stride] and d_work (work_bytes >=
 * spicey_spectrum_workspace_bytes) are DEVICE buffers.  One kernel launch per distinct N of the list (dynamic LDS of 16 N
 * bytes each), enqueued on `stream` (a hipStream_t, NULL = default stream) without synchronising.  SPICEY_ERR_BAD_DESC,
 * with a text containing "spectrum" in spicey_last_error(NULL), nothing launched and the buffers untouched, for: an
 * unknown signal, kind or window; a column out of range; signal = 1 with d_i == NULL; log2n outside 3..13; step_from < 0
 * or step_from + N > n_points; a band outside [0, N/2] or with bin_from > bin_to; out_stride shorter than the longest row;
 * dt not finite or <= 0; a workspace that is too small; n_req <= 0; null buffers. */
int32_t spicey_spectrum_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v,
                               const double *d_i, int32_t n_i, const SpiceySpecReq *reqs, int32_t n_req, double *d_out,
                               int32_t out_stride, void *d_work, int64_t work_bytes, void *stream);
/* spicey_run_measure_timing with the spectrum pass behind the other three: one transient run, currents recorded only if
 * a request of any list has signal = 1, then the measurement pass (if n_req > 0), the harmonics pass (if n_four > 0), the
 * timing pass (if n_timing > 0) and the spectrum pass (n_spec >= 1) on the handle's stream over the same device
 * waveforms; only meas, four, timing, spec [n_inst][n_spec][spec_stride] and iters (or NULL) come back — also after
 * SPICEY_ERR_SINGULAR.  meas / four / timing may be NULL when their count is 0.  Everything else is as for
 * spicey_run_measure. */
int32_t spicey_run_measure_spectrum(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst,
                                    const SpiceyMeasReq *reqs, int32_t n_req, double *meas, const SpiceyFourReq *freqs,
                                    int32_t n_four, double *four, int32_t four_stride, const SpiceyTimingReq *treqs,
                                    int32_t n_timing, double *timing, const SpiceySpecReq *sreqs, int32_t n_spec, double *spec,
                                    int32_t spec_stride, int32_t *iters);
/* Duration in ms of the last spicey_run_measure_spectrum's spectrum pass (all of its launches), measured with HIP events. */
double spicey_last_spectrum_ms(SpiceyHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Products of two signals (what SPICE users ask of a power stage: the power an element takes, P_out / P_in): a sixth
 * pass over the same step-major buffers.  Every other pass reads ONE signal; the average of a product is not the product
 * of the averages, so v i has to be formed sample by sample — here, on the device.
 * One request = two factors a and b, each exactly SpiceyMeasReq's signal / col / col_ref (they may come from different
 * arrays: a voltage times a current), a sign and an inclusive window of steps.  Per step k of the window
 *   a_k = A[k][a_col], minus A[k][a_col_ref] when a_col_ref >= 0 (one rounded subtraction); b_k likewise from B;
 *   p_k = a_k * b_k, one rounded product, negated (exactly) when neg = 1.
 * Result, SPICEY_POWER_ROW doubles per (instance, request):
 *   {min_p, max_p, step_min, step_max, sum_p, first_p, last_p, sum_aa, sum_bb, first_a, last_a, first_b, last_b, 0, 0, 0}
 * with sum_aa = sum a_k a_k and sum_bb = sum b_k b_k (the square rounded first, then added).  The extremes and their steps
 * follow the rule of the measurement pass's stats: the plain comparisons p < m and p > m in ascending step order, so the
 * FIRST occurrence is named and a NaN never replaces an extreme (it does enter the sums); each chunk starts from its first
 * sample.  Summation order, the project's fixed rule: chunks of 256 steps counted from step_from, inside a chunk one
 * addition after the other from the chunk's first term, the chunk partials added in ascending order.  No FMA contraction,
 * no atomics: a row is a function of the window's samples and the request alone — not of n_inst, the launch or the other
 * requests of the list. */
#define SPICEY_POWER_ROW 16
typedef struct SpiceyPowerReq {
  int32_t a_signal, a_col, a_col_ref;   /* factor a: exactly SpiceyMeasReq's signal / col / col_ref */
  int32_t b_signal, b_col, b_col_ref;   /* factor b likewise; a and b may come from different arrays */
  int32_t neg, reserved;                /* neg = 1: p = -(a b) (an exact negation); reserved: 0 */
  int64_t step_from, step_to;           /* inclusive window; step_to = -1: the last point */
} SpiceyPowerReq;                        /* 48 bytes */

/* Bytes of device workspace spicey_power_device needs: the request table, then the chunk partials
 * [n_inst][ceil(n_points / 256)][n_req][16] doubles, each region rounded up to 256 bytes; -1 for counts <= 0. */
int64_t spicey_power_workspace_bytes(int32_t n_inst, int64_t n_points, int32_t n_req);
/* The pass alone, on any DEVICE buffers d_v [n_inst][n_points][n_v] and d_i [n_inst][n_points][n_i] (or NULL): needs no
 * handle.  reqs is a HOST array; d_out [n_inst][n_req][SPICEY_POWER_ROW] and d_work (work_bytes >=
 * spicey_power_workspace_bytes) are DEVICE buffers.  Two kernels, enqueued on `stream` (a hipStream_t, NULL = default
 * stream) without synchronising.  SPICEY_ERR_BAD_DESC, with a text that starts "power: " in spicey_last_error(NULL),
 * nothing launched and the buffers untouched, for: an unknown signal; a column out of range; a current factor with d_i ==
 * NULL; neg not 0 or 1; a nonzero reserved; a window outside the run or with step_from > step_to; dt not finite or <= 0; a
 * workspace that is too small; n_req <= 0; null buffers. */
int32_t spicey_power_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v,
                            const double *d_i, int32_t n_i, const SpiceyPowerReq *reqs, int32_t n_req, double *d_out,
                            void *d_work, int64_t work_bytes, void *stream);
/* spicey_run_measure_spectrum with the product pass behind the other four: one transient run, currents recorded only if
 * a request of any list names one (here: a_signal = 1 or b_signal = 1), then the measurement pass (if n_req > 0), the
 * harmonics pass (if n_four > 0), the timing pass (if n_timing > 0), the spectrum pass (if n_spec > 0) and the product
 * pass (n_power >= 1) on the handle's stream over the same device waveforms; only meas, four, timing, spec, power
 * [n_inst][n_power][SPICEY_POWER_ROW] and iters (or NULL) come back — also after SPICEY_ERR_SINGULAR.  meas / four /
 * timing / spec may be NULL when their count is 0.  Everything else is as for spicey_run_measure. */
int32_t spicey_run_measure_power(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst,
                                 const SpiceyMeasReq *reqs, int32_t n_req, double *meas, const SpiceyFourReq *freqs,
                                 int32_t n_four, double *four, int32_t four_stride, const SpiceyTimingReq *treqs,
                                 int32_t n_timing, double *timing, const SpiceySpecReq *sreqs, int32_t n_spec, double *spec,
                                 int32_t spec_stride, const SpiceyPowerReq *preqs, int32_t n_power, double *power,
                                 int32_t *iters);
/* Duration in ms of the last spicey_run_measure_power's product pass (both kernels), measured with HIP events. */
double spicey_last_power_ms(SpiceyHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Waveform VALUES (a decimated trace to plot, the waveform on the caller's own time grid, one signal's value where
 * another crosses — SPICE's .meas FIND / DERIV ... AT / WHEN): a pass over the same step-major buffers whose answers are
 * samples, not sums.  A request names its signal y exactly as SpiceyMeasReq does (signal, col, col_ref: one rounded
 * subtraction per sample) and is of one of three kinds.
 *
 * kind 0, TRACE.  The inclusive window [step_from, step_to] (step_to = -1: the last point) of n samples in `buckets` = B
 *   buckets, 1 <= B <= min(n, SPICEY_TRACE_MAX_BUCKETS).  Bucket b covers the steps step_from + floor(b n / B) ..
 *   step_from + floor((b + 1) n / B) - 1, the products formed in 64-bit integers; B <= n, so no bucket is empty.  Result:
 *   6 doubles per bucket {min, step_min, max, step_max, first, last}, 6 B in all; step_* is the absolute step of the FIRST
 *   occurrence, as a double.  The extremes follow the rule of the measurement pass's stats inside a bucket: the bucket is
 *   cut into sub-chunks of 256 steps counted from the bucket's own first step, each sub-chunk starts from its first sample
 *   and uses the plain comparisons x < m and x > m in ascending step order, and the sub-chunks are combined in ascending
 *   order by the same comparisons — so a NaN never replaces an extreme, and is one only where it is a (sub-chunk's, then
 *   the bucket's) first sample, exactly as under stats.  With B = n the row is the waveform itself.
 * kind 1, POINTS.  A run [first, first + count) of the call's point table (SpiceyValPoint {k, f}, shared by all
 *   instances; 0 <= k <= n_points - 2, 0 <= f <= 1).  Per point, every operation rounded on its own (no FMA contraction):
 *     d = y[k+1] - y[k];  value = (f == 0) ? y[k] : (f == 1) ? y[k+1] : y[k] + f d;  slope = d / dt.
 *   Result: 4 doubles per point {k, f, value, slope}, 4 count in all.
 * kind 2, FIND.  The same two formulas at the crossing a row of the timing pass found for THAT instance: with row =
 *   timing[inst][timing_row] ({k_trig, t_trig, L_trig, k_targ, t_targ, L_targ, n_trig, n_targ}), k = row[3], L = row[5] and
 *   x the edge's own signal (x_signal, x_col, x_col_ref), f = (L - x[k]) / (x[k+1] - x[k]) — the timing pass's operations in
 *   its order, so (k + f) dt is row[4] bit for bit.  Result: 4 doubles {k, f, value, slope}.  k = -1 (edge not found), or
 *   any k outside [0, n_points - 2], gives {-1, 0, 0, 0} and no sample is read.
 *
 * Each request's row sits at the head of out_stride doubles, the rest 0.  No field is a floating-point accumulation: a row
 * is a function of the samples, dt and the request alone (kind 2: and of that instance's timing row) — not of n_inst, the
 * launch or the other requests of the list — and is bit-identical to a plain numpy evaluation
 * (spicey_amd.measure.reduce_reference_values).  Fields a kind does not use are ignored; reserved must be 0. */
#define SPICEY_TRACE_MAX_BUCKETS 4096
#define SPICEY_VAL_TRACE 0
#define SPICEY_VAL_POINTS 1
#define SPICEY_VAL_FIND 2
typedef struct SpiceyValReq {
  int32_t kind;                          /* SPICEY_VAL_TRACE, _POINTS, _FIND */
  int32_t signal, col, col_ref;          /* y: exactly SpiceyMeasReq's signal / col / col_ref */
  int32_t x_signal, x_col, x_col_ref;    /* kind 2: the signal of the edge (that of the timing request's targ) */
  int32_t timing_row;                    /* kind 2: index into the timing list of the same call */
  int64_t step_from, step_to;            /* kind 0: inclusive window; step_to = -1: the last point */
  int64_t first, count;                  /* kind 1: the run of the point table */
  int32_t buckets, reserved;             /* kind 0: B; reserved: 0 */
} SpiceyValReq;                          /* 72 bytes */
typedef struct SpiceyValPoint {
  int64_t k;                             /* the interval [k, k + 1], 0 <= k <= n_points - 2 */
  double f;                              /* the place in it, 0 <= f <= 1 */
} SpiceyValPoint;                        /* 16 bytes */

/* Bytes of device workspace spicey_values_device needs: the point table (n_pts x 16 bytes), the tables of the trace and of
 * the points / find requests, then the trace partials [n_inst][sum over trace requests of B * S][6] doubles with S =
 * ceil(ceil(n / B) / 256), each region rounded up to 256 bytes.  The partials scale with the samples the traces cover (B S
 * <= n / 256 + 2 B), not with n_req times the chunks of the run.  -1 for a list no launch accepts (columns, buffers and the
 * point table's values are not looked at). */
int64_t spicey_values_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyValReq *reqs, int32_t n_req, int64_t n_pts);
/* The pass alone, on any DEVICE buffers d_v [n_inst][n_points][n_v] and d_i [n_inst][n_points][n_i] (or NULL): needs no
 * handle.  reqs and pts (n_pts >= 0 records, NULL when 0) are HOST arrays; d_timing [n_inst][n_timing][8] (the result of
 * spicey_timing_device; NULL when no request is of kind 2), d_out [n_inst][n_req][out_stride] and d_work (work_bytes >=
 * spicey_values_workspace_bytes) are DEVICE buffers.  A clear of d_out and up to three kernels, enqueued on `stream` (a
 * hipStream_t, NULL = default stream) without synchronising.  SPICEY_ERR_BAD_DESC, with a text that starts "values: " in
 * spicey_last_error(NULL), nothing launched and the buffers untouched, for: an unknown kind or signal; a column out of
 * range; a current signal with d_i == NULL; a window outside the run; buckets outside 1 .. min(n, 4096); a point run
 * outside the table; a point's k outside [0, n_points - 2] or f outside [0, 1] or not finite; n_points < 2 with a points or
 * find request; timing_row outside [0, n_timing) or a kind-2 request with d_timing == NULL; out_stride shorter than the
 * longest row; dt not finite or <= 0; a workspace that is too small; n_req <= 0; null buffers; a nonzero reserved. */
int32_t spicey_values_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v,
                             const double *d_i, int32_t n_i, const SpiceyValReq *reqs, int32_t n_req,
                             const SpiceyValPoint *pts, int64_t n_pts, const double *d_timing, int32_t n_timing, double *d_out,
                             int32_t out_stride, void *d_work, int64_t work_bytes, void *stream);

/* The reduced run by struct: what the five spicey_run_measure* entry points do, with the values pass behind them and
 * every list optional.  One transient run, currents recorded only if a request of any list names one, then on the
 * handle's stream over the same device waveforms the passes whose count is > 0, in this order: measurement, harmonics,
 * timing, spectrum, products, values; only their results and iters (or NULL) come back — also after SPICEY_ERR_SINGULAR.
 * The values pass reads the timing pass's device rows as its d_timing, so a kind-2 request's timing_row indexes `treqs`.
 * struct_bytes = sizeof(SpiceyReducedLists) of the caller's header: a later pass is appended behind the last member, and
 * the library reads the members it knows.  SPICEY_ERR_BAD_DESC, text starting "reduced: ", nothing run, for: lists NULL;
 * struct_bytes smaller than the 160 bytes of this version; a nonzero reserved; a negative count; every count 0; a list or
 * result pointer NULL where its count is > 0.  A kind-2 request whose timing_row >= n_timing is refused
 * by the values pass's own judge ("values: ...").  Everything else is as for spicey_run_measure. */
typedef struct SpiceyReducedLists {
  int64_t struct_bytes;
  const SpiceyMeasReq *reqs;     double *meas;    /* [n_inst][n_req][8] */
  const SpiceyFourReq *freqs;    double *four;    /* [n_inst][n_four][four_stride] */
  const SpiceyTimingReq *treqs;  double *timing;  /* [n_inst][n_timing][8] */
  const SpiceySpecReq *sreqs;    double *spec;    /* [n_inst][n_spec][spec_stride] */
  const SpiceyPowerReq *preqs;   double *power;   /* [n_inst][n_power][SPICEY_POWER_ROW] */
  int32_t n_req, n_four, four_stride, n_timing, n_spec, spec_stride, n_power, n_values;
  const SpiceyValReq *vreqs;     double *values;  /* [n_inst][n_values][values_stride] */
  const SpiceyValPoint *pts;     int64_t n_pts;
  int32_t values_stride, reserved;                /* reserved: 0 */
} SpiceyReducedLists;                             /* 160 bytes */
int32_t spicey_run_reduced(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst,
                           const SpiceyReducedLists *lists, int32_t *iters);
/* Duration in ms of the last spicey_run_reduced's values pass (the clear and its kernels), measured with HIP events. */
double spicey_last_values_ms(SpiceyHandle *h);

/* Library build info: "spicey_hip <abi> gfx950 …" */
const char *spicey_version(void);

/* ---------------------------------------------------------------------------------------------------------------
 * AC sweep: replaces the per-frequency body of
 *   simulateAC(ckt)              /root/reference/lib/analysis/simulateAC.ts:64-130
 * i.e. buildLinearSystemForAC (:25-62, lib/stamping/stamp{Admittance,VoltageSource}Complex.ts), solveComplex
 * (lib/math/solveComplex.ts:4-73) and the recording (:84-126), for every (instance, frequency) pair in one launch.
 * The host keeps the frequency list (buildFrequencyArray :9-23, utils/logspace.ts — Math.pow is engine-defined), the
 * source phasors (Complex.fromPolar, math/Complex.ts:16-19) and the `R <name> must be > 0` check (:39).
 * Diodes and switches of the descriptor are ignored, like the reference's AC analysis ignores them.
 *   freqs   [n_freq] Hz
 *   vph     [n_inst][nV][2] source phasors (re, im)
 *   out_v   [n_inst][n_freq][n_out][2]   complex node voltages (re, im)
 *   out_i   [n_inst][n_freq][nR+nC+nL+nV][2] complex currents in the reference's recording order R, C, L, V, or NULL
 * HOST buffers; blocking.  Status: SPICEY_ERR_SINGULAR -> Error("Singular matrix (complex)") (solveComplex.ts:28),
 * SPICEY_ERR_COMPLEX_DIV -> Error("Complex divide by ~0") (a pivot with |z|^2 < 1e-15, Complex.ts:40-42); the message of
 * spicey_ac_last_error names the first failing (instance, frequency), the one at which the reference would throw.
 * spicey_ac_create reads SpiceyOptions.device, threads, force_global, debug bits 4 and 7, and interpreter: 3 selects the
 * reference-order AC engine — the reference's own solveComplex (dense stamp in element order, partial pivoting on V8's
 * Math.hypot, its |f| < EPS row-update skip, back substitution in its order), one workgroup per (instance, frequency):
 * every output bit and every SPICEY_ERR_SINGULAR / SPICEY_ERR_COMPLEX_DIV exactly where the reference has them (an
 * inductor's "Complex divide by ~0" included, frequency by frequency; no structural pre-check).  A | b in LDS up to n ~ 97
 * unknowns, else an n x (n + 1) slab per slot in global memory, at most 1 GiB per launch (force_global = 1: always).
 * threads: 0 = 64 for n <= 64, else 256; 64..1024 honoured (same bits), others refused with SPICEY_ERR_BAD_DESC.
 * spicey_ac_get_info then reports interpreter = 3, threads, lds_bytes (0 on the slab) and n_workgroups (the slots of
 * the last run).  Never chosen automatically; any other interpreter value keeps the default path. */
typedef struct SpiceyAcHandle SpiceyAcHandle;
int32_t spicey_ac_create(const SpiceyDesc *desc, const SpiceyOptions *opt /* device, threads, force_global, debug, interpreter */,
                         SpiceyAcHandle **out);
int32_t spicey_ac_run(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, double *out_v, double *out_i);
int32_t spicey_ac_get_info(SpiceyAcHandle *h, SpiceyInfo *info);
double spicey_ac_last_kernel_ms(SpiceyAcHandle *h);
const char *spicey_ac_last_error(SpiceyAcHandle *h);
void spicey_ac_destroy(SpiceyAcHandle *h);

/* Per instance of the last sweep (spicey_ac_run / spicey_ac_run_measure), status[n_inst]: 0, or the code
 * (SPICEY_ERR_SINGULAR / SPICEY_ERR_COMPLEX_DIV) of the instance's LOWEST failing frequency index, and in
 * first_freq[n_inst] (or NULL) that index, -1 for an instance that is fine.  Both engines answer; for the sparse engine the
 * words are those after the dense partial-pivoting fallback has repeated the solves that tripped a pivot guard.  Returns the
 * number of nonzero entries; -1 without a handle or a status buffer, before any run, and when the last run was refused
 * before its launch (bad arguments, a HIP error).  A structurally singular descriptor is answered: every instance
 * SPICEY_ERR_SINGULAR at frequency index 0.
 * When spicey_ac_run returns SPICEY_ERR_SINGULAR / SPICEY_ERR_COMPLEX_DIV, out_v / out_i have still been copied: the rows
 * of every instance whose status is 0 are complete (each (instance, frequency) solve is independent; a failed solve leaves
 * only its own slot undefined). */
int32_t spicey_ac_last_inst_status(SpiceyAcHandle *h, int32_t *status /* [n_inst] */, int64_t *first_freq /* [n_inst] or NULL */);

/* ---------------------------------------------------------------------------------------------------------------
 * Measurements over an AC sweep on the device (the -3 dB corner, the peak, the phase at unity gain): a reduction pass over
 * the complex buffers [n_inst][n_freq][n][2] a sweep wrote; only [n_inst][n_req][8] doubles leave the device.
 * One request = one complex signal H_k over the frequency indices k, one inclusive window, one kind:
 *   num_signal   0 = out_v, 1 = out_i; num_col the column; num_col_ref = -1: none, else the numerator is
 *                a[num_col] - a[num_col_ref] of the same array, one rounded subtraction per part
 *   den_signal   -1 = no denominator (H = numerator), else 0 / 1 with den_col / den_col_ref likewise: H = num / den by the
 *                reference's Complex.div arithmetic (math/Complex.ts:38-47) without its |d| < EPS throw,
 *                  d = b.re b.re + b.im b.im;  re = (a.re b.re + a.im b.im) / d;  im = (a.im b.re - a.re b.im) / d
 *                — a zero denominator gives the IEEE result (NaN or infinity)
 *   what         the measured real quantity q_k: 0 = |H|^2 = re re + im im, 1 = re, 2 = im.  No sqrt, log or atan2 runs on
 *                the device: magnitudes, decibels and phases are the host's to derive from the returned re / im, so a CPU
 *                and the device can agree on every bit
 *   k_from, k_to inclusive window of frequency indices; k_to = -1: the last index
 *   kind         0 = extrema, 1 = crossings
 *   level, dir, which, rel   crossings only (0 otherwise): dir +1 = rises, -1 = falls, 0 = both; which 0 = report the
 *                first crossing's bracket, 1 = the last one's; rel 0: the threshold is `level`, rel 1: it is
 *                level * q_{k_from}, one rounded product ("3 dB below the passband", per instance)
 *   reserved     0
 * Results, 8 doubles per (instance, request):
 *   extrema    {min, max, k_min, k_max, re@k_min, im@k_min, re@k_max, im@k_max}: the result of m = q_{k_from}, then the
 *              plain comparisons q < m and q > m in ascending k — the FIRST occurrence wins and a NaN sample never replaces
 *              an extreme (a window whose first sample is NaN keeps that NaN as both extremes, at k_from).  A one-sample
 *              window is the point read-out "H at this frequency".
 *   crossings  {count, k_first, k_last, re_k, im_k, re_k+1, im_k+1, thr} over the intervals (k, k + 1) with both ends in
 *              the window: a rise is q_k < thr && q_k+1 >= thr, a fall q_k > thr && q_k+1 <= thr; k_first / k_last are
 *              the lower ends of the first / last such interval, the four H parts those of the interval `which` names, thr
 *              the threshold actually used.  count = 0: k_first = k_last = -1 and the H parts are 0.
 * No field is a floating-point accumulation (counts are integers), so every result is a function of the window's samples
 * and the request alone: it does not depend on the launch geometry, on n_inst or on the other requests of the list.  The
 * implementation keeps that true: no atomics, no FMA contraction. */
typedef struct SpiceyAcMeasReq {
  int32_t num_signal, num_col, num_col_ref;
  int32_t den_signal, den_col, den_col_ref;
  int32_t what, kind;
  int64_t k_from, k_to;
  double level;
  int32_t dir, which, rel, reserved;
} SpiceyAcMeasReq;

/* Bytes of device workspace spicey_ac_measure_device needs (the request table: the kernel keeps no partials); -1 for
 * counts <= 0. */
int64_t spicey_ac_measure_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t n_req);
/* The reduction alone, on any DEVICE buffers d_v [n_inst][n_freq][n_v][2] and d_i [n_inst][n_freq][n_i][2] (or NULL): needs
 * no handle.  reqs is a HOST array; d_meas [n_inst][n_req][8] and d_work (work_bytes >= spicey_ac_measure_workspace_bytes)
 * are DEVICE buffers.  Enqueued on `stream` (a hipStream_t, NULL = default stream) without synchronising.
 * SPICEY_ERR_BAD_DESC, with a text containing "ac measure" in spicey_last_error(NULL) and nothing launched, for: an unknown
 * kind, signal, what, dir, which or rel; a column out of range; a current signal with d_i == NULL; a window outside
 * [0, n_freq) or with k_from > k_to; n_req <= 0; a nonzero reserved word; a workspace that is too small. */
int32_t spicey_ac_measure_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const double *d_i,
                                 int32_t n_i, const SpiceyAcMeasReq *reqs, int32_t n_req, double *d_meas, void *d_work,
                                 int64_t work_bytes, void *stream);
/* One sweep — exactly that of spicey_ac_run, in either engine — whose results stay on the device: out_v (and out_i only if
 * a request has a current signal) are allocated there and reduced on the handle's stream after the dense fallback has
 * repaired its slots; only meas [n_inst][n_req][8] (HOST) comes back.  Columns are those of the handle (SpiceyInfo.n_out,
 * n_cur).  The return value and spicey_ac_last_inst_status are as after spicey_ac_run; meas is also filled when the sweep
 * reports SPICEY_ERR_SINGULAR / SPICEY_ERR_COMPLEX_DIV, where the rows of instances whose status is nonzero are undefined.
 * A refused request list (SPICEY_ERR_BAD_DESC, text in spicey_ac_last_error) runs nothing. */
int32_t spicey_ac_run_measure(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, const SpiceyAcMeasReq *reqs,
                              int32_t n_req, double *meas);
/* Duration in ms of the last spicey_ac_run_measure's reduction, measured with HIP events. */
double spicey_ac_last_measure_ms(SpiceyAcHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Current injection and noise analysis.  The reference has no current source, so this has no reference behaviour: it is
 * the one thing an analogue user needs on top of simulateAC to ask for an output impedance or for thermal noise.
 *
 * spicey_ac_run_inject is spicey_ac_run with a current I = (re, im) injected into node_p and drawn from node_n (node ids
 * of the descriptor, 0 = ground): after the source phasors, b[node_p - 1] += I and b[node_n - 1] -= I, at every frequency
 * and in every instance, in every path a solve can take (the dense partial-pivoting fallback included).  vph may be NULL:
 * every phasor zero.  Refused with SPICEY_ERR_BAD_DESC, nothing run: inj NULL, struct_bytes != sizeof(SpiceyAcInject), a node
 * outside [0, n_nodes], node_p == node_n, a non-finite amplitude, a handle of the reference-order engine (interpreter = 3).
 * A later spicey_ac_run on the same handle injects nothing and gives the bits it gave before.
 *
 * With unit injection, every phasor zero and out = v(node_p) - v(node_n), the complex symmetry of the MNA matrix of R, C, L
 * and V makes the solution the adjoint one (DESIGN.md "Noise analysis"): out is Z_out, i(V_in) the voltage gain V_in -> out,
 * i(R_k) the gain to out of a voltage source in series with R_k.  The noise pass reduces such a sweep:
 *   d_spec    [n_inst][n_freq][4]  {onoise = sum_k kt4 R_k |i(R_k)|^2 in V^2/Hz, gain2 = |i(V_in)|^2 (0 without an input),
 *                                   zout_re, zout_im}
 *   d_contrib [n_inst][nR]         every resistor's kt4 R |i(R)|^2 integrated over the window by the trapezoidal rule, V^2
 *   d_total   [n_inst][2]          the same integral of onoise and of onoise / gain2 (an IEEE quotient: inf / NaN show)
 * with the fixed operation and summation order of noise_exec.h, no FMA contraction, no atomics: the CPU and the device agree
 * on every bit.  Nothing is square-rooted or compared on the device.  A window of one frequency integrates to +0.0.
 *   out_p, out_n   columns of out_v (d_v) of the output pair, -1 = ground; not both -1, not equal
 *   in_col         column of out_i (d_i) of the input source's current, -1 = none
 *   k_from, k_to   inclusive window of frequency indices, k_to = -1: the last
 *   kt4            4 k_B T, formed on the host (k_B = 1.380649e-23); finite and >= 0
 * The resistors' currents are the first nR columns of out_i. */
typedef struct SpiceyAcInject {
  int64_t struct_bytes;
  int32_t node_p, node_n;
  double re, im;
} SpiceyAcInject;
typedef struct SpiceyAcNoiseReq {
  int64_t struct_bytes;
  int32_t out_p, out_n, in_col, reserved;
  int64_t k_from, k_to;
  double kt4;
} SpiceyAcNoiseReq;
int32_t spicey_ac_run_inject(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, const SpiceyAcInject *inj,
                             double *out_v, double *out_i);
/* Bytes of device workspace spicey_ac_noise_device needs (the request record); -1 for counts <= 0. */
int64_t spicey_ac_noise_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nR);
/* The reduction alone, on any DEVICE buffers (d_v [n_inst][n_freq][n_v][2], d_i [n_inst][n_freq][n_i][2], d_R [n_inst][nR] in
 * ohms, d_freqs [n_freq], the three results, d_work): needs no handle.  req is a HOST struct.  Enqueued on `stream` without
 * synchronising.  SPICEY_ERR_BAD_DESC with a text containing "noise" in spicey_last_error(NULL), nothing launched, for: a
 * null buffer, counts <= 0, nR > n_i, a column out of range, out_p == out_n, a window outside [0, n_freq) or with
 * k_from > k_to, a bad kt4, a nonzero reserved word, a wrong struct_bytes, a workspace that is too small. */
int32_t spicey_ac_noise_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                               const double *d_R, int32_t nR, const double *d_freqs, const SpiceyAcNoiseReq *req, double *d_spec,
                               double *d_contrib, double *d_total, void *d_work, int64_t work_bytes, void *stream);
/* One injected sweep (spicey_ac_run_inject; the currents are always recorded) whose out_v / out_i stay on the device and are
 * reduced there on the handle's stream, after the dense fallback has repaired its slots; spec [n_inst][n_freq][4], contrib
 * [n_inst][nR] and total [n_inst][2] (HOST) come back, and in gain [n_inst][n_freq][2] (HOST, or NULL) the complex i(V_in) whose
 * squared magnitude is gain2 (untouched when in_col = -1).  Columns are those of the handle.  The return value and
 * spicey_ac_last_inst_status are as after spicey_ac_run: an instance with a failed solve has its code and undefined rows, the
 * others are complete.  A refused request or injection (SPICEY_ERR_BAD_DESC, text in spicey_ac_last_error) runs nothing. */
int32_t spicey_ac_run_noise(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, const SpiceyAcInject *inj,
                            const SpiceyAcNoiseReq *req, double *spec, double *contrib, double *total, double *gain);
/* Duration in ms of the last spicey_ac_run_noise's reduction, measured with HIP events. */
double spicey_ac_last_noise_ms(SpiceyAcHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * AC sensitivity analysis: how out = v(out_p) - v(out_n) moves when an element value moves, for every R, C and L at every
 * frequency, from two sweeps.  Sweep D is the plain one (the netlist's phasors), sweep X has every phasor zero and a unit
 * current injected into the output pair; both record the element currents.  The matrix is complex symmetric, so X is the
 * adjoint solution and d out / d Y_e = -dx_e dd_e (DESIGN.md "AC sensitivities").  With prod = i_X(e) i_D(e), w = (2 pi) f and
 * p the element's value, the absolute sensitivity S_e = p d out / d p is
 *   R: p prod        C: j prod / (w p)  (+0 where w p == 0)        L: j prod (w p)
 * and the relative ones are m_e = Re(S_e / H) = d ln|H| / d ln p_e and phi_e = Im(S_e / H) = d arg H / d ln p_e (radians), H = out
 * of sweep D (IEEE quotients: H == 0 shows inf / NaN).  The pass reduces the two sweeps:
 *   d_spec  [n_inst][n_freq][6]      {H.re, H.im, wc_mag = sum_e t_e |m_e|, var_mag = sum_e (t_e m_e)^2, wc_ph = sum_e t_e |phi_e|,
 *                                     var_ph = sum_e (t_e phi_e)^2}, t_e = tol[e] the element's relative tolerance
 *   d_peak  [n_inst][nE][4]          {m_e where |m_e| is largest over the window, its frequency index, phi_e where |phi_e| is
 *                                     largest, its frequency index} — the first of equal magnitudes, indices stored as doubles
 *   d_full  [n_inst][n_freq][nE][2]  {m_e, phi_e}, optional
 * with the fixed operation and summation order of sens_exec.h, no FMA contraction, no atomics: the CPU and the device agree on
 * every bit, and d_peak holds the same bits with and without d_full.  Elements are numbered as the columns of out_i: the nR
 * resistors, the nC capacitors, the nL inductors; nE = nR + nC + nL.
 *   out_p, out_n   columns of out_v (d_v) of the output pair, -1 = ground; not both -1, not equal
 *   nR, nC, nL     the element counts (a handle's run wants its own)
 *   k_from, k_to   inclusive window of frequency indices of d_peak, k_to = -1: the last */
typedef struct SpiceyAcSensReq {
  int64_t struct_bytes;
  int32_t out_p, out_n, nR, nC, nL, reserved;
  int64_t k_from, k_to;
} SpiceyAcSensReq;
/* Bytes of device workspace spicey_ac_sens_device needs (the request record and the tolerances); -1 for counts <= 0. */
int64_t spicey_ac_sens_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nE);
/* The reduction alone, on any DEVICE buffers (d_v_dir [n_inst][n_freq][n_v][2] of sweep D, d_i_dir and d_i_adj
 * [n_inst][n_freq][n_i][2] of sweeps D and X, d_R / d_C / d_L [n_inst][n<kind>] in ohms, farads and henries — NULL where the
 * count is 0 —, d_freqs [n_freq], d_spec, d_peak, d_full or NULL, d_work): needs no handle.  req and tol [nE] are HOST data:
 * the tolerances are judged here and go to the device through the workspace, behind the request record.  Enqueued on `stream`
 * without synchronising.  SPICEY_ERR_BAD_DESC with a text containing "sens" in spicey_last_error(NULL), nothing launched,
 * for: a null required buffer, counts <= 0, nE = 0, a negative count, nR + nC + nL > n_i, a column out of range, out_p ==
 * out_n, a window outside [0, n_freq) or with k_from > k_to, a negative or non-finite tolerance, a nonzero reserved word, a
 * wrong struct_bytes, a workspace that is too small. */
int32_t spicey_ac_sens_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v_dir, int32_t n_v, const double *d_i_dir,
                              const double *d_i_adj, int32_t n_i, const double *d_R, const double *d_C, const double *d_L, const double *tol,
                              const double *d_freqs, const SpiceyAcSensReq *req, double *d_spec, double *d_peak, double *d_full, void *d_work,
                              int64_t work_bytes, void *stream);
/* Two sweeps on the handle — D with vph and no injection, then X with inj and every phasor zero; inj names the nodes of the
 * output pair with amplitude 1 — whose out_v / out_i stay on the device and are reduced there on the handle's stream, after
 * the dense fallback has repaired their slots; spec [n_inst][n_freq][6], peak [n_inst][nE][4] and, if not NULL, full
 * [n_inst][n_freq][nE][2] (HOST) come back.  tol is HOST [nE].  Columns are those of the handle, and req's nR, nC, nL must be
 * the handle's.  A slot's status is D's where nonzero, else X's; the return value and spicey_ac_last_inst_status follow from
 * that merged table as after spicey_ac_run: an instance with a failed solve has its code and undefined rows, the others are
 * complete.  A refused request, tolerance list or injection (SPICEY_ERR_BAD_DESC, text in spicey_ac_last_error; the
 * reference-order engine, interpreter = 3, refuses every injection) runs nothing.  A later spicey_ac_run gives the bits it
 * gave before.  spicey_ac_last_kernel_ms reports the sum of the two sweeps. */
int32_t spicey_ac_run_sens(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, const SpiceyAcInject *inj,
                           const SpiceyAcSensReq *req, const double *tol, double *spec, double *peak, double *full);
/* Duration in ms of the last spicey_ac_run_sens's reduction, measured with HIP events. */
double spicey_ac_last_sens_ms(SpiceyAcHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Monte Carlo tolerance analysis (SPICE's .mc): the distribution of |H|^2, H = v(out_p) - v(out_n), over n_inst samples whose R,
 * C and L are drawn on the device around their nominal values, swept in one batched sweep and reduced ACROSS the instances on
 * the device: per frequency the order statistics at given ranks, the sum and the sum of squares, the number of samples outside
 * a spec mask; per sample the number of frequencies at which it violates the mask.  Fixed operation order (mc_exec.h), integer
 * random numbers, no FMA contraction, no atomics: the CPU and the device agree on every bit.
 *
 * The draw.  Sample s, element e (the column order of out_i: the nR resistors, the nC capacitors, the nL inductors; nE = nR + nC
 * + nL) takes Philox4x32-10 of counter (s, e, 0, 0) under key (seed & 0xffffffff, seed >> 32), forms the 52-bit integer
 * m = (x0 << 20) | (x1 >> 12), and interpolates the HOST-built table icdf [K + 1], K = 2^log2K, log2K in [0, 12], of the inverse
 * distribution function in units of the element's tolerance: j = m >> (52 - log2K), frac = the remaining bits times 2^-(52 - log2K),
 * d = icdf[j] + frac (icdf[j + 1] - icdf[j]).  With g = 1 + tol[e] d a capacitor or inductor becomes nom g; a resistor becomes
 * R' = R g in ohms, and the array the sweep reads gets the quotient 1.0 / R'.  keep_first: sample 0 takes g = 1 without drawing,
 * so its rows are the nominal bits.  The nominal values are rows per sample, [n_inst][n<kind>].
 *
 * The reduction.  q[s][k] = H.re H.re + H.im H.im, each part of H one rounded subtraction (a column of -1 is ground).  A sample
 * marked invalid leaves every statistic.  A violation at k is !(q >= lo[k] && q <= hi[k]) — a NaN violates —, lo / hi being
 * limits of |H|^2 (+-inf: none; a NULL side: none on that side; both NULL: no mask, nothing violates).
 *   d_sample [n_inst][2] int64      {frequencies at which the sample violates, the lowest such index or -1}; {-1, -1} if invalid
 *   d_freq   [n_freq][4 + n_rank]   {n_valid, valid samples violating at k, sum of q, sum of q q, q_(ranks[0]), q_(ranks[1]), ...}:
 *                                   q_(r) the r-th smallest of the n_valid values (NaNs sort behind +inf); the sums run over the
 *                                   sorted values, lane l of 64 adding x[l], x[l + 64], ... from +0.0 and the partials meeting
 *                                   by s[l] += s[l + stride], stride 32 .. 1
 * Each frequency is sorted by one workgroup in LDS, so n_inst <= 16384. */
typedef struct SpiceyAcMcReq {
  int64_t struct_bytes;
  int32_t out_p, out_n;   /* columns of out_v (d_v) of the output pair, -1 = ground; not both -1, not equal (the draw ignores them) */
  int32_t log2K;          /* the table has 2^log2K + 1 entries */
  int32_t keep_first;     /* nonzero: sample 0 is the nominal circuit */
  uint64_t seed;
  int64_t reserved;       /* 0 */
} SpiceyAcMcReq;
/* Bytes of device workspace that serve spicey_ac_mc_draw_device and spicey_ac_mc_reduce_device alike; -1 for counts <= 0,
 * n_inst > 16384, log2K outside [0, 12] or n_rank < 0. */
int64_t spicey_ac_mc_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nE, int32_t log2K, int32_t n_rank);
/* The draw alone, on any DEVICE buffers (d_R in ohms, d_C, d_L: nominal [n_inst][n<kind>]; d_Rinv_out, d_C_out, d_L_out: drawn,
 * the first as 1 / ohms; NULL where the count is 0; d_work): needs no handle.  req, tol [nE] and icdf [K + 1] are HOST data, judged
 * here; they go to the device through the workspace.  Enqueued on `stream` without synchronising.  SPICEY_ERR_BAD_DESC with a
 * text containing "mc" in spicey_last_error(NULL), nothing launched, for: a null required buffer, n_inst <= 0 or > 16384, a
 * negative count, nE = 0, a negative or non-finite tolerance, tol[e] max|icdf| >= 1 (a value could turn non-positive), a
 * non-finite or decreasing table, log2K outside [0, 12], a nonzero reserved word, a wrong struct_bytes, a workspace that is too
 * small. */
int32_t spicey_ac_mc_draw_device(int32_t device, int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C,
                                 const double *d_L, const double *tol, const double *icdf, const SpiceyAcMcReq *req, double *d_Rinv_out,
                                 double *d_C_out, double *d_L_out, void *d_work, int64_t work_bytes, void *stream);
/* The reduction alone, on any DEVICE buffer d_v [n_inst][n_freq][n_v][2] (with d_sample, d_freq, d_work): needs no handle.  req,
 * valid [n_inst] (one byte per sample, nonzero = valid; NULL: all), lo / hi [n_freq] (or NULL) and ranks [n_rank], each in [0,
 * n_valid), are HOST data.  Enqueued on `stream` without synchronising.  Refused like the draw, and for: n_freq or n_v <= 0,
 * n_rank < 0, a column out of range, out_p == out_n, a rank outside [0, n_valid). */
int32_t spicey_ac_mc_reduce_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const uint8_t *valid,
                                   const double *lo, const double *hi, const int64_t *ranks, int32_t n_rank, const SpiceyAcMcReq *req,
                                   int64_t *d_sample, double *d_freq, void *d_work, int64_t work_bytes, void *stream);
/* A Monte Carlo run on the handle, whose n_inst instances are the samples and whose rows are their nominal values: everything is
 * judged first (a refusal — SPICEY_ERR_BAD_DESC, text in spicey_ac_last_error — runs nothing); the draw writes scratch value
 * arrays (the handle's own are never written); ONE sweep, exactly that of spicey_ac_run in either engine and in every path a solve
 * can take, the dense fallback included, reads them; its voltages stay on the device and currents are neither recorded nor
 * allocated.  A sample is valid when none of its solves failed.  Per probability p in probs [n_prob], each in [0, 1], the ranks
 * r = (int64) floor(p (double)(n_valid - 1)) and min(r + 1, n_valid - 1) are reduced, so n_rank = 2 n_prob and the host
 * interpolates.  Back come freq_stats [n_freq][4 + 2 n_prob], sample [n_inst][2] (int64) and, with keep_first and nominal not
 * NULL, nominal [n_freq][2]: the complex H of sample 0.  tol [nE], icdf, lo, hi (or NULL) and probs are HOST arrays.  The return
 * value and spicey_ac_last_inst_status are as after spicey_ac_run.  When no sample is valid nothing is reduced and the outputs
 * are untouched.  A later spicey_ac_run gives the bits it gave before. */
int32_t spicey_ac_run_mc(SpiceyAcHandle *h, int64_t n_freq, const double *freqs, const double *vph, const SpiceyAcMcReq *req, const double *tol,
                         const double *icdf, const double *lo, const double *hi, const double *probs, int32_t n_prob, double *freq_stats,
                         int64_t *sample, double *nominal);
/* Duration in ms of the last spicey_ac_run_mc's reduction, and of its draw, measured with HIP events. */
double spicey_ac_last_mc_ms(SpiceyAcHandle *h);
double spicey_ac_last_mc_draw_ms(SpiceyAcHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Monte Carlo of transient runs: the distribution of measured scalars over n_inst samples whose R, C and L are drawn on the
 * device, run as the instances of ONE transient, measured by the passes of spicey_run_reduced and reduced ACROSS the instances
 * on the device.  Fixed operation order (tran_mc_exec.h), integer random numbers, no FMA contraction, no atomics: the CPU and
 * the device agree on every bit.
 *
 * The draw is that of spicey_ac_mc_draw_device (counter, key, table, operations), except that a resistor's array gets R' = R g
 * in ohms: the transient kernels form 1.0 / R themselves.
 *
 * A scalar is a program of at most 48 instructions over a stack of at most 4 doubles, run per sample on its rows of the passes
 * with fixed rows — 0 measure [8], 1 timing [8], 2 power [SPICEY_POWER_ROW]:
 *   FIELD (pass, row, field)   pushes rows_pass[s][row][field]
 *   CONST (c)                  pushes c
 *   ADD SUB MUL DIV            pop b, pop a, push a o b: one rounded operation
 *   GUARD                      pops g; if !(g >= 0) the scalar is NaN whatever else the program computes
 * and the one value left is x[s][j]; a NaN is stored as 0x7ff8000000000000, and so is every x of an invalid sample.
 * There is no comparison other than GUARD's: "a > 0" is GUARD(a) followed by GUARD(0 / a), whose quotient is NaN exactly at a = 0.
 *
 * The reduction.  A violation of scalar j is !(x >= lo[j] && x <= hi[j]): a NaN violates (lo / hi NULL: -inf / +inf).
 *   d_sample [n_inst][2] int64           {scalars the sample violates, the lowest such j or -1}; {-1, -1} if invalid
 *   d_stat   [n_scalar][8 + 2 n_prob]    {n_valid, n_num, n_viol, sum x, sum x x, s_min, s_max, 0, q_(r0), q_(r0 + 1), q_(r1), ...}:
 *                                        n_num the valid samples that are not NaN; the sums over those, sorted, lane l of 64
 *                                        adding x[l], x[l + 64], ... from +0.0 and the partials meeting by s[l] += s[l + stride],
 *                                        stride 32 .. 1; s_min / s_max the lowest sample index with the smallest / largest
 *                                        value; per probability p the order statistics at r = (int64)(p (double)(n_num - 1))
 *                                        and min(r + 1, n_num - 1).  n_num = 0: sums +0.0, indices -1, order statistics NaN.
 * The values are ordered as unsigned integers (-inf < ... < -0 < +0 < ... < +inf < NaN < invalid) by one workgroup per scalar
 * in LDS, so n_inst <= 16384. */
#define SPICEY_MCOP_FIELD 1
#define SPICEY_MCOP_CONST 2
#define SPICEY_MCOP_ADD 3
#define SPICEY_MCOP_SUB 4
#define SPICEY_MCOP_MUL 5
#define SPICEY_MCOP_DIV 6
#define SPICEY_MCOP_GUARD 7
#define SPICEY_MC_SCALAR_INS 48
#define SPICEY_MC_SCALAR_STACK 4
typedef struct SpiceyMcIns {
  int32_t op;                /* SPICEY_MCOP_* */
  int32_t pass, row, field;  /* FIELD; else 0 */
  double c;                  /* CONST (finite); else 0 */
} SpiceyMcIns;               /* 24 bytes */
typedef struct SpiceyMcScalar {
  int32_t n_ins;             /* 1 .. SPICEY_MC_SCALAR_INS */
  int32_t reserved;          /* 0 */
  SpiceyMcIns ins[SPICEY_MC_SCALAR_INS];
} SpiceyMcScalar;            /* 1160 bytes */
typedef struct SpiceyTranMcReq {
  int64_t struct_bytes;
  int32_t log2K;             /* the table has 2^log2K + 1 entries */
  int32_t keep_first;        /* nonzero: sample 0 is the nominal circuit */
  uint64_t seed;
  int64_t reserved;          /* 0 */
} SpiceyTranMcReq;
/* The rows of one pass on the device: [n_inst][n_rows][stride] (d_rows NULL and n_rows 0: the pass did not run). */
typedef struct SpiceyMcRows {
  const double *d_rows;
  int32_t n_rows, stride;
} SpiceyMcRows;
/* Bytes of device workspace that serve spicey_tran_mc_draw_device and spicey_tran_mc_reduce_device alike; -1 for arguments no
 * launch accepts. */
int64_t spicey_tran_mc_workspace_bytes(int32_t n_inst, int32_t n_scalar, int32_t nE, int32_t log2K, int32_t n_prob);
/* The draw alone on any DEVICE buffers, as spicey_ac_mc_draw_device but with d_R_out in ohms.  Refusals are SPICEY_ERR_BAD_DESC
 * with a text starting "tran mc: " in spicey_last_error(NULL), nothing launched. */
int32_t spicey_tran_mc_draw_device(int32_t device, int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C,
                                   const double *d_L, const double *tol, const double *icdf, const SpiceyTranMcReq *req, double *d_R_out,
                                   double *d_C_out, double *d_L_out, void *d_work, int64_t work_bytes, void *stream);
/* The scalars and the reduction alone on any DEVICE row buffers: rows [3] (measure, timing, power), scalars [n_scalar], valid
 * [n_inst] (bytes, NULL: all), lo / hi [n_scalar] (or NULL) and probs [n_prob] (each in [0, 1]) are HOST data; d_x [n_inst][n_scalar],
 * d_stat and d_sample as above.  Needs no handle; enqueued on `stream` without synchronising.  SPICEY_ERR_BAD_DESC, text
 * starting "tran mc: ", nothing launched, for: a program whose stack underflows, exceeds 4 or does not end at depth 1; n_ins
 * outside [1, 48]; an unknown opcode; a FIELD of a pass without rows, or whose pass, row or field is out of range; a CONST that
 * is not finite; a nonzero reserved word or unused instruction word; n_inst <= 0 or > 16384; n_scalar <= 0; n_prob < 0; a
 * probability outside [0, 1]; a NaN limit; a null buffer; a pass with n_rows < 0, stride <= 0 or rows without a pointer; a
 * workspace that is too small. */
int32_t spicey_tran_mc_reduce_device(int32_t device, int32_t n_inst, const SpiceyMcRows *rows, const SpiceyMcScalar *scalars, int32_t n_scalar,
                                     const uint8_t *valid, const double *lo, const double *hi, const double *probs, int32_t n_prob, double *d_x,
                                     double *d_stat, int64_t *d_sample, void *d_work, int64_t work_bytes, void *stream);
/* A Monte Carlo run on the handle, whose n_inst instances are the samples and whose value rows are their nominal values.
 * Everything is judged first (a refusal — SPICEY_ERR_BAD_DESC, text in spicey_last_error(h) — runs nothing); the draw writes
 * scratch value arrays (the handle's own are never written); ONE transient, exactly that of spicey_run_reduced, reads them; the
 * passes of `lists` run behind it as in spicey_run_reduced and their rows stay on the device (the result pointers of `lists`
 * are ignored); a sample is valid iff its spicey_last_inst_status entry is 0; the scalars and the reduction run over the valid
 * samples, and stat [n_scalar][8 + 2 n_prob], sample [n_inst][2], x [n_inst][n_scalar] (or NULL) and iters (or NULL) come
 * back.  The spectrum, fourier and values lists are refused in this call.  With no valid sample nothing is reduced and the
 * outputs are untouched.  The return value, the end state and spicey_last_inst_status are as after spicey_run_reduced of the
 * drawn circuits; a later plain run binds the handle's own arrays and gives the bits it gave before.  tol [nE], icdf, scalars,
 * lo, hi (or NULL) and probs are HOST arrays. */
int32_t spicey_run_mc(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *lists,
                      const SpiceyTranMcReq *req, const double *tol, const double *icdf, const SpiceyMcScalar *scalars, int32_t n_scalar,
                      const double *lo, const double *hi, const double *probs, int32_t n_prob, double *stat, int64_t *sample, double *x,
                      int32_t *iters);
/* Duration in ms of the last spicey_run_mc's scalars and reduction, and of its draw, measured with HIP events. */
double spicey_last_tran_mc_ms(SpiceyHandle *h);
double spicey_last_tran_mc_draw_ms(SpiceyHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Sensitivities and corners of transient measurements: a deterministic design in the place of the Monte Carlo draw.  The
 * n_inst instances of ONE transient are the variants of one topology; the passes of spicey_run_reduced measure them, the scalar
 * programs above turn the rows into x [n_inst][n_scalar], and a reduction ACROSS the instances forms central differences.
 * Fixed operation order (tran_sens_exec.h), no FMA contraction, no atomics: the CPU and the device agree on every bit.
 *
 * The design writes v' = v g (one product; resistors in ohms) for every element e of the nE = nR + nC + nL, order R, C, L:
 *   SPICEY_TS_ONE_AT_A_TIME   act [nA] strictly ascending element indices, step [nA] finite in (0, 1); n_inst = 1 + 2 nA.
 *                             Instance 0 is nominal; instance 1 + 2a has element act[a] at g = 1.0 + step[a], instance 2 + 2a
 *                             has it at g = 1.0 - step[a]; every other g is 1.0.
 *   SPICEY_TS_LEVELS          lvl [n_inst][nE] int8 in {-1, 0, +1}, tol [nE] finite in [0, 1): g = 1.0 + (double)lvl tol[e].
 *
 * The reduction, one wave per scalar j, lane l the elements a = l, l + 64, ...; with x0 = x[0][j], xp = x[1 + 2a][j],
 * xm = x[2 + 2a][j], h = step[a], t = tol_act[a] (the tolerance of element act[a]), every operation rounded on its own:
 *   d = (xp - xm) / (2.0 h)    c = ((xp - x0) + (xm - x0)) / (h h)    sign = +1 if d > 0, -1 if d < 0, else 0
 * An element is a number iff its three instances are valid, none of x0, xp, xm is NaN and neither d nor c is NaN; otherwise
 * d = c = 0x7ff8000000000000 and sign = 0.
 *   d_sens  [n_scalar][nA][2]   {d, c}
 *   d_sign  [n_scalar][nA]      int8
 *   d_bound [n_scalar][8]       {x0, wc, rss2, n_num, a_max, contrib_max, n_interior, 0}: wc = sum |d| t and
 *                               rss2 = sum (d t) (d t) over the numbers, lane l adding its elements in ascending a from +0.0
 *                               and the partials meeting by s[l] += s[l + stride], stride 32 .. 1; n_num the numbers;
 *                               a_max the lowest a with the largest |d| t (-1 without a number) and contrib_max that
 *                               product (+0.0 without); n_interior = #{a : |d| < |c| t}, the elements whose fitted parabola
 *                               has its vertex inside the tolerance interval.  x0 is NaN if instance 0 is invalid.
 * Counts and indices are doubles.  No square root runs on the device. */
#define SPICEY_TS_ONE_AT_A_TIME 0
#define SPICEY_TS_LEVELS 1
typedef struct SpiceyTranSensReq {
  int64_t struct_bytes;
  int32_t mode;              /* SPICEY_TS_ONE_AT_A_TIME or SPICEY_TS_LEVELS */
  int32_t nA;                /* ONE_AT_A_TIME: the active elements (>= 1); LEVELS: 0 */
  int64_t reserved[2];       /* 0 */
} SpiceyTranSensReq;         /* 32 bytes */
/* Bytes of device workspace that serve spicey_tran_sens_design_device (either mode) and spicey_tran_sens_reduce_device alike;
 * -1 for arguments no launch accepts (n_inst < 1 or > 16384, n_scalar < 1, nE < 1, nA < 0). */
int64_t spicey_tran_sens_workspace_bytes(int32_t n_inst, int32_t n_scalar, int32_t nE, int32_t nA);
/* The design alone on any DEVICE buffers ([n_inst][n<kind>] each); req, act, step (ONE_AT_A_TIME) or lvl, tol (LEVELS) are HOST
 * data.  Needs no handle; enqueued on `stream` without synchronising.  Refusals are SPICEY_ERR_BAD_DESC with a text starting
 * "tran sens: " in spicey_last_error(NULL), nothing launched: a null request, struct_bytes, a nonzero reserved word, an unknown
 * mode; n_inst < 1 or > 16384; negative counts or no element; ONE_AT_A_TIME with nA < 1, n_inst != 1 + 2 nA, act not strictly
 * ascending or outside [0, nE), a step that is not finite or outside (0, 1); LEVELS with nA != 0, a tolerance that is negative,
 * >= 1 or not finite, a level outside {-1, 0, 1}; a null buffer; a workspace that is too small. */
int32_t spicey_tran_sens_design_device(int32_t device, int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C,
                                       const double *d_L, const SpiceyTranSensReq *req, const int32_t *act, const double *step, const int8_t *lvl,
                                       const double *tol, double *d_R_out, double *d_C_out, double *d_L_out, void *d_work, int64_t work_bytes, void *stream);
/* The scalars (the kernel and the judge of spicey_tran_mc_reduce_device) and the reduction alone on any DEVICE row buffers:
 * rows [3], scalars [n_scalar], valid [n_inst] (bytes, NULL: all), step [nA] and tol_act [nA] are HOST data; d_x
 * [n_inst][n_scalar], d_sens, d_sign and d_bound as above.  Enqueued on `stream` without synchronising.  SPICEY_ERR_BAD_DESC,
 * text starting "tran sens: ", nothing launched, for: everything the scalar judge refuses; nA < 1 or n_inst != 1 + 2 nA; a step
 * outside (0, 1) or not finite; a tolerance negative, >= 1 or not finite; a null buffer; a workspace that is too small. */
int32_t spicey_tran_sens_reduce_device(int32_t device, int32_t n_inst, const SpiceyMcRows *rows, const SpiceyMcScalar *scalars, int32_t n_scalar,
                                       const uint8_t *valid, const double *step, const double *tol_act, int32_t nA, double *d_x, double *d_sens,
                                       int8_t *d_sign, double *d_bound, void *d_work, int64_t work_bytes, void *stream);
/* A sensitivity run on the handle, whose n_inst = 1 + 2 req->nA instances are the variants and whose value rows are their
 * nominal values.  Everything is judged first (a refusal — SPICEY_ERR_BAD_DESC, text starting "tran sens: " in
 * spicey_last_error(h) — runs nothing); the ONE_AT_A_TIME design writes scratch value arrays (the handle's own are never
 * written); ONE transient, exactly that of spicey_run_reduced, reads them; the passes of `lists` run behind it and their rows
 * stay on the device (the result pointers of `lists` are ignored); an instance is valid iff its spicey_last_inst_status entry
 * is 0; the scalars and the reduction run, and sens [n_scalar][nA][2], sign [n_scalar][nA], bound [n_scalar][8], x
 * [n_inst][n_scalar] (or NULL) and iters (or NULL) come back; the tolerance of active element a is tol[act[a]].  If instance 0
 * is invalid nothing is reduced and the outputs are untouched.  The fourier, spectrum and values lists are refused.  The return
 * value, the end state and spicey_last_inst_status are as after spicey_run_reduced of the variants; a later plain run binds the
 * handle's own arrays and gives the bits it gave before.  act, step, tol [nE] and scalars are HOST arrays. */
int32_t spicey_run_sens(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *lists,
                        const SpiceyTranSensReq *req, const int32_t *act, const double *step, const double *tol, const SpiceyMcScalar *scalars,
                        int32_t n_scalar, double *sens, int8_t *sign, double *bound, double *x, int32_t *iters);
/* The same with the LEVELS design: lvl [n_inst][nE] and tol [nE] are HOST arrays; only x [n_inst][n_scalar] comes back, the
 * NaN 0x7ff8000000000000 for an invalid instance.  With no valid instance nothing is written. */
int32_t spicey_run_levels(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *lists,
                          const SpiceyTranSensReq *req, const int8_t *lvl, const double *tol, const SpiceyMcScalar *scalars, int32_t n_scalar,
                          double *x, int32_t *iters);
/* Duration in ms of the last spicey_run_sens's / spicey_run_levels's scalars and reduction, and of its design, measured with
 * HIP events. */
double spicey_last_tran_sens_ms(SpiceyHandle *h);
double spicey_last_tran_sens_design_ms(SpiceyHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Periodic steady state by shooting Newton: a design over the STATE of the instances and a dense Newton update on the device.
 * The state of one circuit is x = [C_vprev | L_iprev | D_vdprev], nX = nC + nL + nD; S_ison is carried, not differentiated.  The
 * n_inst = n_ckt W instances of ONE transient over one period — W = 1 + nX (SPICEY_PSS_NEWTON) or 1 (SPICEY_PSS_SETTLE),
 * instance c W + j belongs to circuit c, j = 0 nominal, j = 1 + a with entry a perturbed — give the period map and its finite
 * differences.  Fixed operation order (pss_exec.h), no FMA contraction, no atomics: the CPU and the device agree on every bit.
 *
 * The design writes the instances' state arrays: s[c][j][a] = base[c][a], and for j == 1 + a the value
 * sp = base[c][a] + rel_step max(|base[c][a]|, scale) with scale = v_scale (C, D entries) or i_scale (L entries), and
 * h_eff[c][a] = sp - base[c][a]; every instance of circuit c gets base_on[c] as S_ison.
 *
 * The update, one 256-thread workgroup per circuit whose done[c] is 0, on the instances' END states e_j (e0 the nominal's):
 *   r = e0 - base; res = max_a |r_a| / (reltol max(|base_a|, |e0_a|) + abstol), abstol = vabstol (C, D) or iabstol (L)
 *   converged: res <= 1 and the nominal's end S_ison equals base_on[c]: done[c] = 1, the base stays, status 0
 *   M[i][a] = (i == a) - (e_{1+a}[i] - e0[i]) / h_eff[a]; Gaussian elimination with partial pivoting, the LOWEST row of the
 *   largest magnitude as pivot (|pivot| < 1e-12: status 3), column-oriented back substitution, every product, quotient and
 *   difference rounded on its own; base[c] += damping d, base_on[c] = the nominal's end S_ison.  SETTLE: base[c] = e0, d = r.
 *   rows [n_ckt][8] = {res, step, n_switch_mismatch, status, a_res, min |pivot|, n_pert_switch_diff, converged}: step the
 *   scaled max-norm of d, max_a |d_a| / (reltol |base_a| + abstol); a_res the lowest entry of the largest residual; min |pivot|
 *   -1 when no pivot was taken; n_pert_switch_diff the perturbed instances whose end S_ison differs from the nominal's (the
 *   Jacobian is noisy then).  Status: 0 converged, 1 moved, 2 the nominal's run was singular, 3 singular Jacobian, 4 a value
 *   that is not finite or a singular perturbed instance, 5 stopped by another circuit's failure.  A status >= 2 leaves the
 *   base as it is and writes itself into done[c]: the circuit is frozen.  nX <= 128 with NEWTON: the matrix lives in LDS. */
#define SPICEY_PSS_NEWTON 0
#define SPICEY_PSS_SETTLE 1
#define SPICEY_PSS_ROW 8
typedef struct SpiceyPssReq {
  int64_t struct_bytes;
  int32_t n_ckt;             /* circuits; the instances are n_ckt W */
  int32_t method;            /* SPICEY_PSS_NEWTON or SPICEY_PSS_SETTLE */
  int32_t max_iter;          /* spicey_run_pss: Newton iterations at most (>= 1) */
  int32_t pad;               /* 0 */
  double damping;            /* a fixed factor in (0, 1] */
  double reltol, vabstol, iabstol; /* > 0 */
  double rel_step, v_scale, i_scale; /* > 0 */
  int64_t reserved;          /* 0 */
} SpiceyPssReq;              /* 88 bytes */
/* Bytes of device workspace of spicey_pss_design_device and spicey_pss_update_device; -1 for arguments no launch accepts
 * (n_ckt < 1, nX < 1, nX > 128 with NEWTON, an unknown method, more than 2^31 - 1 state entries). */
int64_t spicey_pss_workspace_bytes(int32_t n_ckt, int32_t nX, int32_t method);
/* The design alone on any DEVICE buffers: d_base [n_ckt][nX], d_base_on [n_ckt][nS], d_h [n_ckt][nX] (written; NEWTON), the
 * state arrays d_Cv / d_Li / d_Dv / d_Son [n_inst][n<kind>] (written; NULL where the count is 0).  perturb = 0 writes the base
 * into every instance and leaves d_h alone.  req is HOST data.  Needs no handle; enqueued on `stream` without synchronising.
 * Refusals are SPICEY_ERR_BAD_DESC with a text starting "pss: " in spicey_last_error(NULL), nothing launched: a null request,
 * struct_bytes, nonzero pad or reserved, an unknown method, n_ckt < 1, negative counts, nX = 0, nX > 128 with NEWTON (the text
 * names method = "settle"), tolerances, steps or scales that are not > 0 and finite, damping outside (0, 1], a null buffer, a
 * workspace that is too small. */
int32_t spicey_pss_design_device(int32_t device, int32_t nC, int32_t nL, int32_t nD, int32_t nS, const SpiceyPssReq *req, int32_t perturb,
                                 const double *d_base, const int32_t *d_base_on, double *d_h, double *d_Cv, double *d_Li, double *d_Dv, int32_t *d_Son,
                                 void *d_work, int64_t work_bytes, void *stream);
/* The update alone on any DEVICE buffers: the state arrays hold the END states; inst_status [n_inst] (HOST; NULL: all 0) the
 * instances' spicey_last_inst_status; d_base, d_base_on, d_delta [n_ckt][nX] (or NULL), d_rows [n_ckt][8] and d_done [n_ckt]
 * are written as above.  The same refusals. */
int32_t spicey_pss_update_device(int32_t device, int32_t nC, int32_t nL, int32_t nD, int32_t nS, const SpiceyPssReq *req, const int32_t *inst_status,
                                 double *d_base, int32_t *d_base_on, const double *d_h, const double *d_Cv, const double *d_Li, const double *d_Dv,
                                 const int32_t *d_Son, double *d_delta, double *d_rows, int32_t *d_done, void *d_work, int64_t work_bytes, void *stream);
/* The shooting-Newton loop on the handle, whose n_inst = req->n_ckt W instances are the circuits' nominal and perturbed copies and
 * whose source table holds the m_steps rows of ONE period (per instance with src_per_inst = 1).  The base starts as instance
 * c W's current state.  Per iteration: the design into the handle's own state arrays; one transient of m_steps - 1 steps from
 * them, exactly that of spicey_run_device_src, into scratch outputs of this call; the update on the end states with the
 * instances' spicey_last_inst_status; the [n_ckt][8] rows into history [max_iter][n_ckt][8] (a circuit that is done keeps its
 * last row; iterations that did not run are not written).  The loop stops when every circuit is done or at max_iter.
 * x [n_ckt][nX], on [n_ckt][nS] (NULL with nS = 0): the base on return; n_iter [n_ckt]: the updates the circuit took part in;
 * status [n_ckt]: 0 converged, 1 max_iter reached, 2 the nominal's own solve was singular, 3 singular Jacobian, 4 a value that
 * is not finite or a singular perturbed instance, 5 stopped by another circuit's failure in its workgroup.  A circuit with a
 * status >= 2 is frozen, the others go on.  On return every instance of circuit c holds base[c] and base_on[c], so
 * spicey_get_state is defined.  Returns SPICEY_OK unless a launch failed or the arguments are refused: SPICEY_ERR_BAD_DESC, text
 * starting "pss: " in spicey_last_error(h), nothing run, the handle as it was — null buffers, n_inst != n_ckt W, nX = 0,
 * nX > 128 with NEWTON, m_steps < 1, max_iter < 1, tolerances, steps or scales that are not > 0, damping outside (0, 1], a
 * wrong struct_bytes, src_per_inst outside {0, 1}.  Every engine of spicey_create is served. */
int32_t spicey_run_pss(SpiceyHandle *h, int64_t m_steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyPssReq *req, double *x,
                       int32_t *on, double *history, int32_t *n_iter, int32_t *status);
/* Duration in ms of the last spicey_run_pss's designs and updates, and of its transients' kernels, each summed over the
 * iterations, measured with HIP events. */
double spicey_last_pss_ms(SpiceyHandle *h);
double spicey_last_pss_tran_ms(SpiceyHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Sizing elements to measured goals: a damped least-squares (Levenberg-Marquardt) loop over element GAINS, updated on the device.
 * One handle holds n_ckt circuits of one topology, independent problems; each has W = 1 + 2 nA instances — instance c W nominal,
 * c W + 1 + 2a with active element a at +h_a, c W + 2 + 2a at -h_a — the one-at-a-time design of spicey_run_sens per circuit.
 * act [nA] are strictly ascending element indices in the order R, C, L; the unknowns are g [n_ckt][nA], factors on the
 * handle's own values (a resistor stays in ohms).  Fixed operation order (fit_exec.h), no FMA contraction, no atomics, no exp,
 * log or sqrt: the CPU and the device agree on every bit.
 *
 * The design writes v' = v for an inactive element, v' = v (g_a (1.0 + h_a)) or v (g_a (1.0 - h_a)) for the active element of
 * a perturbed instance and v' = v g_a otherwise, every product rounded on its own.
 *
 * The update, one 256-thread workgroup per circuit whose done[c] is 0, on x [n_inst][n_scalar] (the scalars of spicey_run_mc's
 * programs), the instances' validity and goals [n_ckt][n_scalar]:
 *   r_j = w_j (x0_j - lo_j) for EQ, else w_j times the amount by which x0_j exceeds its bound (negative below lo), else +0.0;
 *   goal j is active iff it is EQ or r_j != 0; F = sum_j r_j r_j in ascending j from +0.0; an invalid nominal or a NaN x0_j makes
 *   the point not evaluable, F = +inf.
 *   accept iff first and F is finite, or not first and F < F_good: J[j][a] = w_j ((x+_j - x-_j) / (2.0 h_a)) over the active j — a
 *   column with an invalid instance or a NaN entry is frozen: zeroed, counted —, A = J^T J, b = -(J^T r), g_good = g, F_good = F,
 *   all kept in the workspace; lambda = lambda0 (first) or lambda lam_down.  An accepted F <= f_tol converges without a solve.
 *   reject: lambda = lambda lam_up, the step is solved again from the kept A and b; lambda > lam_max: status 5.
 *   solve M d = b, M = A with M[a][a] = A[a][a] + lambda A[a][a] (a zero diagonal becomes 1.0): Gaussian elimination with partial
 *   pivoting, the LOWEST row of the largest magnitude as pivot (|pivot| < pivot_min: status 3), column-oriented back substitution.
 *   d_a is clamped to +-max_step; an accepted point with max|d| <= x_tol converges; else g_a = g_good_a (1.0 + d_a), clamped to
 *   [g_lo_a, g_hi_a].  With every status but 1, g[c] = g_good[c]: the gains always belong to a point that was evaluated.
 *   rows [n_ckt][8] = {F, F_good, lambda, accepted, status, max|d|, n_frozen, n_clamped}.  Status: 0 converged (done[c] = 1),
 *   1 moved, 2 the first nominal is not evaluable, 3 singular system, 4 a value that is not finite, 5 stalled; a status >= 2
 *   writes itself into done[c]: the circuit is frozen, the others go on.  nA <= 128: the matrix lives in LDS (132 096 bytes). */
#define SPICEY_FIT_EQ 0
#define SPICEY_FIT_AT_MOST 1
#define SPICEY_FIT_AT_LEAST 2
#define SPICEY_FIT_BETWEEN 3
#define SPICEY_FIT_ROW 8
typedef struct SpiceyFitReq {
  int64_t struct_bytes;
  int32_t n_ckt;             /* circuits; the instances are n_ckt (1 + 2 nA) */
  int32_t nA;                /* active elements, 1 .. 128 */
  int32_t max_iter;          /* spicey_run_fit: updates at most (>= 1) */
  int32_t pad;               /* 0 */
  double lambda0;            /* >= 0 */
  double lam_up, lam_down;   /* > 1; in (0, 1] */
  double lam_max;            /* >= lambda0 */
  double max_step;           /* > 0: the largest relative change of a gain in one step */
  double x_tol, f_tol;       /* >= 0 */
  double pivot_min;          /* > 0 */
  int64_t reserved;          /* 0 */
} SpiceyFitReq;              /* 96 bytes */
typedef struct SpiceyFitGoal {
  int32_t kind, pad;         /* SPICEY_FIT_*; 0 */
  double lo, hi;             /* EQ: lo is the target; AT_MOST: hi; AT_LEAST: lo; BETWEEN: lo <= hi */
  double weight;             /* finite, > 0 */
} SpiceyFitGoal;             /* 32 bytes */
/* Bytes of device workspace of spicey_fit_design_device and spicey_fit_update_device; -1 for arguments no launch accepts
 * (n_ckt < 1, nA outside 1 .. 128, n_ckt (1 + 2 nA) > 16384, n_scalar < 1).  The workspace carries A, b, g_good, F_good
 * and lambda from one update to the next: the same buffer serves the whole loop. */
int64_t spicey_fit_workspace_bytes(int32_t n_ckt, int32_t nA, int32_t n_scalar);
/* The design alone on any DEVICE buffers: d_R / d_C / d_L [n_inst][n<kind>] the nominal values, d_g [n_ckt][nA], the outputs
 * d_*_out of the same shapes (NULL where the count is 0).  req, act [nA] and step [nA] are HOST data.  Needs no handle; enqueued
 * on `stream` without synchronising.  Refusals are SPICEY_ERR_BAD_DESC with a text starting "fit: " in spicey_last_error(NULL),
 * nothing launched: a null request, struct_bytes, nonzero pad or reserved, n_ckt < 1, nA outside 1 .. 128, more than 16384
 * instances, active elements out of range or not strictly ascending, steps outside (0, 1), a null buffer, a workspace that is
 * too small; the update's also n_scalar < 1, bounds that are not 0 < g_lo <= g_hi finite, a weight that is not finite and > 0, an
 * unknown goal kind, a bound that is not finite or lo > hi, lam_down outside (0, 1], lam_up <= 1, the other numbers of the request. */
int32_t spicey_fit_design_device(int32_t device, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C, const double *d_L,
                                 const SpiceyFitReq *req, const int32_t *act, const double *step, const double *d_g, double *d_R_out, double *d_C_out,
                                 double *d_L_out, void *d_work, int64_t work_bytes, void *stream);
/* The update alone on any DEVICE buffers: d_x [n_inst][n_scalar], d_g [n_ckt][nA], d_rows [n_ckt][8] and d_done [n_ckt] are
 * written as above; first != 0 marks the circuits' first update.  step [nA], g_lo / g_hi [n_ckt][nA], goals [n_ckt][n_scalar]
 * and valid [n_inst] (bytes; NULL: every instance is valid) are HOST data.  The same refusals. */
int32_t spicey_fit_update_device(int32_t device, const SpiceyFitReq *req, int32_t n_scalar, int32_t first, const double *step, const double *g_lo,
                                 const double *g_hi, const SpiceyFitGoal *goals, const uint8_t *valid, const double *d_x, double *d_g, double *d_rows,
                                 int32_t *d_done, void *d_work, int64_t work_bytes, void *stream);
/* The loop on the handle, whose n_inst = req->n_ckt (1 + 2 nA) instances are the circuits' nominal and perturbed copies.  The
 * handle's state at entry is kept; per iteration it is restored, the design goes into scratch value arrays of this call, ONE
 * transient bound to them runs exactly as under spicey_run_sens, the measure / timing / power passes of `lists` leave their rows
 * on the device, the scalar programs (spicey_run_mc's) turn them into x, and the update runs; only the [n_ckt][8] rows and the
 * done flags come back, into history [max_iter][n_ckt][8] (a circuit that is done keeps its last row; iterations that did not
 * run are not written).  The loop stops when every circuit is done or at max_iter.  g0 [n_ckt][nA] are the starting gains.
 * On return g [n_ckt][nA] and F [n_ckt] are the best evaluated point, x [n_ckt][n_scalar] (or NULL) the nominals' scalars there,
 * n_iter [n_ckt] the updates the circuit took part in, status [n_ckt]: 0 converged, 1 max_iter reached, 2 the first nominal
 * not evaluable, 3 singular system, 4 a value that is not finite, 5 stalled.  The handle's own values are untouched and its
 * state is the state at entry: a later plain run gives the bits it gave before.  The fourier, spectrum and values lists are
 * refused.  A matrix that is singular by its structure gives every circuit status 2 and SPICEY_OK, nothing run, as
 * spicey_run_pss does.  A launch or a transient that fails ends the call with its error and the outputs as far as they were
 * written; the handle's state is the state at entry then too.  Refusals: SPICEY_ERR_BAD_DESC, text starting "fit: " in
 * spicey_last_error(h), nothing run — the request's numbers, max_iter < 1, null buffers, n_inst != n_ckt (1 + 2 nA), a
 * starting gain that is not finite and > 0, and the design's, the update's, the lists' and the scalars' own. */
int32_t spicey_run_fit(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *lists,
                       const SpiceyFitReq *req, const int32_t *act, const double *step, const double *g_lo, const double *g_hi, const double *g0,
                       const SpiceyFitGoal *goals, const SpiceyMcScalar *scalars, int32_t n_scalar, double *g, double *F, double *history,
                       int32_t *n_iter, int32_t *status, double *x, int32_t *iters);
/* Duration in ms of the last spicey_run_fit's designs and updates, and of its transients' kernels, each summed over the
 * iterations, measured with HIP events. */
double spicey_last_fit_ms(SpiceyHandle *h);
double spicey_last_fit_tran_ms(SpiceyHandle *h);

/* ---------------------------------------------------------------------------------------------------------------
 * Result formatting fast path (host code, no GPU): the CSV text of
 *   formatTranResult(tran)       /root/reference/lib/formatting/formatTranResult.ts:1-23
 * straight from the typed arrays spicey_run filled.  Every number is Number.prototype.toPrecision(6) exactly as
 * ECMA-262 defines it (ties to the larger digit string, exponential notation for e < -6 or e >= 6).
 *   times    [n_points]
 *   values   [n_points][stride]; series j is column cols[j] (the caller applies the JS key order / probe filter)
 *   header   first line, e.g. "t(s), 1:V, 2:V"
 * Returns the byte length of the text (lines joined by "\n", no trailing newline) and writes it when out_cap
 * suffices (call with out = NULL to size the buffer); -1 on bad arguments. */
int64_t spicey_format_tran(int64_t n_points, int32_t n_series, const double *times, const double *values, int64_t stride,
                           const int32_t *cols, const char *header, char *out, int64_t out_cap);
/* toPrecision(6) of one double into dst (>= 32 bytes, not NUL-terminated); returns the length. */
int32_t spicey_to_precision6(double x, char *dst32);

#ifdef __cplusplus
}
#endif
#endif /* SPICEY_HIP_H */
