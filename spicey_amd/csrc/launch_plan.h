// launch_plan.h — the launch plan of a transient handle (every shape decision of spicey_create) and the shape helpers it
// reads.  No HIP header: the emulator library and the CPU tests run the very policy the product runs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/spicey_hip.h"
#include "program.h"
#include "symbolic.h"
#include "tran_pt_layout.h"

#define SPICEY_LDS_MAX 163840  // 160 KiB per CU on MI355X (MI355X_MICROARCH.md "Chip-level parameters")

size_t spicey_lds_bytes(const SpiceyProg &P, int K, bool lds, int tail_n = 0);
size_t spicey_front_lds_bytes(const SpiceyProg &P);
size_t spicey_gw_doubles_per_wg(const SpiceyProg &P, int K);

// v2 builds (register-resident program, one instance per workgroup).  MINW (waves per SIMD the register budget is cut
// for) is chosen so that NO variant spills: ROCm 7.2's hipcc places spill stores of values defined in divergent loops
// where EXEC can be zero (the store is lost and a later reload returns a previous kernel's scratch) — observed as stale
// vPrev registers; the Makefile therefore fails the build if any kernel reports a non-zero ScratchSize.
//   T <= 256 : 28 slots, 12 entries, 4 elements per thread (one wave per SIMD, 256 VGPRs, no spills to AGPRs)
//   (K = 2 interleaved instances: every variant tried — 16 to 32 slots — spilled 9 vector registers to AGPRs; the 16-bit
//   interpreter is therefore built for K = 1 only and interleaved instances run on interpreter 1)
//   T <= 512 : 16 slots,  8 entries, 2 elements per thread (<= 256 VGPRs)
//   T <= 1024:  8 slots,  4 entries, 1 element  per thread (<= 128 VGPRs)
// `packed` = the two-workgroups-per-CU geometry: 512 threads, <= 128 VGPRs; only 4 slots stay resident.  A streamed phase
// costs an exposed L2 round trip per solve whatever its size, so spicey_build_resident fills the slots for the fewest
// streamed PHASES (chunks go wherever slots are free, a level as row records where two slots of a wave are): on the
// 1000-node chains only the widest factor level is streamed, with the next record fetched behind the one at hand.
// Hybrid workspace: 512 threads as the plain build, or 1024 threads with 4 slots (with 8 the build spills 10 registers
// at the 128-register cap).
// `fresh` = the packed build for FRESH-FILL programs (program.h: nKeep): phase B restores the kept entries only, two per
// thread, both with a dynamic-stamp descriptor — 8 vector registers fewer than the 6-entry packed build, which pay for
// keeping the first streamed record of factor level 0 in flight under B (tran_exec.h).  spicey_plan takes it, with a
// program built with fresh_fill, where the kept and the dynamic entries fit 2 x 512 and the circuit is not linear (a
// linear circuit reuses the factors of step 0: B re-stamps nothing after it, so there is nothing to save, and the
// build's few extra instructions per record showed as -1.7 % on rc_ladder(1000) x 512); otherwise the 6-entry build.
#define SPICEY_V2_RMAX256 28  // (32 slots spilled 6 vector registers to AGPRs: refused by check_no_spills.py)
struct SpiceyV2Shape {
  bool packed, hybrid;
  int threads, rmax, nsv, nel, minw;  // workgroup size (launch bound), slots, re-stamped entries and elements per thread, waves per SIMD
  bool fresh = false;
  bool early = false;  // the shape also has early-prefetch kernels (tran_v2_run.h: EP), which a handle takes unless SPICEY_NO_EARLY_PREFETCH is set
  bool slots = false;  // ... and an operand-slot kernel (tran_v2_phases.h: OS), taken where the slots fit unless SPICEY_NO_OPERAND_SLOTS is set
  bool ready = false;  // ... and that kernel's ready-argument form (tran_v2_run.h: RA), taken by an operand-slot run unless SPICEY_NO_READY_ARGS is set
  bool addr = false;   // ... and that form with operand addresses (tran_v2_run.h: OA), taken by a ready-argument run where spicey_addr_fits holds unless SPICEY_NO_OPERAND_ADDR is set
  bool top_regs = false;  // ... and that one with the register-exchange top (tran_v2_run.h: TR), taken by an operand-address run whose top has 1 .. 6 stages unless SPICEY_NO_TOP_REGS is set
  bool u0_resident = false;  // ... and that one with the resident level-0 record (tran_v2_run.h: UR), taken by a register-exchange-top run where spicey_u0_resident_fits holds unless SPICEY_NO_U0_RESIDENT is set
  bool top_fold = false;  // ... and that one with the last factor level folded into the top (tran_v2_run.h: TF), taken by a resident-record run where spicey_top_fold_table holds unless SPICEY_NO_TOP_FOLD is set
  bool stamp_fuse = false;  // ... and that one whose Z stamps the next step, with no phase B in the time loop (tran_v2_run.h: SF), taken by a folded run where spicey_stamp_fuse_table holds unless SPICEY_NO_STAMP_FUSE is set
  bool fixed_schedule = false;  // ... and that one with the time loop written out for what the plan holds (tran_v2_run.h: FS), taken by a fused run where spicey_fixed_schedule_fits holds unless SPICEY_NO_FIXED_SCHEDULE is set
};
// `early`: Z's element parameters come from one record per thread (SpiceyRun::zpar) and are fetched, with the next source
// value, at the tail of the last factor phase.  The fresh packed build has it; the other builds were left as they are.
// (spicey_launch_tran_v2 instantiates one kernel per entry; each kind in ascending threads)
constexpr SpiceyV2Shape SPICEY_V2_SHAPES[] = {{true, false, 512, 4, 6, 2, 4},    {true, false, 512, 4, 2, 2, 4, true, true, true, true, true, true, true, true, true, true},
                                              {false, true, 512, 16, 8, 2, 2},   {false, true, 1024, 4, 4, 1, 4},
                                              {false, false, 256, SPICEY_V2_RMAX256, 12, 4, 1},
                                              {false, false, 512, 16, 8, 2, 2},  {false, false, 1024, 8, 4, 1, 4}};
constexpr int SPICEY_V2_NSHAPES = (int)(sizeof(SPICEY_V2_SHAPES) / sizeof(SPICEY_V2_SHAPES[0]));
// index of the build that runs `threads` threads: the first of the kind that holds them; -1 = none
int spicey_v2_shape(int threads, bool packed, bool hybrid, bool fresh = false);
// stages of the tridiagonal top of `pcr_n` rows, S = ceil(log2 pcr_n) (spicey_tran_run_v2 forms the same number): the
// unrolled top, and with it its register-exchange form, runs S = 1 .. 6, i.e. 2 .. 64 rows
inline int spicey_top_stages(int pcr_n) {
  int S = 0;
  while ((1 << S) < pcr_n) S++;
  return S;
}

// Environment knobs of the transient handle, read once by spicey_create.
struct SpiceyKnobs {
  bool no_hybrid = false;            // SPICEY_NO_HYBRID: never take the hybrid workspace
  bool front_right_looking = false;  // SPICEY_FRONT_RIGHT_LOOKING: experiments, the round-2 sweep of staged fronts
  bool force_group_abort = false;    // SPICEY_TEST_FORCE_GROUP_ABORT: tests, the first attempt of every group launch aborts
  int group_timeout_ms = 0;          // SPICEY_GROUP_TIMEOUT_MS: group-mode wait bound when SpiceyOptions leaves it 0
  bool no_phase_table = false;       // SPICEY_NO_PHASE_TABLE: the 16-bit interpreter fetches its phase arguments by scalar loads in every phase (tran_exec.h)
  bool no_fresh_fill = false;        // SPICEY_NO_FRESH_FILL: the packed geometry keeps the default program and the 6-entry build (the in-library A/B switch)
  bool fresh_fill_linear = false;    // SPICEY_FRESH_FILL_LINEAR: tests, a linear circuit (factor reuse) takes the fresh build too
  bool no_early_prefetch = false;    // SPICEY_NO_EARLY_PREFETCH: a shape with early-prefetch kernels keeps its plain build and the handle no parameter record (the in-library A/B switch)
  bool no_operand_slots = false;     // SPICEY_NO_OPERAND_SLOTS: an early-prefetch run keeps the kernel that masks ground by compare and select and writes no slot (the in-library A/B switch)
  bool no_ready_args = false;        // SPICEY_NO_READY_ARGS: an operand-slot run keeps the kernel that moves all of Z's arguments to scalars at the phase head (the in-library A/B switch)
  bool no_operand_addr = false;      // SPICEY_NO_OPERAND_ADDR: a ready-argument run keeps the kernel that addresses its LDS operands as W[field] (the in-library A/B switch)
  bool no_top_regs = false;          // SPICEY_NO_TOP_REGS: an operand-address run keeps the kernel whose tridiagonal top exchanges its rows through LDS (the in-library A/B switch)
  bool no_u0_resident = false;       // SPICEY_NO_U0_RESIDENT: a register-exchange-top run keeps the kernel that fetches level 0's row record in every step (the in-library A/B switch)
  bool no_top_fold = false;          // SPICEY_NO_TOP_FOLD: a resident-record run keeps the kernel that runs the last factor level as a phase of its own (the in-library A/B switch)
  bool no_stamp_fuse = false;        // SPICEY_NO_STAMP_FUSE: a folded run keeps the kernel that stamps in a phase B of its own (the in-library A/B switch)
  bool no_fixed_schedule = false;    // SPICEY_NO_FIXED_SCHEDULE: a fused run keeps the kernel whose time loop decides its schedule in every step (the in-library A/B switch)
};
SpiceyKnobs spicey_read_knobs();

// What the plan asks of the device: `open` runs once the descriptor is validated (select device `device`, report its CU
// count, or an error code and message); `grp_blocks_per_cu` is the group kernel's occupancy (spicey_grp_blocks_per_cu).
struct PlanDevice {
  std::function<int32_t(int device, int *ncu, std::string &err)> open;
  std::function<int(const SpiceyProg &P, int K, int threads)> grp_blocks_per_cu;
};

// Reference-order engine (SpiceyOptions.interpreter = 3, exact_exec.h): the per-instance workspace, offsets in doubles
// from its base (the int32 arrays start at a double boundary).  A | b is n rows of stride ld (n + 1 padded to an odd
// count: column reads of the pivot search stay off one LDS bank); q = the stamp quantities of one iteration (R 1/R | C Gc
// | C Ieq | L Gl | L iPrev | S 1/R | V source | D gd | D ieq | 1.0), slot offsets of each kind below.
struct SpiceyExactWs {
  int32_t ld, mw;  // row stride of A | b; 32-bit words of one row's nonzero-column mask
  int32_t nq, qR, qGc, qIc, qGl, qIl, qS, qV, qGd, qIeq, qOne;
  int64_t A, x, q, vdlin, act_f, perm, act_r, mask, doubles;
};
SpiceyExactWs spicey_exact_ws(const SpiceyDesc &d);
#define SPICEY_EXACT_STATIC_LDS 256  // bytes of static LDS of the exact kernel (reduction scratch, counters)

// Reference-order AC engine (spicey_ac_create with interpreter = 3, ac_exact_exec.h): the workspace of one (instance,
// frequency) slot, offsets in complex (16-byte) units from its base.  A | b is n rows of stride ld (n + 1 padded to an
// odd count); q = the stamp quantities of one frequency (R 1/R | C jwC | L 1/(jwL) | V phasor | (1, 0)); f = the
// multipliers of the active rows; perm and the active rows' indices are int32 arrays.
struct SpiceyAcExactWs {
  int32_t ld, nq, qR, qC, qL, qV, qOne;
  int64_t A, x, q, f, perm, act, cx;
};
SpiceyAcExactWs spicey_ac_exact_ws(const SpiceyDesc &d);
#define SPICEY_AC_EXACT_STATIC_LDS 256            // bytes of static LDS of the exact AC kernel (reduction scratch, counters)
#define SPICEY_AC_EXACT_SLAB_MAX ((int64_t)1 << 30)  // global slab of one launch: at most 1 GiB (a larger slot runs alone)

struct AcExactPlan {
  int T = 64;
  bool lds = true;       // workspace in LDS (else each slot's slab of a global buffer)
  size_t lds_bytes = 0;  // dynamic LDS per workgroup (0 on the slab)
  SpiceyAcExactWs ws{};
};
// Shape of an exact AC handle: validates the descriptor and the options it reads (threads, force_global).
int32_t spicey_ac_exact_plan(const SpiceyDesc *desc, const SpiceyOptions &opt, AcExactPlan &plan, std::string &err);
// slots (workgroups) per launch of a sweep over `slots` (instance, frequency) pairs
int64_t spicey_ac_exact_chunk(const AcExactPlan &plan, int64_t slots);

struct LaunchPlan {
  int n_inst = 0, K = 1, T = 256, grid = 1, interp = 1;
  int G = 1;             // workgroups per instance group (group mode: global workspace only)
  bool packed = false;   // two 512-thread workgroups per CU
  bool fresh = false;    // packed: hp is a fresh-fill program and runs on the fresh build (SPICEY_V2_SHAPES)
  bool early = false;    // the run takes the shape's early-prefetch kernel: the handle owns a parameter record (spicey_zpar_doubles)
  bool slots = false;    // ... in its operand-slot form: the two constants of tran_pt.h (spicey_slot_index) fit behind the phase table
  bool ready = false;    // ... with ready arguments (tran_v2_run.h: RA), for every run whose step count spicey_ready_steps_ok accepts: spicey_ready_run
  // the shape has an operand-address kernel (tran_v2_run.h: OA) and the program meets its conditions — K = 1, LDS workspace,
  // no hybrid layout, spicey_addr_fits — and SPICEY_NO_OPERAND_ADDR is not set: every ready-argument run of the handle takes
  // that kernel (spicey_addr_run).  A property of the program and its shape: the knobs of the forms below it (phase table,
  // early prefetch, operand slots, ready arguments) decide whether a ready-argument run happens, not this flag.
  bool addr = false;
  // ... and a form of that kernel with the register-exchange top (tran_v2_run.h: TR), the plan says `addr`, the program's top
  // has 1 .. 6 stages and SPICEY_NO_TOP_REGS is not set: every operand-address run of the handle takes it (spicey_top_regs_run)
  bool top_regs = false;
  // ... and a form of that kernel with the resident level-0 record (tran_v2_run.h: UR), where the plan says `top_regs`,
  // spicey_u0_resident_fits holds for the program and its resident layout and SPICEY_NO_U0_RESIDENT is not set: every
  // register-exchange-top run of the handle takes it (spicey_u0_resident_run)
  bool u0_resident = false;
  // ... and a form of that kernel with the last factor level folded into the top (tran_v2_run.h: TF), where the plan says
  // `u0_resident`, spicey_top_fold_table holds for the program and SPICEY_NO_TOP_FOLD is not set: every resident-record run
  // of the handle takes it (spicey_top_fold_run)
  bool top_fold = false;
  // ... and a form of that kernel whose Z stamps the next step (tran_v2_run.h: SF), where the plan says `top_fold`,
  // spicey_stamp_fuse_table holds for the program and SPICEY_NO_STAMP_FUSE is not set: every folded run of the handle takes
  // it (spicey_stamp_fuse_run)
  bool stamp_fuse = false;
  // ... and a form of that kernel with the time loop written out (tran_v2_run.h: FS), where the plan says `stamp_fuse`,
  // spicey_fixed_schedule_fits holds for the program and its resident layout, the handle asks for no empty diagnostics
  // phases and SPICEY_NO_FIXED_SCHEDULE is not set: every fused run of the handle takes it (spicey_fixed_schedule_run)
  bool fixed_schedule = false;
  bool lds = true;       // workspace in LDS (else global memory)
  size_t lds_bytes = 0;
  int64_t algo_bytes = 0;
  SpiceyExactWs xws{};   // interpreter 3 only
};

// Every decision of spicey_create, in its order and with its error codes and messages (err).  Builds hp (and, for the
// 16-bit interpreter, hres).
int32_t spicey_plan(const SpiceyDesc *desc, const SpiceyOptions &opt, const SpiceyKnobs &knobs, const PlanDevice &dev, HostProgram &hp,
                    HostResident &hres, LaunchPlan &plan, std::string &err);
// whether a run of `steps` steps on a planned handle takes the ready-argument kernel: the plan said so and the per-step
// offsets fit the 32 x 32 -> 64-bit product that kernel forms them with (tran_pt_layout.h); otherwise the operand-slot kernel
bool spicey_ready_run(const LaunchPlan &plan, int64_t steps);
// LaunchPlan::addr of a program with header `P` and `tail_n` tail levels on build `shape` (an index into SPICEY_V2_SHAPES,
// < 0: none) at K instances per workgroup, workspace in LDS or not: what spicey_plan decides, as a function of its own
bool spicey_plan_addr(const SpiceyProg &P, int tail_n, int K, bool lds, int shape, const SpiceyKnobs &knobs);
// ... and whether that run takes the kernel's operand-address form: a ready-argument run of a plan that says `addr`
bool spicey_addr_run(const LaunchPlan &plan, int64_t steps);
// LaunchPlan::top_regs of a plan whose `addr` is decided, for a top of `pcr_n` rows on build `shape`: what spicey_plan decides
bool spicey_plan_top_regs(bool addr, int pcr_n, int shape, const SpiceyKnobs &knobs);
// ... and whether that run takes the register-exchange top: an operand-address run of a plan that says `top_regs`
bool spicey_top_regs_run(const LaunchPlan &plan, int64_t steps);
// The resident level-0 record (tran_v2_run.h: UR) is for a program P with the phase descriptors st_desc (HostResident, [2L][8])
// on T threads where ALL of this holds — the kernel's phase 0 then runs the one record in each thread's registers and
// nothing else:
//   - factor phase 0 exists below the tridiagonal top and is streamed in its row-record encoding (st_desc[0] = 1);
//   - it has at least one and at most T row records (st_desc[2]): record `tid` is thread tid's, there is no second trip;
//   - it has no generic remainder (st_desc[5] = 0, and with it no right-hand-side remainder, st_desc[6]);
//   - the circuit is not linear: a reused factorisation runs another share of the phase (its right-hand-side column).
bool spicey_u0_resident_fits(const SpiceyProg &P, const uint32_t *st_desc, int T);
// LaunchPlan::u0_resident of a plan whose `top_regs` is decided, on build `shape`: what spicey_plan decides
bool spicey_plan_u0_resident(bool top_regs, const SpiceyProg &P, const uint32_t *st_desc, int T, int shape, const SpiceyKnobs &knobs);
// ... and whether that run takes the resident level-0 record: a register-exchange-top run of a plan that says `u0_resident`
bool spicey_u0_resident_run(const LaunchPlan &plan, int64_t steps);
// The fold of the last factor level into the tridiagonal top (tran_v2_run.h: TF): lane i of the top's wave runs the row
// record of top row i itself and keeps a_ii, y_i and the two fills in registers as the row {a, b, c, d} of the cyclic
// reduction; the level's phase, its barrier and the round trip of the four values through W are gone.
// spicey_top_fold_table builds the table the kernel's prologue copies into the top's first (unused) row buffer — 64 records
// of 8 words, kept behind the parameter record SpiceyRun::zpar (program.h) — and returns false unless ALL of this holds for the program hp (`tail_n`: its resident
// layout's tail levels):
//   - a fresh-fill program with a tridiagonal top at pcr_level >= 1 whose operand slots fit (spicey_slots_fit), not linear
//     (a reused factorisation runs the right-hand-side column of the level alone, which no record of this table does);
//   - every task of factor level pcr_level - 1 (rec16: the records the level's phase runs) is VALID, has one or two inline
//     products (no overflow list), forms no reciprocal (SPICEY_R16_RECIP clear: the top judges its own pivots) and targets
//     the sub-diagonal, diagonal, super-diagonal or right-hand-side entry of a top row (pcr_tab), each target at most once;
//   - a row that has any task has both its diagonal's and its right-hand side's, over the same pivots — the same L_ik and
//     d_k in the same order —, and each fill it has is ONE product with the L_ik and d_k of one of those pivots, two fills
//     with different ones: the row's tasks are then exactly what one row record stands for (program.h: fus16 — where the
//     program has that encoding of the level, the table's records are its records, tests/top_fold_host);
//   - no backward record (rec16 / ovf16 of the phases below the top) names a sub-diagonal, diagonal or super-diagonal entry
//     of a top row as its pivot's diagonal or as a U operand: nothing after the top misses the values that no longer reach
//     W.  (A backward record's target and x operands are right-hand-side / solution slots, never matrix entries; the top's
//     own x slots are written as ever.)
// Beside the resident level-0 record: at pcr_level == 1 the folded level WOULD be level 0, the record's own.  The two never
// meet — the record needs level 0 streamed (more than T x 4 slots of tasks), the fold at most 64 x 4 tasks on it — and
// spicey_plan_top_fold does not rely on that: it refuses pcr_level < 2.
// (No diagnostics phase reads W between the levels here: the packed shapes are never diagnostics builds, spicey_plan.)
// A table record is the row's row record (program.h: fus16) with its four targets turned into READ operands — nothing of it is written:
//   [0] a_ii's index, or the +0.0 slot's where the record creates the entry (SPICEY_ROW_FRESH_AII)   [1] meta as in fus16
//   [2] y_i   [3..8], [9..14] the two pivots as in fus16, but the sixth field = where that pivot's side of the row starts
//   from: the fill target, the +0.0 slot for a fresh one; without a fill, the neighbour entry of pcr_tab that the other
//   pivot does not produce (+0.0 slot: no such neighbour)   [15] bit 0: pivot 0's side is the SUPER-diagonal (else the sub-).
// A top row without a record gets one with no pivot (meta = VALID << 8): its four entries are read as they stand.
bool spicey_top_fold_table(const HostProgram &hp, int tail_n, std::vector<uint32_t> &table);
// LaunchPlan::top_fold of a plan whose `u0_resident` is decided, on build `shape`: what spicey_plan decides
bool spicey_plan_top_fold(bool u0_resident, const HostProgram &hp, int tail_n, int shape, const SpiceyKnobs &knobs);
// ... and whether that run takes the fold: a resident-record run of a plan that says `top_fold`
bool spicey_top_fold_run(const LaunchPlan &plan, int64_t steps);
// The stamp fuse (tran_v2_run.h: SF): Z forms the next step's matrix entries and right-hand-side rows from the conductances
// and companion currents it has just computed, in registers, writes the entries straight into W and, behind one barrier,
// the rows; the time loop holds no phase B, and c.gd / c.u are not written in it.  That needs every sum of phase B to draw on values of ONE
// thread of Z.  spicey_stamp_fuse_table deals the stamped entries and the rows to the threads that produce their operands
// — table[tid * 6 + {0, 1}]: entry slots, + {2, 3}: row slots, + 4: the row of source tid; slot j goes with the thread's
// item j, diode and capacitor tid + j T — and returns false unless ALL of this holds for the fresh-fill program hp on T threads with
// `nsv` entries and `nel` items per thread (`tail_n`: its resident layout's tail levels):
//   - nsv == nel == 2, operand addresses fit (spicey_addr_fits: every W index is below 2^14), not linear (a reused
//     factorisation stamps nothing), no switch (no re-iteration: a_reiterate is the other reader of c.gd / c.u), no inductor;
//   - every beyond-capacity loop of B and Z is empty (TranPhases2::set_remainders: nKeep and nDynEnt <= nsv T, n, nOut, nR,
//     nC, nD <= nel T, nV <= T, no entry with more than two dynamic stamps, no row with more than four contributions);
//   - every dynamic field of a stamped entry (ent_dd, e < nKeep) names a diode, and both fields of one entry the same diode
//     i: the entry takes entry slot i / T of thread i mod T, which no other entry may claim;
//   - a row with a source's value has that one field alone, added; every source has exactly one such row.  The source's
//     thread, t, writes it from the parked value: it is the thread's fifth word and takes none of the two row slots;
//   - every other row with a contribution has at most one capacitor's and one diode's field, both of item i: it takes row
//     slot i / T of thread i mod T, which no other row may claim;
//   - entries and rows that depend on nothing (a kept static entry, a row that is 0.0 in every step) go to the free slots, in
//     ascending (item, thread) order; there must be enough of them.
// A slot word: bits 0-15 the target's index in W (an entry's id is its index: the static part is statv[id]), SPICEY_SF_*
// flags above them (tran_pt_layout.h).  The operands enter in the order of the descriptor's fields today: an entry is
// sv + (+-g) [+ (+-g)], a row 0.0 + first + second with SPICEY_SF_SWAP where the diode's field comes first; a field that the
// descriptor leaves empty read -0.0, so leaving it out changes no bit.
bool spicey_stamp_fuse_table(const HostProgram &hp, int tail_n, int T, int nsv, int nel, std::vector<uint32_t> &table);
// LaunchPlan::stamp_fuse of a plan whose `top_fold` is decided, on build `shape`: what spicey_plan decides
bool spicey_plan_stamp_fuse(bool top_fold, const HostProgram &hp, int tail_n, int T, int shape, const SpiceyKnobs &knobs);
// ... and whether that run takes the fuse: a folded run of a plan that says `stamp_fuse`
bool spicey_stamp_fuse_run(const LaunchPlan &plan, int64_t steps);
// The fixed schedule (tran_v2_run.h: FS): the time loop of a fused run written out — U_0 from the resident record, the resident
// factor levels 1 .. pcr_level - 2, the folded top with the merged backward phase and the early fetch, the remaining
// backward phases, Z and its second phase — with no phase mask, no streamed path, no overflow list and no fork on the phase
// table.  spicey_fixed_schedule_fits returns false unless ALL of this holds for the program hp and its resident layout hres
// (the loop would mis-run anything else):
//   - a tridiagonal top of 1 .. 6 stages at pcr_level >= 2 (the fold's own conditions, asked again) and at most 254 phases;
//   - no phase of the run is streamed but level 0, whose record is resident in its own registers (UR): st_cnt[p] == 0 for
//     every p > 0, st_cnt[0] > 0;
//   - every factor phase the loop runs, 0 .. pcr_level - 2, has tasks, and the resident layout has no LDS tail (tail_n == 0:
//     a top replaces it).  (An empty phase would not be mis-run — its compare chain matches no slot — but the loop has no
//     mask to skip it by and would pay its barrier in every step, where the other form pays nothing: stricter than
//     correctness needs, on purpose);
//   - a backward phase exists below the top and the first of them is merged into the top's wave (k_merge == 2 nLevels -
//     pcr_level < 2 nLevels - 1): with pcr_level > 0 that is the z-prefetch bit of the loop, and the source park has a last
//     backward phase of its own to ride on;
//   - every resident record of a phase the loop runs — factor or backward, row-record chunks apart, which have no count — has
//     at most two products: none uses the overflow list.
// (That Z has no beyond-capacity loop — zrem == 0 — and that nothing re-iterates is the fuse's: spicey_stamp_fuse_table.)
bool spicey_fixed_schedule_fits(const HostProgram &hp, const HostResident &hres);
// LaunchPlan::fixed_schedule of a plan whose `stamp_fuse` is decided, on build `shape`; debug_empty: the empty diagnostics
// phases per solve that the handle's options ask for (SpiceyRun::debug_empty_phases — the written-out loop has none)
bool spicey_plan_fixed_schedule(bool stamp_fuse, const HostProgram &hp, const HostResident &hres, int shape, int debug_empty, const SpiceyKnobs &knobs);
// ... and whether that run takes the fixed schedule: a fused run of a plan that says `fixed_schedule`
bool spicey_fixed_schedule_run(const LaunchPlan &plan, int64_t steps);
// doubles of the parameter record SpiceyRun::zpar of a planned handle: five per resident item, NEL x T items per instance
// (0: the plan runs a build without it); a plan that says `top_fold` keeps SPICEY_TOP_FOLD_WORDS words of table behind them
size_t spicey_zpar_doubles(const LaunchPlan &plan, const HostProgram &hp);
void fill_info(const LaunchPlan &plan, const HostProgram &hp, const HostResident &hres, const SpiceyOptions &opt, SpiceyInfo *info);
