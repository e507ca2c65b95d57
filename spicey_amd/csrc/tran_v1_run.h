// tran_v1_run.h — the v1 run driver, spicey_tran_run, with the dense-front sweeps (tran_exec.h is the map).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fronts_exec.h"
#include "program.h"
#include "tran_common.h"
#include "tran_v1_phases.h"

// The whole run of one workgroup.  Exec supplies `phase(f)` (run f(tid) for every thread, then
// barrier) and `threads()`.  All control flow is workgroup-uniform: flags are read after barriers.
// FRONTS: compile the dense-front sweeps in (their triangular solves keep 16 doubles per thread in registers: kernels
// built with them are launched with <= 512 threads; the others keep their 1024-thread register budget untouched).
template <int K, bool FRONTS = false, class Exec>
SPICEY_HD void spicey_tran_run(Exec &ex, const SpiceyProg &P, const SpiceyRun &R, WgCtx<K> &c, int wg) {
  TranPhases<K> ph{P, R, c, ex.threads()};
  TranPhases<K> phl{P, R, c, ex.local_threads()};  // the same phases over ONE workgroup's threads (group mode)
  ex.phase(SPICEY_PH_PRO, [&](int tid) {
    if (tid == 0) { c.flags[0] = 0; c.flags[1] = 0; c.flags[2] = -1; }
    ph.p0_gstat(tid);
  });
  ex.phase(SPICEY_PH_PRO, [&](int tid) { ph.p1_static(tid); });
  ex.phase(SPICEY_PH_PRO, [&](int tid) { ph.a0_initial(tid); });
  unsigned long long solves = 0;
  int32_t code = 0;
  int64_t err_step = 0;
  int32_t err_iter = 0;
  if (c.flags[1]) { code = 1; }
  const bool linear = P.nD == 0 && P.nS == 0 && P.nDynEnt == 0 && !R.no_reuse;  // see spicey_tran_run_v2
  // dense fronts above the cut (K = 1 only; the host enables them for nonlinear circuits, so `linear` is false then)
  const bool use_fronts = FRONTS && K == 1 && P.nFronts > 0 && R.front_ws != nullptr;
  FrontsRun<Exec> fr{ex, P, R, c.W, c.flags, c.inst[0], c.valid[0], use_fronts ? R.front_ws + (size_t)wg * (size_t)P.front_ws : nullptr,
                     use_fronts ? R.front_flags + (size_t)wg * 2 * (size_t)P.nFronts : nullptr, ex.local_threads(),
                     use_fronts && R.front_ticks ? R.front_ticks + (size_t)wg * 4 * (size_t)P.nFronts : nullptr};
  unsigned int fepoch = 0;
  for (int64_t step = 0; step <= R.steps && code == 0; step++) {
    if (ex.failed()) { code = 3; err_step = step; break; }  // a cross-workgroup barrier timed out (group mode only)
    int iter = 0;
    for (;;) {
      ex.phase(SPICEY_PH_B, [&](int tid) { ph.b_stamp(tid); });
      if (TranPhases<K>::DIAG && R.skip_risk && !(linear && step > 0))  // diagnostics: the stamped matrix, before the factor levels touch it
        ex.phase(SPICEY_PH_S, [&](int tid) { spicey_skip_risk<K>(P, R, c, tid, ex.threads(), linear ? (unsigned long long)(R.steps + 1) : 1ull); });
      ex.mark(SPICEY_PH_B);
      {
        // Group mode: runs of narrow factor levels (<= 1024 tasks, one per thread: the last pivots of the top separator) also go to
        // workgroup 0 alone; a group barrier separates such a run from the next level that everybody works on.
        bool local_run = false;
        int l_first = 0;
        if constexpr (FRONTS) if (use_fronts && P.nBins > 0) {
          // subtree-local levels below the cut (program.h): every workgroup walks its bins through all those levels with
          // its own barriers; one group barrier, then the targets above the cut take their products in one phase
          ex.for_each_wg([&](int g, int G) {
            for (int l = 0; l < P.front_cut; l++) ex.wg_phase([&](int tid) { phl.u_bins(tid, l, g, G, linear && step > 0); });
          });
          ex.mark(SPICEY_PH_U0 + 18);
          ex.sync();
          ex.mark(SPICEY_PH_U0 + 19);
          l_first = P.front_cut;
        }
        // (above a front cut the lists are empty: nothing to walk; with bins, one phase is left)
        const int l_end = use_fronts ? P.front_cut + (P.nBins > 0 ? 1 : 0) : P.nLevels;
        for (int l = l_first; l < l_end; l++) {
          const uint32_t nsl = P.lvl_slice[l + 1] - P.lvl_slice[l];
          if (nsl == 0) continue;
          if (ex.serial_chain() && nsl <= 16) {
            ex.local_phase([&](int tid) { phl.u_level(tid, l, linear && step > 0); });
            local_run = true;
          } else {
            if (local_run) ex.sync();
            local_run = false;
            if (l_first > 0 && l == l_first) ex.phase_marked(SPICEY_PH_U0 + 22, [&](int tid) { ph.u_level(tid, l, linear && step > 0); });
            else ex.phase(SPICEY_PH_U0 + (l < 31 ? l : 31), [&](int tid) { ph.u_level(tid, l, linear && step > 0); });
          }
        }
        // (a trailing local run flows straight into the backward chain below, which workgroup 0 runs as well)
        if (local_run && (!ex.serial_chain() || use_fronts)) ex.sync();
      }
      ex.mark(SPICEY_PH_U0);
      if constexpr (FRONTS) if (use_fronts) {
        // upper tree: every workgroup sweeps its share of the fronts up, then down (flags between workgroups, no group
        // barrier inside); one group barrier afterwards publishes the upper unknowns to the levels below the cut
        fepoch++;
        const unsigned long long t_sweep = fr.forward(fepoch);
        ex.mark(SPICEY_PH_U0 + 1);
        fr.backward(fepoch, t_sweep);
        ex.mark(SPICEY_PH_U0 + 2);
        ex.local_phase([&](int tid) { if (tid == 0) c.W[(size_t)P.one_slot * K] = 1.0; });
        ex.sync();
        ex.mark(SPICEY_PH_U0 + 3);
      }
      if (ex.serial_chain()) {
        // Group mode: the backward levels carry little work (mesh 100^2: 172 k products over 297 levels) but each
        // would cost a cross-workgroup barrier (~4.7 us): ONE workgroup of the group walks them with its own
        // workgroup barriers, the others wait at the single group barrier behind the chain.
        // (with dense fronts the levels that are left are the WIDE ones at the bottom of the tree — thousands of rows each,
        // the interface phase included: those go to all workgroups, one group barrier each)
        bool local_run = false;
        int l_last = 0;
        if (use_fronts && P.nBins > 0) l_last = P.front_cut + 1;  // (the interface and the levels below it follow, bin by bin)
        for (int l = use_fronts ? P.front_cut : P.nLevels - 1; l >= l_last; l--) {  // (backward level `front_cut`: the interface)
          const uint32_t nsl = P.bk_lvl_slice[l + 1] - P.bk_lvl_slice[l];
          if (nsl == 0) continue;
          if (use_fronts && nsl > 16) {
            if (local_run) ex.sync();
            local_run = false;
            ex.phase(SPICEY_PH_K0 + 31, [&](int tid) { ph.k_level(tid, l); });
            continue;
          }
          ex.local_phase([&](int tid) { phl.k_level(tid, l); });
          local_run = true;
        }
        if constexpr (FRONTS) if (l_last > 0) {
          if (local_run) ex.sync();
          local_run = true;  // (one group barrier behind the bins)
          ex.mark(SPICEY_PH_U0 + 20);
          ex.for_each_wg([&](int g, int G) {
            for (int l = P.front_cut; l >= 0; l--) ex.wg_phase([&](int tid) { phl.k_bins(tid, l, g, G); });
          });
          ex.mark(SPICEY_PH_U0 + 21);
        }
        if (local_run || !use_fronts) ex.sync();
      } else {
        int l_last = 0;
        if (use_fronts && P.nBins > 0) l_last = P.front_cut + 1;
        for (int l = use_fronts ? P.front_cut : P.nLevels - 1; l >= l_last; l--) {
          if (P.bk_lvl_slice[l] == P.bk_lvl_slice[l + 1]) continue;
          ex.phase(SPICEY_PH_K0 + (l < 31 ? l : 31), [&](int tid) { ph.k_level(tid, l); });
        }
        if constexpr (FRONTS) if (l_last > 0)
          ex.for_each_wg([&](int g, int G) {
            for (int l = P.front_cut; l >= 0; l--) ex.wg_phase([&](int tid) { phl.k_bins(tid, l, g, G); });
          });
      }
      ex.phase(SPICEY_PH_K0, [&](int tid) { ph.k_scale(tid); });
      ex.mark(SPICEY_PH_K0);
      // a cross-workgroup barrier that timed out inside this iteration leaves a partially computed workspace: nothing of
      // it may be recorded or reported as a success (group mode only; the flag is sticky and uniform across the group)
      if (ex.failed()) { code = 3; err_step = step; err_iter = iter; break; }
      if (c.flags[1]) { code = 1; err_step = step; err_iter = iter; break; }
      if (P.nS == 0) break;
      ex.phase(SPICEY_PH_S, [&](int tid) { ph.s_switches(tid); });
      const int switched = c.flags[0];
      if (!switched || iter == SPICEY_MAX_ITER - 1) break;
      iter++;
      ex.phase(SPICEY_PH_A, [&](int tid) { ph.a_reiterate(tid); });  // b_stamp (next) resets flags[0] after this barrier
    }
    if (code) break;
    {
      int nvalid = 0;
      for (int k = 0; k < K; k++) nvalid += c.valid[k];
      solves += (unsigned long long)(iter + 1) * (unsigned long long)nvalid;
    }
    ex.phase(SPICEY_PH_Z, [&](int tid) {
      if (tid == 0 && R.iters)
        for (int k = 0; k < K; k++)
          if (c.valid[k]) R.iters[(size_t)c.inst[k] * (size_t)(R.steps + 1) + (size_t)step] = iter + 1;
      ph.z_record(tid, step, linear);
    });
    ex.mark(SPICEY_PH_Z);
    if (ex.failed()) { code = 3; err_step = step; break; }  // also covers the last step and runs with steps = 0
  }
  ex.phase(SPICEY_PH_PRO, [&](int tid) {
    if (tid == 0) {
      R.status[wg * 4 + 0] = code;
      R.status[wg * 4 + 1] = c.flags[2];
      R.status[wg * 4 + 2] = (int32_t)err_step;
      R.status[wg * 4 + 3] = err_iter;
      R.solves[wg] = solves;
    }
  });
}
