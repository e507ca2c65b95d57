// tran_v1_phases.h — the diagnostics and the v1 phases, TranPhases<K> (tran_exec.h is the map).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "program.h"
#include "tran_common.h"

// ---- diagnostics -------------------------------------------------------------------------------------------------------
// Right after phase B the workspace holds the stamped matrix A (leaf diagonals as reciprocals).  The reference eliminates
// with partial pivoting, so its multiplier for row i at column k is a_ik / max_j |a_jk| (of the matrix as updated so far)
// and `if (Math.abs(f) < EPS) continue` (solveReal.ts:46) SKIPS the row update when that is below 1e-15 — a nonzero
// coupling silently dropped, which a static sparse order does not reproduce (deviations).  This pass counts the
// columns of the STAMPED matrix in which some nonzero entry is below 1e-15 x the column's largest: the first-order
// indicator of that situation (exact for the first pivot; fills and updated entries are not looked at).  One thread per
// column, read-only, no influence on the solve.  `weight` = solves the count stands for (a linear circuit's matrix is
// looked at once, at step 0, for all its steps).
template <int K, bool HYB = false>
SPICEY_HD void spicey_skip_risk(const SpiceyProg &P, const SpiceyRun &R, const WgCtx<K> &c, int tid, int T, unsigned long long weight) {
  SPICEY_NOUNROLL
  for (int col = tid; col < P.n; col += T) {
    const uint32_t j0 = P.col_ptr[col], j1 = P.col_ptr[col + 1];
    for (int k = 0; k < K; k++) {
      if (!c.valid[k]) continue;
      double mx = 0.0, mn = 1.0e308;
      bool any = false;
      for (uint32_t j = j0; j < j1; j++) {
        const uint32_t e = P.col_ent[j];
        const uint32_t id = SPICEY_IDX(e);
        double v;
        if (HYB) {  // hybrid workspace: leaf-owned entries in the global array, the others at their LDS index
          const uint32_t g0 = (uint32_t)P.hyb_g0, nr = (uint32_t)P.nRestore, g2 = (uint32_t)P.hyb_g2;
          if (id < g0 || (id >= nr && id < nr + g2)) v = fabs(c.G[(size_t)id * K + k]);
          else v = fabs(c.W[(size_t)(id - g0 - (id >= nr ? g2 : 0u)) * K + k]);
        } else {
          v = fabs(c.W[(size_t)id * K + k]);
        }
        if (e & SPICEY_TGT_RECIP) v = 1.0 / v;
        if (v != 0.0) { any = true; mx = v > mx ? v : mx; mn = v < mn ? v : mn; }
      }
      if (any && mn / mx < SPICEY_EPS) SPICEY_ATOMIC_ADD_U64(R.skip_risk + c.inst[k], weight);  // (a quotient, like the reference's f)
    }
  }
}
// the one-shot linearisation error of a step (SpiceyRun::lin_err): every wave reports the largest |vd(x) - vd_lin| of its diodes
SPICEY_HD void spicey_lin_err_report(const SpiceyRun &R, size_t inst, int64_t step, int tid, double lerr) {
  const double m = SPICEY_WAVE_MAX(lerr);
  if (SPICEY_WAVE_LEADER(tid) && m > 0.0) {
    unsigned long long bits;
    __builtin_memcpy(&bits, &m, 8);
    SPICEY_ATOMIC_MAX_U64(R.lin_err + inst * (size_t)(R.steps + 1) + (size_t)step, bits);
  }
}

template <int K>
struct TranPhases {
  const SpiceyProg &P;
  const SpiceyRun &R;
  WgCtx<K> &c;
  int T;  // threads
  // the diagnostics of SpiceyOptions.diagnostics are compiled into the kernels with K <= 2 only (the 4-instance kernels have
  // no registers to spare: with them the build reports a stack frame); the host keeps K <= 2 when the option is set
  static constexpr bool DIAG = K <= 2;

  SPICEY_HD double volt(int32_t xi, int k) const { return xi < 0 ? 0.0 : c.W[(size_t)xi * K + k]; }

  // ---- prologue -----------------------------------------------------------------------------
  SPICEY_HD void p0_gstat(int tid) const {
    const double dtc = spicey_max_nan(R.dt, SPICEY_EPS);
    for (int k = 0; k < K; k++) {
      if (!c.valid[k]) continue;
      const size_t in = (size_t)c.inst[k];
      double *g = R.gstat + in * P.nGstat;
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nGstat; i += T) {
        double v;
        if (i < P.nR) v = 1.0 / R.R_val[in * P.nR + i];
        else if (i < P.nR + P.nC) v = R.C_val[in * P.nC + (i - P.nR)] / dtc;
        else if (i < P.nR + P.nC + P.nL) v = dtc / R.L_val[in * P.nL + (i - P.nR - P.nC)];
        else v = 1.0;
        g[i] = v;
      }
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nD; i += T) {
        const double vt = R.D_n[in * P.nD + i] * SPICEY_VT300;
        R.dpar[(in * P.nD + i) * 2 + 0] = 1.0 / vt;
        R.dpar[(in * P.nD + i) * 2 + 1] = R.D_is[in * P.nD + i] / vt;
      }
    }
  }
  SPICEY_HD void p1_static(int tid) const {
    for (int k = 0; k < K; k++) {
      if (!c.valid[k]) continue;
      const size_t in = (size_t)c.inst[k];
      const double *g = R.gstat + in * P.nGstat;
      double *sv = R.statv + in * P.nLU;
      SPICEY_NOUNROLL
      for (int e = tid; e < P.nLU; e += T) {
        double v = 0.0;
        for (uint32_t j = P.stat_ptr[e]; j < P.stat_ptr[e + 1]; j++) {
          const uint32_t ix = P.stat_idx[j];
          const double gv = g[SPICEY_IDX(ix)];
          v = (ix & SPICEY_NEG) ? v - gv : v + gv;
        }
        if (P.ent_flag[e] == 1) {  // static leaf diagonal: pre-invert once per run
          if (fabs(v) < SPICEY_EPS) { c.flags[1] = 1; c.flags[2] = c.inst[k]; }
          v = 1.0 / v;
        }
        sv[e] = v;
      }
      double *rc = R.rcoef + in * P.nRhsIdx;
      SPICEY_NOUNROLL
      for (int j = tid; j < P.nRhsIdx; j += T) rc[j] = g[P.rhs_cof[j]];
    }
  }
  // evaluate elements from the state entering the run (step 0, iter 0)
  SPICEY_HD void a0_initial(int tid) const {
    const int oL = P.nC, oV = P.nC + P.nL, oD = P.nC + P.nL + P.nV;
    for (int k = 0; k < K; k++) {
      const size_t in = (size_t)c.inst[k];
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nC; i += T) c.u[(size_t)i * K + k] = R.C_vprev[in * P.nC + i];
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nL; i += T) c.u[(size_t)(oL + i) * K + k] = R.L_iprev[in * P.nL + i];
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nV; i += T) c.u[(size_t)(oV + i) * K + k] = R.src[in * R.src_stride + i];
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nS; i += T) {
        const int on = R.S_ison[in * P.nS + i];
        c.ison[(size_t)i * K + k] = on;
        c.gd[(size_t)i * K + k] = spicey_switch_g(on, R.S_ron[in * P.nS + i], R.S_roff[in * P.nS + i]);
      }
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nD; i += T) {
        double g, q;
        spicey_diode(R.D_vdprev[in * P.nD + i], R.D_is[in * P.nD + i], R.D_n[in * P.nD + i], g, q);
        c.gd[(size_t)(P.nS + i) * K + k] = g;
        c.u[(size_t)(oD + i) * K + k] = q;
        if (DIAG && R.lin_vd && c.valid[k]) R.lin_vd[in * P.nD + i] = R.D_vdprev[in * P.nD + i];
      }
    }
    static_copy(tid, true);
    if (tid == 0) c.flags[0] = 0;
  }
  SPICEY_HD void static_copy(int tid, bool all = false) const {
    const int ne = all ? P.nLU : P.nRestore;  // entries >= nRestore are never written after the first copy
    for (int k = 0; k < K; k++) {
      const double *sv = R.statv + (size_t)c.inst[k] * P.nLU;
      SPICEY_NOUNROLL
      for (int e = tid; e < ne; e += T) c.W[(size_t)e * K + k] = sv[e];
    }
  }

  // ---- B: dynamic stamps + right-hand side ----------------------------------------------------
  SPICEY_HD void b_stamp(int tid) const {
    if (tid == 0) c.flags[0] = 0;
    SPICEY_NOUNROLL
    for (int t = tid; t < P.nDynEnt; t += T) {
      const uint32_t et = P.dyn_ent[t];
      const uint32_t e = SPICEY_IDX(et);
      const uint32_t j0 = P.dyn_ptr[t], j1 = P.dyn_ptr[t + 1];
      for (int k = 0; k < K; k++) {
        double v = R.statv[(size_t)c.inst[k] * P.nLU + e];
        for (uint32_t j = j0; j < j1; j++) {
          const uint32_t ix = P.dyn_idx[j];
          const double gv = c.gd[(size_t)SPICEY_IDX(ix) * K + k];
          v = (ix & SPICEY_NEG) ? v - gv : v + gv;
        }
        if (et & SPICEY_TGT_RECIP) {
          if (fabs(v) < SPICEY_EPS && c.valid[k]) { c.flags[1] = 1; c.flags[2] = c.inst[k]; }
          v = spicey_rcp(v);
        }
        c.W[(size_t)e * K + k] = v;
      }
    }
    SPICEY_NOUNROLL
    for (int r = tid; r < P.n; r += T) {
      const uint32_t j0 = P.rhs_ptr[r], j1 = P.rhs_ptr[r + 1];
      for (int k = 0; k < K; k++) {
        const double *rc = R.rcoef + (size_t)c.inst[k] * P.nRhsIdx;
        double acc = 0.0;
        for (uint32_t j = j0; j < j1; j++) {
          const uint32_t ix = P.rhs_idx[j];
          const double t = rc[j] * c.u[(size_t)SPICEY_IDX(ix) * K + k];
          acc = (ix & SPICEY_NEG) ? acc - t : acc + t;
        }
        c.W[(size_t)(P.nLU + r) * K + k] = acc;
      }
    }
  }

  // ---- U_l: Schur updates of one elimination-tree level ----------------------------------------
  SPICEY_HD void u_level(int tid, int l, bool reuse = false) const {
    const int nw = T >> 6, w = tid >> 6, lane = tid & 63;
    for (uint32_t s = P.lvl_slice[l] + w; s < P.lvl_slice[l + 1]; s += nw) u_slice(s, lane, reuse);
  }
  // the slices of level l that belong to the bins g, g + G, ... (subtree-local levels below the front cut, program.h),
  // dealt to this workgroup's waves in one round-robin over all of them
  SPICEY_HD void u_bins(int tid, int l, int g, int G, bool reuse) const {
    const uint32_t nw = (uint32_t)(T >> 6), w = (uint32_t)(tid >> 6);
    const int lane = tid & 63;
    const uint32_t *bs = P.bin_upd + (size_t)l * (size_t)(P.nBins + 1);
    uint32_t i = 0;
    for (int b = g; b < P.nBins; b += G) {
      const uint32_t s0 = bs[b], s1 = bs[b + 1];
      for (uint32_t s = s0 + (w + nw - i % nw) % nw; s < s1; s += nw) u_slice(s, lane, reuse);
      i += s1 - s0;
    }
  }
  SPICEY_HD void u_slice(uint32_t s, int lane, bool reuse) const {
    {
      const uint32_t t = s * 64 + lane;
      const uint32_t tgt = P.upd_tgt[t];
      if (tgt == SPICEY_TGT_PAD) return;
      const uint32_t cnt = P.upd_cnt[t];
      const uint32_t off = P.upd_slice[s].off + lane;
      const uint32_t ti = SPICEY_IDX(tgt);
      if (reuse && ti < (uint32_t)P.nLU) return;  // reused factorisation: right-hand-side column only
      double acc[K];
      for (int k = 0; k < K; k++) acc[k] = c.W[(size_t)ti * K + k];
      uint32_t j = 0;
      // long product lists (dense fronts of large circuits): 4 products' indices and operands are in flight at once —
      // one dependent L2 round trip per 4 products instead of per product; the summation order is unchanged
      for (; j + 4 <= cnt; j += 4) {
        uint32_t li[4], di[4], ui[4];
        for (int q = 0; q < 4; q++) {
          li[q] = P.upd_pairs[off + ((j + q) * 3 + 0) * 64];
          di[q] = P.upd_pairs[off + ((j + q) * 3 + 1) * 64];
          ui[q] = P.upd_pairs[off + ((j + q) * 3 + 2) * 64];
        }
        double lv[4][K], dv[4][K], uv[4][K];
        for (int q = 0; q < 4; q++)
          for (int k = 0; k < K; k++) {
            lv[q][k] = c.W[(size_t)li[q] * K + k]; dv[q][k] = c.W[(size_t)di[q] * K + k]; uv[q][k] = c.W[(size_t)ui[q] * K + k];
          }
        for (int q = 0; q < 4; q++)
          for (int k = 0; k < K; k++) acc[k] = fma(-(lv[q][k] * dv[q][k]), uv[q][k], acc[k]);
      }
      for (; j < cnt; j++) {
        const uint32_t li = P.upd_pairs[off + (j * 3 + 0) * 64];
        const uint32_t di = P.upd_pairs[off + (j * 3 + 1) * 64];
        const uint32_t ui = P.upd_pairs[off + (j * 3 + 2) * 64];
        for (int k = 0; k < K; k++)
          acc[k] = fma(-(c.W[(size_t)li * K + k] * c.W[(size_t)di * K + k]), c.W[(size_t)ui * K + k], acc[k]);
      }
      if (tgt & SPICEY_TGT_RECIP) {
        for (int k = 0; k < K; k++) {
          if (fabs(acc[k]) < SPICEY_EPS && c.valid[k]) { c.flags[1] = 1; c.flags[2] = c.inst[k]; }
          acc[k] = spicey_rcp(acc[k]);
        }
      }
      for (int k = 0; k < K; k++) c.W[(size_t)ti * K + k] = acc[k];
    }
  }

  // ---- K_l: backward substitution, column-oriented: the pivots of level l update the rows below them --------
  SPICEY_HD void k_level(int tid, int l) const {
    const int nw = T >> 6, w = tid >> 6, lane = tid & 63;
    for (uint32_t s = P.bk_lvl_slice[l] + w; s < P.bk_lvl_slice[l + 1]; s += nw) k_slice(s, lane);
  }
  SPICEY_HD void k_bins(int tid, int l, int g, int G) const {  // see u_bins
    const uint32_t nw = (uint32_t)(T >> 6), w = (uint32_t)(tid >> 6);
    const int lane = tid & 63;
    const uint32_t *bs = P.bin_bk + (size_t)l * (size_t)(P.nBins + 1);
    uint32_t i = 0;
    for (int b = g; b < P.nBins; b += G) {
      const uint32_t s0 = bs[b], s1 = bs[b + 1];
      for (uint32_t s = s0 + (w + nw - i % nw) % nw; s < s1; s += nw) k_slice(s, lane);
      i += s1 - s0;
    }
  }
  SPICEY_HD void k_slice(uint32_t s, int lane) const {
    {
      const uint32_t t = s * 64 + lane;
      const uint32_t yi = P.bk_x[t];
      if (yi == SPICEY_TGT_PAD) return;
      const uint32_t cnt = P.bk_cnt[t];
      const uint32_t off = P.bk_slice[s].off + lane;
      double acc[K];
      for (int k = 0; k < K; k++) acc[k] = c.W[(size_t)yi * K + k];
      uint32_t j = 0;
      // (as in u_slice: 4 products' indices, then their operands, in flight together; the order of the sum is unchanged)
      if constexpr (K <= 2)  // (the 4-instance kernels have no registers to spare)
      for (; j + 4 <= cnt; j += 4) {
        uint32_t ki[4], di[4], ui[4];
        for (int q = 0; q < 4; q++) {
          ki[q] = P.bk_pairs[off + ((j + q) * 3 + 0) * 64];
          di[q] = P.bk_pairs[off + ((j + q) * 3 + 1) * 64];
          ui[q] = P.bk_pairs[off + ((j + q) * 3 + 2) * 64];
        }
        double kv[4][K], dv[4][K], uv[4][K];
        for (int q = 0; q < 4; q++)
          for (int k = 0; k < K; k++) {
            kv[q][k] = c.W[(size_t)ki[q] * K + k]; dv[q][k] = c.W[(size_t)di[q] * K + k]; uv[q][k] = c.W[(size_t)ui[q] * K + k];
          }
        for (int q = 0; q < 4; q++)
          for (int k = 0; k < K; k++) acc[k] = fma(-(kv[q][k] * dv[q][k]), uv[q][k], acc[k]);
      }
      for (; j < cnt; j++) {
        const uint32_t ki = P.bk_pairs[off + (j * 3 + 0) * 64];
        const uint32_t di = P.bk_pairs[off + (j * 3 + 1) * 64];
        const uint32_t ui = P.bk_pairs[off + (j * 3 + 2) * 64];
        for (int k = 0; k < K; k++)
          acc[k] = fma(-(c.W[(size_t)ki * K + k] * c.W[(size_t)di * K + k]), c.W[(size_t)ui * K + k], acc[k]);
      }
      for (int k = 0; k < K; k++) c.W[(size_t)yi * K + k] = acc[k];
    }
  }
  // x[i] = y[i] * dinv[i] for every unknown (after the last level)
  SPICEY_HD void k_scale(int tid) const {
    SPICEY_NOUNROLL
    for (int i = tid; i < P.n; i += T) {
      const uint32_t di = P.bk_d[i];
      for (int k = 0; k < K; k++) c.W[(size_t)(P.nLU + i) * K + k] *= c.W[(size_t)di * K + k];
    }
  }

  // ---- S: switch hysteresis (updateSwitchStatesFromSolution, simulateTRAN.ts:108-128) -----------
  SPICEY_HD void s_switches(int tid) const {
    SPICEY_NOUNROLL
    for (int i = tid; i < P.nS; i += T)
      for (int k = 0; k < K; k++) {
        const size_t in = (size_t)c.inst[k];
        const double vctrl = volt(P.S_cp[i], k) - volt(P.S_cn[i], k);
        const int on = c.ison[(size_t)i * K + k];
        int next = on;
        if (on) {
          if (vctrl < R.S_voff[in * P.nS + i]) next = 0;
        } else if (vctrl > R.S_von[in * P.nS + i]) {
          next = 1;
        }
        if (next != on) {
          c.ison[(size_t)i * K + k] = next;
          c.flags[0] = 1;
        }
      }
  }
  // ---- A': re-linearise for iteration >= 1 (diodes from x, simulateTRAN.ts:81-85) ----------------
  SPICEY_HD void a_reiterate(int tid) const {
    const int oD = P.nC + P.nL + P.nV;
    for (int k = 0; k < K; k++) {
      const size_t in = (size_t)c.inst[k];
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nS; i += T)
        c.gd[(size_t)i * K + k] = spicey_switch_g(c.ison[(size_t)i * K + k], R.S_ron[in * P.nS + i], R.S_roff[in * P.nS + i]);
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nD; i += T) {
        double g, q;
        const double vd = volt(P.D_a[i], k) - volt(P.D_b[i], k);
        spicey_diode(vd, R.D_is[in * P.nD + i], R.D_n[in * P.nD + i], g, q);
        c.gd[(size_t)(P.nS + i) * K + k] = g;
        c.u[(size_t)(oD + i) * K + k] = q;
        if (DIAG && R.lin_vd && c.valid[k]) R.lin_vd[in * P.nD + i] = vd;
      }
    }
    static_copy(tid);
  }

  // ---- Z: record, update state, evaluate the next step's companions ----------------------------
  SPICEY_HD void z_record(int tid, int64_t step, bool keep_factors = false) const {
    const bool last = step == R.steps;
    const int oL = P.nC, oV = P.nC + P.nL, oD = P.nC + P.nL + P.nV;
    const int cR = 0, cC = P.nR, cL = P.nR + P.nC, cV = cL + P.nL, cS = cV + P.nV, cD = cS + P.nS;
    for (int k = 0; k < K; k++) {
      if (!c.valid[k]) continue;
      const size_t in = (size_t)c.inst[k];
      double *ov = R.out_v + (in * (size_t)(R.steps + 1) + (size_t)step) * P.nOut;
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nOut; i += T) ov[i] = volt(P.out_x[i], k);
      const bool cur = R.out_i != nullptr;
      double *oi = cur ? R.out_i + (in * (size_t)(R.steps + 1) + (size_t)step) * P.nCur : nullptr;
      const double *g = R.gstat + in * P.nGstat;
      if (cur)
        SPICEY_NOUNROLL
        for (int i = tid; i < P.nR; i += T) oi[cR + i] = (volt(P.R_a[i], k) - volt(P.R_b[i], k)) * g[i];
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nC; i += T) {
        const double dv = volt(P.C_a[i], k) - volt(P.C_b[i], k);
        if (cur) oi[cC + i] = g[P.nR + i] * (dv - c.u[(size_t)i * K + k]);
        c.u[(size_t)i * K + k] = dv;
        if (last) R.C_vprev[in * P.nC + i] = dv;
      }
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nL; i += T) {
        const double dv = volt(P.L_a[i], k) - volt(P.L_b[i], k);
        const double il = g[P.nR + P.nC + i] * dv + c.u[(size_t)(oL + i) * K + k];
        if (cur) oi[cL + i] = il;
        c.u[(size_t)(oL + i) * K + k] = il;
        if (last) R.L_iprev[in * P.nL + i] = il;
      }
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nV; i += T) {
        if (cur) oi[cV + i] = c.W[(size_t)P.V_x[i] * K + k];
        if (!last) c.u[(size_t)(oV + i) * K + k] = R.src[in * R.src_stride + (size_t)(step + 1) * P.nV + i];
      }
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nS; i += T) {
        const int on = c.ison[(size_t)i * K + k];
        const double gs = spicey_switch_g(on, R.S_ron[in * P.nS + i], R.S_roff[in * P.nS + i]);
        if (cur) oi[cS + i] = (volt(P.S_a[i], k) - volt(P.S_b[i], k)) * gs;
        c.gd[(size_t)i * K + k] = gs;
        if (last) R.S_ison[in * P.nS + i] = on;
      }
      double lerr = 0.0;
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nD; i += T) {
        const double vd = volt(P.D_a[i], k) - volt(P.D_b[i], k);
        const double is = R.D_is[in * P.nD + i];
        const double *dp = R.dpar + (in * P.nD + i) * 2;  // {1/(N VT), Is/(N VT)} from the prologue
        double gg, q, irec;
        spicey_diode_k(vd, is, dp[0], dp[1], cur, gg, q, irec);
        if (cur) oi[cD + i] = irec;  // unclamped, simulateTRAN.ts:214-217
        c.gd[(size_t)(P.nS + i) * K + k] = gg;
        c.u[(size_t)(oD + i) * K + k] = q;
        if (last) R.D_vdprev[in * P.nD + i] = vd;
        if (DIAG && R.lin_vd) {  // diagnostics: how far the junction moved from where this solve had it linearised
          const double e = fabs(vd - R.lin_vd[in * P.nD + i]);
          lerr = e > lerr ? e : lerr;
          R.lin_vd[in * P.nD + i] = vd;
        }
      }
      if (DIAG && R.lin_err) spicey_lin_err_report(R, in, step, tid, lerr);
    }
    if (!keep_factors) static_copy(tid);  // a linear circuit keeps the factors of step 0 in W
  }
};
