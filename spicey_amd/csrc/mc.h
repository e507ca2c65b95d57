// mc.h — the host side of the Monte Carlo pass: validation, plan and workspace layout (mc_exec.h holds the arithmetic and the
// mapping).  Plain C++, shared by spicey_abi.cpp, ac_abi.cpp, mc.hip and the CPU harness of tests/mc_host; the launchers of
// mc.hip are declared at the end for translation units that have the HIP runtime's types.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>

#include "../../include/spicey_hip.h"
#include "mc_exec.h"

// The draw's workspace: the record | tol [nE] | icdf [K + 1].
inline int64_t spicey_mc_draw_tol_offset() { return spicey_meas_align((int64_t)sizeof(SpiceyMcDrawArgs)); }
inline int64_t spicey_mc_draw_icdf_offset(int32_t nE) { return spicey_mc_draw_tol_offset() + spicey_meas_align((int64_t)nE * (int64_t)sizeof(double)); }
inline int64_t spicey_mc_draw_bytes(int32_t nE, int32_t log2K) {
  if (nE <= 0 || log2K < 0 || log2K > SPICEY_MC_MAX_LOG2K) return -1;
  return spicey_mc_draw_icdf_offset(nE) + spicey_meas_align((((int64_t)1 << log2K) + 1) * (int64_t)sizeof(double));
}

// The reduction's workspace: the record | valid [n_inst] bytes | lo [n_freq] | hi [n_freq] | ranks [n_rank] — the head, one
// copy from the host — | qT [n_freq][n_pad].
struct SpiceyMcLayout { int64_t off_valid, off_lo, off_hi, off_ranks, head_bytes, total_bytes; int32_t n_pad; };
inline int32_t spicey_mc_pad(int32_t n_inst) {
  int32_t p = 1;
  while (p < n_inst) p <<= 1;
  return p;
}
inline bool spicey_mc_layout(int32_t n_inst, int64_t n_freq, int32_t n_rank, SpiceyMcLayout &l) {
  if (n_inst <= 0 || n_inst > SPICEY_MC_MAX_INST || n_freq <= 0 || n_rank < 0) return false;
  l.n_pad = spicey_mc_pad(n_inst);
  l.off_valid = spicey_meas_align((int64_t)sizeof(SpiceyMcReduceArgs));
  l.off_lo = l.off_valid + spicey_meas_align(n_inst);
  l.off_hi = l.off_lo + spicey_meas_align(n_freq * (int64_t)sizeof(double));
  l.off_ranks = l.off_hi + spicey_meas_align(n_freq * (int64_t)sizeof(double));
  l.head_bytes = l.off_ranks + spicey_meas_align((int64_t)(n_rank ? n_rank : 1) * (int64_t)sizeof(int64_t));
  l.total_bytes = l.head_bytes + n_freq * (int64_t)l.n_pad * (int64_t)sizeof(uint64_t);
  return true;
}
inline int64_t spicey_mc_reduce_bytes(int32_t n_inst, int64_t n_freq, int32_t n_rank) {
  SpiceyMcLayout l;
  return spicey_mc_layout(n_inst, n_freq, n_rank, l) ? l.total_bytes : -1;
}

// What serves either call (spicey_ac_mc_workspace_bytes); -1 for arguments no launch accepts.
inline int64_t spicey_mc_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nE, int32_t log2K, int32_t n_rank) {
  const int64_t a = spicey_mc_draw_bytes(nE, log2K), b = spicey_mc_reduce_bytes(n_inst, n_freq, n_rank);
  return a < 0 || b < 0 ? -1 : (a > b ? a : b);
}

// threads of the sorting workgroup: a pair each up to the most a workgroup has (the result does not depend on it)
inline int32_t spicey_mc_sort_threads(int32_t n_pad) {
  const int32_t t = n_pad / 2;
  return t < SPICEY_MC_LANES ? SPICEY_MC_LANES : t > SPICEY_MC_SORT_MAX ? SPICEY_MC_SORT_MAX : t;
}

inline const char *spicey_mc_judge_req(const SpiceyAcMcReq *req) {
  if (!req) return "null request";
  if (req->struct_bytes != (int64_t)sizeof(SpiceyAcMcReq)) return "struct_bytes is not sizeof(SpiceyAcMcReq)";
  if (req->reserved != 0) return "reserved must be 0";
  if (req->log2K < 0 || req->log2K > SPICEY_MC_MAX_LOG2K) return "log2K outside [0, 12]";
  return nullptr;
}

// Every refusal of a draw, judged before the device is touched (a refusal launches nothing).  tol [nE] and icdf [K + 1] are
// HOST arrays.  true: `A` is the kernel's record, buffers included, except A.tol and A.icdf, which the launcher points into
// the workspace.
inline bool spicey_mc_draw_judge(int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C, const double *d_L, const double *tol,
                                 const double *icdf, const SpiceyAcMcReq *req, double *d_oR, double *d_oC, double *d_oL, bool have_work, int64_t work_bytes,
                                 SpiceyMcDrawArgs &A, std::string &err) {
  const char *what = spicey_mc_judge_req(req);
  if (what) {
  } else if (n_inst <= 0) what = "bad counts (n_inst >= 1)";
  else if (n_inst > SPICEY_MC_MAX_INST) what = "n_inst exceeds 16384, the keys one workgroup sorts in LDS";
  else if (nR < 0 || nC < 0 || nL < 0) what = "bad counts (nR, nC, nL >= 0)";
  else if (nR == 0 && nC == 0 && nL == 0) what = "no element (nR + nC + nL = 0)";
  else if (!tol || !icdf || !have_work || (nR && (!d_R || !d_oR)) || (nC && (!d_C || !d_oC)) || (nL && (!d_L || !d_oL))) what = "null buffer";
  else if (work_bytes < spicey_mc_draw_bytes(nR + nC + nL, req->log2K)) what = "workspace too small (spicey_ac_mc_workspace_bytes)";
  else {
    const int64_t K = (int64_t)1 << req->log2K;
    for (int64_t j = 0; j <= K && !what; j++)
      if (!std::isfinite(icdf[j]) || (j > 0 && !(icdf[j] >= icdf[j - 1]))) what = "the table must be finite and non-decreasing";
    if (!what) {
      const double top = std::fmax(std::fabs(icdf[0]), std::fabs(icdf[K]));
      for (int32_t e = 0; e < nR + nC + nL && !what; e++)
        if (!(tol[e] >= 0.0) || !std::isfinite(tol[e])) what = "a tolerance must be finite and >= 0";
        else if (!(tol[e] * top < 1.0)) what = "tol * max|icdf| >= 1: a drawn value could be zero or negative";
    }
  }
  if (what) {
    err = std::string("mc: ") + what;
    return false;
  }
  A = SpiceyMcDrawArgs{d_R, d_C, d_L, nullptr, nullptr, d_oR, d_oC, d_oL, req->seed, n_inst, nR, nC, nL, req->log2K, req->keep_first ? 1 : 0};
  return true;
}

// Every refusal of a reduction.  valid [n_inst] (or null: all valid), lo / hi [n_freq] (or null: no limit on that side; both
// null: no mask) and ranks [n_rank] are HOST arrays.  true: `A` is the kernels' record except the pointers into the
// workspace, which the launcher sets.
inline bool spicey_mc_reduce_judge(int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const uint8_t *valid, const int64_t *ranks, int32_t n_rank,
                                   const SpiceyAcMcReq *req, bool have_out, int64_t work_bytes, SpiceyMcReduceArgs &A, std::string &err) {
  const char *what = spicey_mc_judge_req(req);
  int32_t n_valid = 0;
  if (what) {
  } else if (n_inst <= 0 || n_freq <= 0 || n_v <= 0 || n_rank < 0) what = "bad counts (n_inst, n_freq, n_v >= 1, n_rank >= 0)";
  else if (n_inst > SPICEY_MC_MAX_INST) what = "n_inst exceeds 16384, the keys one workgroup sorts in LDS";
  else if ((int64_t)n_inst * n_freq > 0x7fffffffll) what = "n_inst * n_freq exceeds the grid limit";
  else if (!d_v || !have_out || (n_rank && !ranks)) what = "null buffer";
  else if (req->out_p < -1 || req->out_p >= n_v || req->out_n < -1 || req->out_n >= n_v) what = "column out of range";
  else if (req->out_p == req->out_n) what = "the output pair names one node twice (or ground twice)";
  else if (work_bytes < spicey_mc_reduce_bytes(n_inst, n_freq, n_rank)) what = "workspace too small (spicey_ac_mc_workspace_bytes)";
  else {
    for (int32_t s = 0; s < n_inst; s++) n_valid += !valid || valid[s];
    for (int32_t j = 0; j < n_rank && !what; j++)
      if (ranks[j] < 0 || ranks[j] >= n_valid) what = "a rank outside [0, n_valid)";
  }
  if (what) {
    err = std::string("mc: ") + what;
    return false;
  }
  const int32_t n_pad = spicey_mc_pad(n_inst);
  A = SpiceyMcReduceArgs{d_v, nullptr, nullptr, nullptr, nullptr, nullptr, n_freq, n_inst, n_pad, n_valid, n_v, req->out_p, req->out_n, n_rank, spicey_mc_sort_threads(n_pad)};
  return true;
}

// The head of the reduction's workspace as the launcher uploads it and the harness reads it: `A`'s pointers set to where
// `base` (the workspace's address on the side that will read it) puts them.  head: l.head_bytes bytes.
inline void spicey_mc_reduce_head(const SpiceyMcLayout &l, SpiceyMcReduceArgs &A, const uint8_t *valid, const double *lo, const double *hi, const int64_t *ranks,
                                  char *head, char *base) {
  const double inf = INFINITY;
  A.valid = valid ? (const uint8_t *)(base + l.off_valid) : nullptr;
  A.lo = lo || hi ? (const double *)(base + l.off_lo) : nullptr;
  A.hi = lo || hi ? (const double *)(base + l.off_hi) : nullptr;
  A.ranks = (const int64_t *)(base + l.off_ranks);
  A.qT = (uint64_t *)(base + l.head_bytes);
  memset(head, 0, (size_t)l.head_bytes);
  memcpy(head, &A, sizeof(A));
  if (valid) memcpy(head + l.off_valid, valid, (size_t)A.n_inst);
  for (int64_t k = 0; k < A.n_freq && (lo || hi); k++) {
    const double a = lo ? lo[k] : -inf, b = hi ? hi[k] : inf;
    memcpy(head + l.off_lo + k * 8, &a, 8);
    memcpy(head + l.off_hi + k * 8, &b, 8);
  }
  if (A.n_rank) memcpy(head + l.off_ranks, ranks, (size_t)A.n_rank * sizeof(int64_t));
}

#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H)
// The draw kernel, enqueued on `st` behind a copy of `A` (HOST, from spicey_mc_draw_judge), tol (HOST [nE]) and icdf (HOST
// [K + 1]) into the head of d_work.  The device must be current.  No synchronisation.
hipError_t spicey_launch_mc_draw(int device, const SpiceyMcDrawArgs &A, const double *tol, const double *icdf, void *d_work, hipStream_t st);
// The two kernels of the reduction, enqueued on `st` behind a copy of `A` (HOST, from spicey_mc_reduce_judge) and of the HOST
// arrays valid, lo, hi and ranks into the head of d_work.  d_sample [n_inst][2] int64, d_freq [n_freq][4 + n_rank].
hipError_t spicey_launch_mc_reduce(int device, const SpiceyMcReduceArgs &A, const uint8_t *valid, const double *lo, const double *hi, const int64_t *ranks,
                                   int64_t *d_sample, double *d_freq, void *d_work, hipStream_t st);
#endif
