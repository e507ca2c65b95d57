// pss.h — the host side of the periodic steady state: validation and workspace layout (pss_exec.h holds the arithmetic, the
// mapping and the order).  Plain C++, shared by device_abi.cpp, pss_abi.cpp, pss.hip and the CPU harness of tests/pss_host; the
// launchers of pss.hip are declared at the end for translation units that have the HIP runtime's types.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/spicey_hip.h"
#include "pss_exec.h"

inline int64_t spicey_pss_align(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
inline int32_t spicey_pss_width(int32_t method, int32_t nX) { return method == SPICEY_PSS_SETTLE ? 1 : 1 + nX; }
// Bytes of dynamic LDS of the update: the matrix with its right-hand side, row stride nX + 1 doubles (132 096 at nX = 128).
inline size_t spicey_pss_lds_bytes(int32_t method, int32_t nX) { return method == SPICEY_PSS_SETTLE ? 0 : (size_t)nX * (size_t)(nX + 1) * sizeof(double); }

// The workspace: the record | ist [n_inst] int32.
struct SpiceyPssLayout { int64_t off_ist, total_bytes, n_inst; };
inline bool spicey_pss_layout(int32_t n_ckt, int32_t nX, int32_t method, SpiceyPssLayout &l) {
  if (n_ckt < 1 || nX < 1 || (method != SPICEY_PSS_NEWTON && method != SPICEY_PSS_SETTLE)) return false;
  if (method == SPICEY_PSS_NEWTON && nX > SPICEY_PSS_MAX_NX) return false;
  l.n_inst = (int64_t)n_ckt * spicey_pss_width(method, nX);
  if (l.n_inst * nX > 0x7fffffffll) return false;
  l.off_ist = spicey_pss_align((int64_t)sizeof(SpiceyPssArgs));
  l.total_bytes = l.off_ist + spicey_pss_align(l.n_inst * (int64_t)sizeof(int32_t));
  return true;
}
inline int64_t spicey_pss_bytes(int32_t n_ckt, int32_t nX, int32_t method) {
  SpiceyPssLayout l;
  return spicey_pss_layout(n_ckt, nX, method, l) ? l.total_bytes : -1;
}

inline bool spicey_pss_pos(double v) { return std::isfinite(v) && v > 0.0; }

// Every refusal of the request and the counts, judged before the device is touched.  run: spicey_run_pss, which looks at max_iter.
inline const char *spicey_pss_judge_req(const SpiceyPssReq *req, int32_t nC, int32_t nL, int32_t nD, int32_t nS, bool run, char *buf, size_t cap) {
  if (!req) return "null request";
  if (req->struct_bytes != (int64_t)sizeof(SpiceyPssReq)) return "struct_bytes is not sizeof(SpiceyPssReq)";
  if (req->pad != 0 || req->reserved != 0) return "pad and reserved must be 0";
  if (req->method != SPICEY_PSS_NEWTON && req->method != SPICEY_PSS_SETTLE) return "unknown method";
  if (req->n_ckt < 1) return "bad counts (n_ckt >= 1)";
  if (nC < 0 || nL < 0 || nD < 0 || nS < 0) return "bad counts (nC, nL, nD, nS >= 0)";
  const int64_t nX = (int64_t)nC + nL + nD;
  if (nX == 0) return "the circuit has no state (nX = nC + nL + nD = 0)";
  if (req->method == SPICEY_PSS_NEWTON && nX > SPICEY_PSS_MAX_NX) {
    snprintf(buf, cap, "nX = %lld states exceed the %d of the Newton update; method = \"settle\" takes any number", (long long)nX, SPICEY_PSS_MAX_NX);
    return buf;
  }
  if (nX > 0x7fffffffll || (int64_t)req->n_ckt * spicey_pss_width(req->method, (int32_t)nX) * nX > 0x7fffffffll) return "too many state entries";
  if (run && req->max_iter < 1) return "max_iter must be >= 1";
  if (!spicey_pss_pos(req->reltol) || !spicey_pss_pos(req->vabstol) || !spicey_pss_pos(req->iabstol)) return "the tolerances must be finite and > 0";
  if (!spicey_pss_pos(req->rel_step) || !spicey_pss_pos(req->v_scale) || !spicey_pss_pos(req->i_scale)) return "rel_step, v_scale and i_scale must be finite and > 0";
  if (!spicey_pss_pos(req->damping) || req->damping > 1.0) return "damping must be in (0, 1]";
  return nullptr;
}

// Every refusal of a design (update = false) or an update.  true: `A` is the kernels' record except A.ist, which
// spicey_pss_head points into the workspace.
inline bool spicey_pss_judge(bool update, int32_t nC, int32_t nL, int32_t nD, int32_t nS, const SpiceyPssReq *req, int32_t perturb, double *base, int32_t *base_on,
                             double *h_eff, double *Cv, double *Li, double *Dv, int32_t *Son, double *delta, double *rows, int32_t *done, bool have_work,
                             int64_t work_bytes, SpiceyPssArgs &A, std::string &err) {
  char buf[192];
  const char *what = spicey_pss_judge_req(req, nC, nL, nD, nS, false, buf, sizeof(buf));
  if (what) {
  } else if (!have_work || !base || (nS && (!base_on || !Son)) || (nC && !Cv) || (nL && !Li) || (nD && !Dv)) what = "null buffer";
  else if (req->method == SPICEY_PSS_NEWTON && (update || perturb) && !h_eff) what = "null buffer";
  else if (update && (!rows || !done)) what = "null buffer";
  else if (work_bytes < spicey_pss_bytes(req->n_ckt, nC + nL + nD, req->method)) what = "workspace too small (spicey_pss_workspace_bytes)";
  if (what) {
    err = std::string("pss: ") + what;
    return false;
  }
  A = SpiceyPssArgs{base, base_on, h_eff, Cv, Li, Dv, Son, delta, rows, done, nullptr, req->damping, req->reltol, req->vabstol, req->iabstol,
                    req->rel_step, req->v_scale, req->i_scale, req->n_ckt, nC, nL, nD, nS, req->method, perturb != 0 && req->method == SPICEY_PSS_NEWTON, 0};
  return true;
}

// The workspace as the launcher uploads it and the harness reads it: A.ist set to where `base` (the workspace's address on the
// side that will read it) puts it.  head: l.total_bytes bytes.
inline void spicey_pss_head(const SpiceyPssLayout &l, SpiceyPssArgs &A, const int32_t *ist, char *head, char *base) {
  memset(head, 0, (size_t)l.total_bytes);
  A.ist = ist ? (const int32_t *)(base + l.off_ist) : nullptr;
  if (ist) memcpy(head + l.off_ist, ist, (size_t)l.n_inst * sizeof(int32_t));
  memcpy(head, &A, sizeof(A));
}

#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H)
// The design kernel, enqueued on `st` behind a copy of `A` (HOST, from spicey_pss_judge) into the head of d_work.  The device
// must be current.  No synchronisation.
hipError_t spicey_launch_pss_design(int device, const SpiceyPssArgs &A, void *d_work, hipStream_t st);
// The update kernel, one workgroup per circuit, behind a copy of `A` and of ist [n_inst] (HOST, or null) into d_work.
hipError_t spicey_launch_pss_update(int device, const SpiceyPssArgs &A, const int32_t *ist, void *d_work, hipStream_t st);
#endif
