// CPU harness of the AC measurements: ac_measure_exec.h — the code the kernel of spicey_amd/csrc/ac_measure.hip runs —
// through an emulation of its launch: `waves` waves take the (instance, request) pairs w, w + waves, ...; the `lanes` lanes
// of a wave each walk their share of the window (spicey_acm_lane), meet in the kernel's butterfly (lane l combines with
// lane l ^ off for off = lanes / 2 .. 1) and lane 0 writes the row (spicey_acm_finish).  Compiled with -ffp-contract=off
// like the kernel's translation unit, so the results are the GPU's bit for bit.
#include <cstring>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/ac_measure_exec.h"

extern "C" int32_t spicey_acm_host_lanes(void) { return SPICEY_ACM_LANES; }
extern "C" int64_t spicey_acm_host_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t n_req) { return spicey_acm_workspace_bytes(n_inst, n_freq, n_req); }

// lanes: a power of two, 1 .. 64; waves: waves launched, 0 = one per pair.  Returns SPICEY_OK, SPICEY_ERR_BAD_DESC (text in
// err), or -1 when the lanes of a wave disagree after the butterfly (the combine would not be order-free).
extern "C" int32_t spicey_acm_host_run(int32_t n_inst, int64_t n_freq, const double *v, int32_t n_v, const double *i, int32_t n_i, const SpiceyAcMeasReq *reqs,
                                       int32_t n_req, double *meas, int32_t lanes, int64_t waves, char *err, int32_t err_cap) {
  std::string e;
  std::vector<SpiceyAcMeasDevReq> table;
  bool ok = n_inst > 0 && lanes >= 1 && lanes <= 64 && (lanes & (lanes - 1)) == 0 && waves >= 0;
  if (!ok) e = "ac measure: bad arguments";
  ok = ok && spicey_acm_plan(reqs, n_req, n_freq, v ? n_v : 0, n_i, i != nullptr, table, e);
  if (!ok) {
    if (err && err_cap > 0) { strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return SPICEY_ERR_BAD_DESC;
  }
  const SpiceyAcmBufs B{v, i, n_v, n_i, n_freq};
  const int64_t total = (int64_t)n_inst * n_req;
  if (waves == 0 || waves > total) waves = total;
  std::vector<SpiceyAcmPart> p((size_t)lanes), nx((size_t)lanes);
  for (int64_t w = 0; w < waves; w++)
    for (int64_t idx = w; idx < total; idx += waves) {
      const int64_t inst = idx / n_req;
      const SpiceyAcMeasDevReq q = table[(size_t)(idx - inst * n_req)];
      const double thr = spicey_acm_thr(B, q, inst);
      for (int32_t l = 0; l < lanes; l++) p[(size_t)l] = spicey_acm_lane(B, q, inst, l, lanes, thr);
      for (int32_t off = lanes / 2; off > 0; off >>= 1) {
        for (int32_t l = 0; l < lanes; l++) {
          nx[(size_t)l] = p[(size_t)l];
          spicey_acm_combine(q.kind, nx[(size_t)l], p[(size_t)(l ^ off)]);
        }
        p.swap(nx);
      }
      for (int32_t l = 1; l < lanes; l++) {
        const SpiceyAcmPart &a = p[0], &b = p[(size_t)l];
        if (a.k0 != b.k0 || a.k1 != b.k1 || a.cnt != b.cnt || (q.kind == 0 && a.k0 != SPICEY_ACM_NONE && (memcmp(&a.v0, &b.v0, 8) || memcmp(&a.v1, &b.v1, 8))))
          return -1;
      }
      spicey_acm_finish(B, q, inst, p[0], thr, meas + (inst * n_req + q.orig) * 8);
    }
  return SPICEY_OK;
}
