// CPU harness of the spectrum pass: spectrum_exec.h — the code the kernel of spicey_amd/csrc/spectrum.hip runs — through an
// emulation of its workgroup: per launch of the plan (one per distinct N) workgroups of `threads` threads take the items
// blockIdx, blockIdx + grid, ..., and every phase of spicey_spec_item runs for all threads of the workgroup in turn before
// the next one starts (the barrier).  The judge, the plan and the tables are the library's (spectrum.h: spicey_spec_judge,
// spicey_spec_head).  Compiled with -ffp-contract=off like the kernel's translation unit, so the results are the GPU's bit
// for bit.  The planes and the candidates start as NaNs / -2: a slot that is read without having been written shows.
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/spectrum.h"

extern "C" int32_t spicey_spec_host_threads(void) { return SPICEY_SPEC_THREADS; }
extern "C" int64_t spicey_spec_host_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceySpecReq *reqs, int32_t n_req) {
  return spicey_spec_workspace_bytes(n_inst, n_points, reqs, n_req);
}
extern "C" int64_t spicey_spec_host_lds_bytes(int32_t log2n) { return (int64_t)spicey_spec_lds_bytes(log2n); }
// T[N/2][2] and w[N] as the library uploads them
extern "C" void spicey_spec_host_tables(int32_t log2n, double *T, double *w) {
  spicey_spec_twiddles(log2n, T);
  spicey_spec_hann(log2n, w);
}

// threads: a power of two, 1 .. 1024; grid: workgroups launched, 0 = one per item; work_bytes: what the caller claims its
// workspace holds (-1: exactly enough).  Returns SPICEY_OK or SPICEY_ERR_BAD_DESC (text in err; `out` untouched).
extern "C" int32_t spicey_spec_host_run(int32_t n_inst, int64_t n_points, double dt, const double *v, int32_t n_v, const double *i, int32_t n_i,
                                        const SpiceySpecReq *reqs, int32_t n_req, double *out, int32_t out_stride, int64_t work_bytes, int32_t threads,
                                        int64_t grid, char *err, int32_t err_cap) {
  std::string e;
  SpiceySpecPlan p;
  bool ok = threads >= 1 && threads <= 1024 && (threads & (threads - 1)) == 0 && grid >= 0;
  if (!ok) e = "spectrum: bad arguments";
  ok = ok && spicey_spec_judge(n_inst, n_points, dt, v != nullptr, n_v, i != nullptr, n_i, reqs, n_req, out != nullptr, out_stride,
                               work_bytes < 0 ? std::numeric_limits<int64_t>::max() : work_bytes, p, e);
  if (!ok) {
    if (err && err_cap > 0) { strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return SPICEY_ERR_BAD_DESC;
  }
  std::vector<unsigned char> head;
  spicey_spec_head(p, head);
  const SpiceySpecDevReq *table = (const SpiceySpecDevReq *)head.data();
  const int32_t *order = (const int32_t *)(head.data() + p.off_order);
  const double *tables = (const double *)(head.data() + p.off_tables);
  const auto par = [threads](auto f) {
    for (int32_t t = 0; t < threads; t++) f(t);
  };
  for (const SpiceySpecLaunch &L : p.launches) {
    const size_t N = (size_t)1 << L.log2n;
    const int64_t items = (int64_t)n_inst * L.count;
    const int64_t blocks = grid == 0 || grid > items ? items : grid;
    for (int64_t b = 0; b < blocks; b++) {
      // (a workgroup's LDS lives as long as the workgroup: what an item left is there when the next one starts)
      std::vector<double> planes(2 * N, std::numeric_limits<double>::quiet_NaN()), cand_p((size_t)threads, std::numeric_limits<double>::quiet_NaN());
      std::vector<int32_t> cand_k((size_t)threads, -2);
      for (int64_t item = b; item < items; item += blocks) {
        const int64_t inst = item / L.count;
        const int32_t r = order[L.first + (item - inst * L.count)];
        const SpiceySpecDevReq q = table[r];
        const int64_t n = q.signal ? n_i : n_v;
        const double *base = (q.signal ? i : v) + inst * n_points * n;
        spicey_spec_item(par, threads, q, tables, base, n, planes.data(), planes.data() + N, cand_p.data(), cand_k.data(),
                         out + (inst * n_req + r) * out_stride, out_stride);
      }
    }
  }
  return SPICEY_OK;
}
