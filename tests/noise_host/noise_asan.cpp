// Stand-alone program for the host sanitizers (`make asan`): the harness's injected sweep — per-solve and resident, threads
// in both orders — and its reduction on an R-C ladder with a floating source, sizes chosen so that rows, lanes and windows
// have ragged ends (67 resistors: one more than a wave plus two; 5 frequencies).  Checks reciprocity on the way: i(V1) of the
// injected sweep against v(out) of the driven one.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/spicey_hip.h"

extern "C" int32_t spicey_noise_host_run(int32_t, int64_t, const double *, int32_t, const double *, int32_t, const double *, int32_t, const double *,
                                         const SpiceyAcNoiseReq *, double *, double *, double *, int32_t, int64_t, char *, int32_t);
extern "C" int32_t spicey_noise_host_sweep(const SpiceyDesc *, int32_t, int64_t, const double *, const double *, int32_t, int32_t, double, double, double *, double *,
                                           int32_t, int32_t, int32_t *, int32_t *, int32_t *);

int main() {
  const int n = 66;  // nodes 1 .. n in a chain, V1 between nodes 1 and 2 (floating), R to ground at node 1
  std::vector<int32_t> Rn1, Rn2, Cn1, Cn2;
  std::vector<double> Rv, Cv;
  Rn1.push_back(1); Rn2.push_back(0); Rv.push_back(50.0);
  for (int k = 2; k < n; k++) { Rn1.push_back(k); Rn2.push_back(k + 1); Rv.push_back(100.0 + 3.0 * k); }
  Rn1.push_back(n); Rn2.push_back(0); Rv.push_back(2200.0);
  Rn1.push_back(7); Rn2.push_back(0); Rv.push_back(910.0);
  for (int k = 2; k <= n; k++) { Cn1.push_back(k); Cn2.push_back(0); Cv.push_back(1e-9 * (1.0 + 0.01 * k)); }
  const int32_t Vn1 = 1, Vn2 = 2;
  const int nR = (int)Rv.size(), nC = (int)Cv.size(), nCur = nR + nC + 1;
  std::vector<double> cvp((size_t)nC, 0.0);
  SpiceyDesc d{};
  d.abi_version = SPICEY_ABI_VERSION;
  d.n_nodes = n; d.n_inst = 1; d.nR = nR; d.nC = nC; d.nV = 1;
  d.R_n1 = Rn1.data(); d.R_n2 = Rn2.data(); d.R_val = Rv.data();
  d.C_n1 = Cn1.data(); d.C_n2 = Cn2.data(); d.C_val = Cv.data(); d.C_vprev = cvp.data();
  d.V_n1 = &Vn1; d.V_n2 = &Vn2;
  const std::vector<double> freqs = {1e3, 3e4, 1e5, 2e6, 5e7};
  const int64_t nf = (int64_t)freqs.size();
  const int32_t out = 40;
  const double one[2] = {1.0, 0.0};
  std::vector<double> dv((size_t)nf * n * 2), di((size_t)nf * nCur * 2), first;
  if (spicey_noise_host_sweep(&d, 64, nf, freqs.data(), one, 0, 0, 0.0, 0.0, dv.data(), di.data(), 0, 1, nullptr, nullptr, nullptr) != SPICEY_OK) return 2;
  double worst = 0.0;
  for (int mode = 0; mode < 4; mode++) {
    std::vector<double> v((size_t)nf * n * 2), i((size_t)nf * nCur * 2);
    int32_t pos[4];
    if (spicey_noise_host_sweep(&d, 64, nf, freqs.data(), nullptr, out, 0, 1.0, 0.0, v.data(), i.data(), mode, 3, nullptr, pos, nullptr) != SPICEY_OK) return 3;
    for (int64_t k = 0; k < nf; k++) {
      const double *g = &i[((size_t)k * nCur + (size_t)(nR + nC)) * 2], *r = &dv[((size_t)k * n + (size_t)(out - 1)) * 2];
      const double m = std::hypot(g[0] - r[0], g[1] - r[1]) / (1e-9 * std::hypot(r[0], r[1]) + 1e-12);
      if (m > worst) worst = m;
    }
    if (mode == 0) first = i;
    std::vector<double> spec((size_t)nf * 4), contrib((size_t)nR), total(2);
    SpiceyAcNoiseReq q{};
    q.struct_bytes = (int64_t)sizeof(q);
    q.out_p = out - 1; q.out_n = -1; q.in_col = nR + nC; q.k_from = mode == 3 ? nf - 2 : 0; q.k_to = -1; q.kt4 = 4 * 1.380649e-23 * 300.15;
    char err[200];
    if (spicey_noise_host_run(1, nf, v.data(), n, i.data(), nCur, Rv.data(), nR, freqs.data(), &q, spec.data(), contrib.data(), total.data(), 1, -1, err, 200) !=
        SPICEY_OK) {
      fprintf(stderr, "%s\n", err);
      return 4;
    }
    double sum = 0.0;
    for (double c : contrib) sum += c;
    if (!(std::fabs(sum - total[0]) <= 1e-12 * total[0]) || !(total[0] > 0.0)) return 5;
  }
  printf("noise_asan ok: reciprocity %.3g of the bar\n", worst);
  return worst <= 1.0 ? 0 : 6;
}
