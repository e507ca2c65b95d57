// Stand-alone program for the host sanitizers (`make asan`): the harness's reduction on buffers of exactly the stated sizes —
// nE = 1 (one resistor) and nE = 130 (60 + 40 + 30: two full waves and two lanes, kind borders inside a wave), 3 instances, 5
// frequencies of which the first is 0, with and without d_full, the whole window and the last two frequencies — and every
// refusal of the judge, after which the results must still hold their sentinel.  Checks on the way that d_peak does not
// depend on d_full and that the peak rows are rows of d_full.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spicey_hip.h"

extern "C" int32_t spicey_sens_host_run(int32_t, int64_t, const double *, int32_t, const double *, const double *, int32_t, const double *, const double *,
                                        const double *, const double *, const double *, const SpiceyAcSensReq *, double *, double *, double *, int32_t, int64_t,
                                        char *, int32_t);

namespace {
uint64_t g_state = 88172645463325252ull;
double rnd() {  // xorshift, in (-1, 1) without 0
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return ((double)(g_state >> 11) + 0.5) / 4503599627370496.0 - 1.0;
}
std::vector<double> fill(size_t n, double scale) {
  std::vector<double> v(n);
  for (double &x : v) x = scale * rnd();
  return v;
}
std::vector<double> positive(size_t n, double scale) {
  std::vector<double> v(n);
  for (double &x : v) x = scale * (1.5 + rnd());
  return v;
}
const double SENTINEL = -7.25;
}  // namespace

int main() {
  const int32_t ni = 3, n_v = 3;
  const int64_t nf = 5;
  const std::vector<double> freqs = {0.0, 1e3, 3e4, 1e5, 2e6};
  const int shapes[2][3] = {{1, 0, 0}, {60, 40, 30}};
  char err[200];
  int runs = 0;
  for (const auto &sh : shapes) {
    const int32_t nR = sh[0], nC = sh[1], nL = sh[2], nE = nR + nC + nL, n_i = nE;  // (no spare column: the last read is the buffer's last)
    const std::vector<double> v = fill((size_t)ni * nf * n_v * 2, 3.0), id = fill((size_t)ni * nf * n_i * 2, 1e-3), ix = fill((size_t)ni * nf * n_i * 2, 2.0);
    const std::vector<double> R = positive((size_t)ni * nR, 1e3), Cv = positive((size_t)ni * nC, 1e-9), Lv = positive((size_t)ni * nL, 1e-3);
    std::vector<double> tol = positive((size_t)nE, 0.01);
    tol[(size_t)nE / 2] = 0.0;
    std::vector<double> peak_ref;
    for (int pass = 0; pass < 4; pass++) {
      const bool with_full = (pass & 1) != 0, tail = (pass & 2) != 0;
      SpiceyAcSensReq q{};
      q.struct_bytes = (int64_t)sizeof(q);
      q.out_p = 1; q.out_n = tail ? -1 : 2; q.nR = nR; q.nC = nC; q.nL = nL; q.k_from = tail ? nf - 2 : 0; q.k_to = -1;
      std::vector<double> spec((size_t)ni * nf * 6, SENTINEL), peak((size_t)ni * nE * 4, SENTINEL), full((size_t)ni * nf * nE * 2, SENTINEL);
      if (spicey_sens_host_run(ni, nf, v.data(), n_v, id.data(), ix.data(), n_i, nR ? R.data() : nullptr, nC ? Cv.data() : nullptr, nL ? Lv.data() : nullptr,
                               tol.data(), freqs.data(), &q, spec.data(), peak.data(), with_full ? full.data() : nullptr, 1, -1, err, 200) != SPICEY_OK) {
        fprintf(stderr, "%s\n", err);
        return 2;
      }
      runs++;
      for (double x : spec) if (x == SENTINEL) return 3;
      for (double x : peak) if (x == SENTINEL) return 3;
      if (!with_full) peak_ref = peak;
      else {
        if (memcmp(peak_ref.data(), peak.data(), peak.size() * sizeof(double)) != 0) return 4;
        for (int32_t in = 0; in < ni; in++)
          for (int32_t e = 0; e < nE; e++) {
            const double *p = &peak[((size_t)in * nE + e) * 4];
            const int64_t km = (int64_t)p[1], kp = (int64_t)p[3];
            if (km < q.k_from || km >= nf || kp < q.k_from || kp >= nf) return 5;
            const double m = full[(((size_t)in * nf + km) * nE + e) * 2], ph = full[(((size_t)in * nf + kp) * nE + e) * 2 + 1];
            if (memcmp(&m, &p[0], 8) != 0 || memcmp(&ph, &p[2], 8) != 0) return 6;
          }
        // the capacitors' rows at f = 0 are +0 / d: zero
        for (int32_t e = nR; e < nR + nC; e++)
          if (full[((size_t)0 * nE + e) * 2] != 0.0 || full[((size_t)0 * nE + e) * 2 + 1] != 0.0) return 7;
      }
    }
    // the refusals: nothing is written
    int refused = 0;
    auto refuse = [&](SpiceyAcSensReq q, const double *tl, int32_t n_inst, int32_t have_out, int64_t wb, const char *text) {
      std::vector<double> spec((size_t)ni * nf * 6, SENTINEL), peak((size_t)ni * nE * 4, SENTINEL);
      err[0] = 0;
      const int32_t rc = spicey_sens_host_run(n_inst, nf, v.data(), n_v, id.data(), ix.data(), n_i, R.data(), Cv.data(), Lv.data(), tl, freqs.data(), &q, spec.data(),
                                              peak.data(), nullptr, have_out, wb, err, 200);
      bool clean = rc == SPICEY_ERR_BAD_DESC && strstr(err, "sens") && strstr(err, text);
      for (double x : spec) clean = clean && x == SENTINEL;
      for (double x : peak) clean = clean && x == SENTINEL;
      if (!clean) fprintf(stderr, "refusal '%s' went wrong: rc %d, text '%s'\n", text, rc, err);
      refused += clean;
    };
    SpiceyAcSensReq ok{};
    ok.struct_bytes = (int64_t)sizeof(ok);
    ok.out_p = 0; ok.out_n = -1; ok.nR = nR; ok.nC = nC; ok.nL = nL; ok.k_from = 0; ok.k_to = -1;
    SpiceyAcSensReq q;
    q = ok; q.out_p = n_v; refuse(q, tol.data(), ni, 1, -1, "column out of range");
    q = ok; q.out_n = 0; refuse(q, tol.data(), ni, 1, -1, "one node twice");
    q = ok; q.k_from = 3; q.k_to = 2; refuse(q, tol.data(), ni, 1, -1, "window");
    q = ok; q.k_to = nf; refuse(q, tol.data(), ni, 1, -1, "window");
    q = ok; q.reserved = 1; refuse(q, tol.data(), ni, 1, -1, "reserved");
    q = ok; q.struct_bytes = 8; refuse(q, tol.data(), ni, 1, -1, "struct_bytes");
    q = ok; q.nR = nR + 1; refuse(q, tol.data(), ni, 1, -1, "exceeds");
    q = ok; q.nR = 0; q.nC = 0; q.nL = 0; refuse(q, tol.data(), ni, 1, -1, "no element");
    q = ok; q.nC = -1; refuse(q, tol.data(), ni, 1, -1, "bad counts");
    refuse(ok, tol.data(), 0, 1, -1, "bad counts");
    refuse(ok, tol.data(), ni, 0, -1, "null buffer");
    refuse(ok, nullptr, ni, 1, -1, "null buffer");
    refuse(ok, tol.data(), ni, 1, 8, "workspace");
    std::vector<double> bad = tol;
    bad[(size_t)nE - 1] = -1e-3; refuse(ok, bad.data(), ni, 1, -1, "tolerance");
    bad[(size_t)nE - 1] = NAN; refuse(ok, bad.data(), ni, 1, -1, "tolerance");
    bad[(size_t)nE - 1] = INFINITY; refuse(ok, bad.data(), ni, 1, -1, "tolerance");
    if (refused != 16) return 8;
  }
  printf("sens_asan ok: %d reductions at nE = 1 and 130, 32 refusals\n", runs);
  return 0;
}
