// Stand-alone program (its own main, no Python, no GPU) that drives the CPU harness of the periodic steady state under the host
// sanitizers (`make asan`): every buffer is a heap allocation of exactly the size the interface states, and the matrix has
// exactly the bytes of the device's dynamic LDS, so a read or write past an end — of the state arrays, the base, the rows, the
// matrix, the workspace head — is reported.  It also checks what can be checked without a reference: a linear period map is
// solved in one update, counts, sentinels after refusals.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../spicey_amd/csrc/pss.h"

extern "C" int32_t spicey_pss_host_design(int32_t, int32_t, int32_t, int32_t, const SpiceyPssReq *, int32_t, const double *, const int32_t *, double *, double *, double *,
                                          double *, int32_t *, int32_t, int64_t, char *, int32_t);
extern "C" int32_t spicey_pss_host_update(int32_t, int32_t, int32_t, int32_t, const SpiceyPssReq *, const int32_t *, double *, int32_t *, const double *, const double *,
                                          const double *, const double *, const int32_t *, double *, double *, int32_t *, int32_t, int64_t, int32_t, char *, int32_t);

namespace {
int failures = 0;
void expect(bool ok, const char *what) {
  if (!ok) { fprintf(stderr, "FAILED: %s\n", what); failures++; }
}
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double rnd() {  // xorshift: [0, 1)
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}
template <class T>
std::unique_ptr<T[]> heap(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }

SpiceyPssReq request(int32_t n_ckt, int32_t method) {
  return SpiceyPssReq{(int64_t)sizeof(SpiceyPssReq), n_ckt, method, 20, 0, 1.0, 1e-6, 1e-9, 1e-12, 1e-6, 1.0, 1e-3, 0};
}

// entry a of instance s in the three state arrays
double &entry(double *Cv, double *Li, double *Dv, int32_t nC, int32_t nL, int32_t nD, int64_t s, int32_t a) {
  if (a < nC) return Cv[s * nC + a];
  if (a < nC + nL) return Li[s * nL + (a - nC)];
  return Dv[s * nD + (a - nC - nL)];
}

// An affine, contracting period map applied to the designed states: one Newton update lands on its fixed point.
void newton_case(int32_t nC, int32_t nL, int32_t nD, int32_t nS, int32_t n_ckt, int32_t threads) {
  const int32_t nX = nC + nL + nD, W = 1 + nX;
  const int64_t ni = (int64_t)n_ckt * W;
  auto base = heap<double>((size_t)n_ckt * nX), h = heap<double>((size_t)n_ckt * nX), delta = heap<double>((size_t)n_ckt * nX);
  auto base_on = heap<int32_t>((size_t)n_ckt * nS), Son = heap<int32_t>((size_t)ni * nS), done = heap<int32_t>((size_t)n_ckt);
  auto Cv = heap<double>((size_t)ni * nC), Li = heap<double>((size_t)ni * nL), Dv = heap<double>((size_t)ni * nD);
  auto rows = heap<double>((size_t)n_ckt * SPICEY_PSS_ROW);
  for (size_t i = 0; i < (size_t)n_ckt * nX; i++) base[i] = 2.0 * rnd() - 1.0;
  for (size_t i = 0; i < (size_t)n_ckt * nS; i++) base_on[i] = rnd() < 0.5;
  for (int32_t c = 0; c < n_ckt; c++) done[c] = 0;
  char err[256];
  SpiceyPssReq req = request(n_ckt, SPICEY_PSS_NEWTON);
  int32_t rc = spicey_pss_host_design(nC, nL, nD, nS, &req, 1, base.get(), nS ? base_on.get() : nullptr, h.get(), nC ? Cv.get() : nullptr, nL ? Li.get() : nullptr,
                                      nD ? Dv.get() : nullptr, nS ? Son.get() : nullptr, 1, -1, err, 256);
  expect(rc == SPICEY_OK, "design accepted");
  if (rc != SPICEY_OK) { fprintf(stderr, "  %s\n", err); return; }
  int64_t moved = 0;
  for (int64_t s = 0; s < ni; s++)
    for (int32_t a = 0; a < nX; a++) moved += entry(Cv.get(), Li.get(), Dv.get(), nC, nL, nD, s, a) != base[(s / W) * nX + a];
  expect(moved == (int64_t)n_ckt * nX, "the design moves exactly one entry per perturbed instance");
  for (size_t i = 0; i < (size_t)n_ckt * nX; i++) expect(h[i] > 0.0, "h_eff is positive");
  // Phi(x) = J x + g with |J| <= 0.9 / nX, applied in place
  std::vector<double> J((size_t)nX * nX), g((size_t)nX), x((size_t)nX), fix((size_t)n_ckt * nX);
  for (int32_t c = 0; c < n_ckt; c++) {
    for (double &v : J) v = (2.0 * rnd() - 1.0) * 0.9 / nX;
    for (double &v : g) v = 2.0 * rnd() - 1.0;
    for (int32_t j = 0; j < W; j++) {
      const int64_t s = (int64_t)c * W + j;
      for (int32_t a = 0; a < nX; a++) x[(size_t)a] = entry(Cv.get(), Li.get(), Dv.get(), nC, nL, nD, s, a);
      for (int32_t i = 0; i < nX; i++) {
        double v = g[(size_t)i];
        for (int32_t a = 0; a < nX; a++) v += J[(size_t)i * nX + a] * x[(size_t)a];
        entry(Cv.get(), Li.get(), Dv.get(), nC, nL, nD, s, i) = v;
      }
    }
    // the fixed point by iteration (a contraction of 0.9)
    std::vector<double> f(g), f2((size_t)nX);
    for (int it = 0; it < 400; it++) {
      for (int32_t i = 0; i < nX; i++) {
        double v = g[(size_t)i];
        for (int32_t a = 0; a < nX; a++) v += J[(size_t)i * nX + a] * f[(size_t)a];
        f2[(size_t)i] = v;
      }
      f = f2;
    }
    for (int32_t a = 0; a < nX; a++) fix[(size_t)c * nX + a] = f[(size_t)a];
  }
  rc = spicey_pss_host_update(nC, nL, nD, nS, &req, nullptr, base.get(), nS ? base_on.get() : nullptr, h.get(), nC ? Cv.get() : nullptr, nL ? Li.get() : nullptr,
                              nD ? Dv.get() : nullptr, nS ? Son.get() : nullptr, delta.get(), rows.get(), done.get(), 1, -1, threads, err, 256);
  expect(rc == SPICEY_OK, "update accepted");
  for (int32_t c = 0; c < n_ckt; c++) {
    const double *r = rows.get() + (size_t)c * SPICEY_PSS_ROW;
    expect(r[3] == 1.0 && r[7] == 0.0 && done[c] == 0 && r[2] == 0.0 && r[6] == 0.0 && r[5] > 0.0 && r[5] <= 2.0, "a row of a circuit that moved");
    for (int32_t a = 0; a < nX; a++) expect(std::fabs(base[(size_t)c * nX + a] - fix[(size_t)c * nX + a]) < 1e-6, "one update reaches the fixed point of a linear map");
  }
}

void settle_case(int32_t nX, int32_t n_ckt) {  // more states than the Newton update takes: capacitors only
  auto base = heap<double>((size_t)n_ckt * nX), Cv = heap<double>((size_t)n_ckt * nX), rows = heap<double>((size_t)n_ckt * SPICEY_PSS_ROW);
  auto done = heap<int32_t>((size_t)n_ckt);
  for (size_t i = 0; i < (size_t)n_ckt * nX; i++) { base[i] = rnd(); Cv[i] = rnd(); }
  for (int32_t c = 0; c < n_ckt; c++) done[c] = 0;
  char err[256];
  SpiceyPssReq req = request(n_ckt, SPICEY_PSS_SETTLE);
  const int32_t rc = spicey_pss_host_update(nX, 0, 0, 0, &req, nullptr, base.get(), nullptr, nullptr, Cv.get(), nullptr, nullptr, nullptr, nullptr, rows.get(), done.get(), 1, -1,
                                            0, err, 256);
  expect(rc == SPICEY_OK, "settle accepted");
  for (size_t i = 0; i < (size_t)n_ckt * nX; i++) expect(base[i] == Cv[i], "settle takes the end state");
}

void refusals() {
  double base[2] = {-7.0, -7.0}, h[2] = {-7.0, -7.0}, Cv[6] = {0}, rows[8] = {-7.0};
  int32_t done[1] = {0};
  char err[256];
  SpiceyPssReq req = request(1, SPICEY_PSS_NEWTON);
  const auto call = [&](int32_t nC, int64_t wb) {
    return spicey_pss_host_update(nC, 0, 0, 0, &req, nullptr, base, nullptr, h, Cv, nullptr, nullptr, nullptr, nullptr, rows, done, 1, wb, 0, err, 256);
  };
  const auto refused = [&](int32_t rc) { return rc == SPICEY_ERR_BAD_DESC && strncmp(err, "pss: ", 5) == 0 && base[0] == -7.0 && rows[0] == -7.0 && done[0] == 0; };
  expect(refused(call(129, -1)) && strstr(err, "settle") != nullptr, "nX = 129 names settle");
  expect(refused(call(0, -1)), "nX = 0");
  expect(refused(call(2, 8)), "small workspace");
  req.reltol = 0.0;
  expect(refused(call(2, -1)), "reltol = 0");
  req.reltol = 1e-6; req.damping = 1.5;
  expect(refused(call(2, -1)), "damping > 1");
  req.damping = 1.0; req.struct_bytes = 80;
  expect(refused(call(2, -1)), "struct_bytes");
}
}  // namespace

int main() {
  for (int32_t threads : {0, 64, 192})
    for (int32_t n_ckt : {1, 3}) {
      newton_case(1, 0, 0, 0, n_ckt, threads);
      newton_case(1, 1, 0, 1, n_ckt, threads);
      newton_case(21, 21, 21, 2, n_ckt, threads);
      newton_case(22, 21, 21, 1, n_ckt, threads);
      newton_case(22, 22, 21, 3, n_ckt, threads);
    }
  newton_case(43, 43, 42, 2, 2, 0);
  settle_case(300, 2);
  refusals();
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("pss_asan: ok\n");
  return 0;
}
