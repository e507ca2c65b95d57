// Stand-alone program (its own main, no Python, no GPU) that drives the CPU harness of the element sizing under the host
// sanitizers (`make asan`): every buffer is a heap allocation of exactly the size the interface states, the workspace has exactly
// spicey_fit_bytes bytes and the matrix exactly the bytes of the device's dynamic LDS, so a read or write past an end — of the
// value arrays, the gains, x, the rows, the matrix, the workspace — is reported.  It also checks what can be checked without a
// reference: a linear model with lambda0 = 0 is solved in one step and converges at the next, counts, sentinels after refusals.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../spicey_amd/csrc/fit.h"

extern "C" int32_t spicey_fit_host_design(int32_t, int32_t, int32_t, const double *, const double *, const double *, const SpiceyFitReq *, const int32_t *, const double *,
                                          const double *, double *, double *, double *, char *, int64_t, char *, int32_t);
extern "C" int32_t spicey_fit_host_update(const SpiceyFitReq *, int32_t, int32_t, const double *, const double *, const double *, const SpiceyFitGoal *, const uint8_t *,
                                          const double *, double *, double *, int32_t *, char *, int64_t, int32_t, char *, int32_t);

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

SpiceyFitReq request(int32_t n_ckt, int32_t nA) {
  return SpiceyFitReq{(int64_t)sizeof(SpiceyFitReq), n_ckt, nA, 30, 0, 0.0, 10.0, 0.1, 1e12, 0.5, 1e-9, 1e-24, 1e-300, 0};
}

// x = B (g - 1) + t per circuit, with EQ goals at t: the scalars are linear in the gains, so with lambda0 = 0 one step lands on g = 1.
void linear_case(int32_t nA, int32_t n_scalar, int32_t n_ckt, int32_t threads) {
  const int32_t W = 1 + 2 * nA, nR = nA / 2, nC = nA - nR, nL = 1, nE = nR + nC + nL;
  const int64_t ni = (int64_t)n_ckt * W;
  auto R = heap<double>((size_t)ni * nR), C = heap<double>((size_t)ni * nC), L = heap<double>((size_t)ni * nL);
  auto oR = heap<double>((size_t)ni * nR), oC = heap<double>((size_t)ni * nC), oL = heap<double>((size_t)ni * nL);
  auto g = heap<double>((size_t)n_ckt * nA), lo = heap<double>((size_t)n_ckt * nA), hi = heap<double>((size_t)n_ckt * nA), step = heap<double>((size_t)nA);
  auto act = heap<int32_t>((size_t)nA);
  auto goals = heap<SpiceyFitGoal>((size_t)n_ckt * n_scalar);
  auto x = heap<double>((size_t)ni * n_scalar), rows = heap<double>((size_t)n_ckt * SPICEY_FIT_ROW);
  auto done = heap<int32_t>((size_t)n_ckt);
  const int64_t wb = spicey_fit_bytes(n_ckt, nA, n_scalar);
  auto work = heap<char>((size_t)wb);
  memset(work.get(), 0, (size_t)wb);
  for (size_t i = 0; i < (size_t)ni * nR; i++) R[i] = 1.0 + rnd();
  for (size_t i = 0; i < (size_t)ni * nC; i++) C[i] = 1.0 + rnd();
  for (size_t i = 0; i < (size_t)ni * nL; i++) L[i] = 1.0 + rnd();
  for (int32_t a = 0; a < nA; a++) { act[a] = a; step[a] = 1.0 / 1024.0; }  // (the inductor stays inactive)
  for (size_t i = 0; i < (size_t)n_ckt * nA; i++) { g[i] = 0.75 + 0.5 * rnd(); lo[i] = 0.01; hi[i] = 100.0; }
  for (int32_t c = 0; c < n_ckt; c++) done[c] = 0;
  std::vector<double> B((size_t)n_scalar * nA), t((size_t)n_scalar);
  for (double &b : B) b = 2.0 * rnd() - 1.0;
  for (int32_t j = 0; j < n_scalar; j++) {
    if (j < nA) B[(size_t)j * nA + j] += 4.0;  // (full column rank where n_scalar >= nA)
    t[(size_t)j] = rnd();
    for (int32_t c = 0; c < n_ckt; c++) goals[(size_t)c * n_scalar + j] = SpiceyFitGoal{SPICEY_FIT_EQ, 0, t[(size_t)j], 0.0, 1.0 + rnd()};
  }
  char err[256];
  SpiceyFitReq req = request(n_ckt, nA);
  if (n_scalar < nA) req.lambda0 = 1e-3;  // (fewer goals than unknowns: J^T J is singular, the damping alone makes the system regular)
  auto evaluate = [&]() {
    int32_t rc = spicey_fit_host_design(nR, nC, nL, nR ? R.get() : nullptr, C.get(), L.get(), &req, act.get(), step.get(), g.get(), nR ? oR.get() : nullptr, oC.get(),
                                        oL.get(), work.get(), wb, err, 256);
    expect(rc == SPICEY_OK, "design accepted");
    // the gains as the design applied them, read back from the value arrays
    for (int64_t s = 0; s < ni; s++)
      for (int32_t j = 0; j < n_scalar; j++) {
        double v = t[(size_t)j];
        for (int32_t a = 0; a < nA; a++) {
          const double gain = a < nR ? oR[s * nR + a] / R[s * nR + a] : oC[s * nC + (a - nR)] / C[s * nC + (a - nR)];
          v += B[(size_t)j * nA + a] * (gain - 1.0);
        }
        x[s * n_scalar + j] = v;
      }
    expect(oL[0] == L[0], "an inactive element keeps its value");
  };
  evaluate();
  int32_t rc = spicey_fit_host_update(&req, n_scalar, 1, step.get(), lo.get(), hi.get(), goals.get(), nullptr, x.get(), g.get(), rows.get(), done.get(), work.get(), wb,
                                      threads, err, 256);
  expect(rc == SPICEY_OK, "first update accepted");
  if (rc != SPICEY_OK) { fprintf(stderr, "  %s\n", err); return; }
  for (int32_t c = 0; c < n_ckt; c++) expect(rows[c * SPICEY_FIT_ROW + 3] == 1.0 && rows[c * SPICEY_FIT_ROW + 4] == 1.0, "first point accepted, moved");
  if (n_scalar >= nA)
    for (size_t i = 0; i < (size_t)n_ckt * nA; i++) expect(fabs(g[i] - 1.0) < 1e-6, "one Gauss-Newton step solves the linear model");
  evaluate();
  rc = spicey_fit_host_update(&req, n_scalar, 0, step.get(), lo.get(), hi.get(), goals.get(), nullptr, x.get(), g.get(), rows.get(), done.get(), work.get(), wb, threads, err,
                              256);
  expect(rc == SPICEY_OK, "second update accepted");
  if (n_scalar >= nA)
    for (int32_t c = 0; c < n_ckt; c++) expect(rows[c * SPICEY_FIT_ROW + 3] == 1.0 && rows[c * SPICEY_FIT_ROW] < 1e-12, "the cost fell to rounding");
}

void refusals() {
  double v[8] = {7, 7, 7, 7, 7, 7, 7, 7}, out[8] = {7, 7, 7, 7, 7, 7, 7, 7}, g[1] = {1.0}, step[1] = {0.5}, lo[1] = {0.5}, hi[1] = {2.0}, rows[8] = {7, 7, 7, 7, 7, 7, 7, 7};
  int32_t act[1] = {0}, done[1] = {0};
  SpiceyFitGoal goal{SPICEY_FIT_EQ, 0, 1.0, 0.0, 1.0};
  char err[256], work[8];
  SpiceyFitReq req = request(1, 1);
  int32_t rc = spicey_fit_host_design(1, 0, 0, v, nullptr, nullptr, &req, act, step, g, out, nullptr, nullptr, work, 8, err, 256);
  expect(rc == SPICEY_ERR_BAD_DESC && strstr(err, "workspace too small") && out[0] == 7, "a small workspace is refused, nothing written");
  rc = spicey_fit_host_update(&req, 1, 1, step, lo, hi, &goal, nullptr, v, g, rows, done, work, 8, 0, err, 256);
  expect(rc == SPICEY_ERR_BAD_DESC && strstr(err, "workspace too small") && rows[0] == 7 && g[0] == 1.0, "the update's too");
  req.nA = 129;
  rc = spicey_fit_host_update(&req, 1, 1, step, lo, hi, &goal, nullptr, v, g, rows, done, work, 8, 0, err, 256);
  expect(rc == SPICEY_ERR_BAD_DESC && strncmp(err, "fit: ", 5) == 0 && strstr(err, "128"), "nA = 129 is refused");
}
}  // namespace

int main() {
  for (int32_t nA : {1, 2, 5, 64, 65, 128})
    for (int32_t n_scalar : {1, 3, 70})
      for (int32_t n_ckt : {1, 3}) {
        if (nA == 128 && n_scalar == 70 && n_ckt == 3) continue;  // (minutes under the sanitizers, and no other path)
        linear_case(nA, n_scalar, n_ckt, nA == 5 ? 64 : 0);
      }
  linear_case(128, 130, 1, 0);
  refusals();
  expect(spicey_fit_lds_bytes(128) == 132096, "132 096 bytes of LDS at nA = 128");
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("fit_asan: all checks passed\n");
  return 0;
}
