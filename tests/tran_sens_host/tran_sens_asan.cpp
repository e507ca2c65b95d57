// Stand-alone program (its own main, no Python, no GPU) that drives the CPU harness of the sensitivities and corners of transient
// measurements under the host sanitizers (`make asan`): every buffer is a heap allocation of exactly the size the interface
// states, so a read or write past an end — of the value arrays, the levels, the rows, the workspace heads, the results — is
// reported.  It also checks what can be checked without a reference: the design's factors, counts, signs, sentinels after refusals.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../spicey_amd/csrc/tran_sens.h"

extern "C" int32_t spicey_ts_host_design(int32_t, int32_t, int32_t, int32_t, const double *, const double *, const double *, const SpiceyTranSensReq *, const int32_t *,
                                         const double *, const int8_t *, const double *, double *, double *, double *, int32_t, int64_t, char *, int32_t);
extern "C" int32_t spicey_ts_host_reduce(int32_t, const SpiceyMcRows *, const SpiceyMcScalar *, int32_t, const uint8_t *, const double *, const double *, int32_t, double *,
                                         double *, int8_t *, double *, int32_t, int64_t, int32_t, char *, int32_t);

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

SpiceyTranSensReq request(int32_t mode, int32_t nA) { return SpiceyTranSensReq{(int64_t)sizeof(SpiceyTranSensReq), mode, nA, {0, 0}}; }

void design_case(int32_t nR, int32_t nC, int32_t nL, int32_t nA) {
  const int32_t nE = nR + nC + nL, ni = 1 + 2 * nA;
  auto R = heap<double>((size_t)ni * nR), Cv = heap<double>((size_t)ni * nC), Lv = heap<double>((size_t)ni * nL);
  auto oR = heap<double>((size_t)ni * nR), oC = heap<double>((size_t)ni * nC), oL = heap<double>((size_t)ni * nL);
  for (size_t i = 0; i < (size_t)ni * nR; i++) R[i] = 1.0 + 1e3 * rnd();
  for (size_t i = 0; i < (size_t)ni * nC; i++) Cv[i] = 1e-9 * (1.0 + rnd());
  for (size_t i = 0; i < (size_t)ni * nL; i++) Lv[i] = 1e-6 * (1.0 + rnd());
  auto act = heap<int32_t>((size_t)nA);
  auto step = heap<double>((size_t)nA);
  for (int32_t a = 0; a < nA; a++) { act[a] = (int32_t)((int64_t)a * nE / nA); step[a] = 1e-3 * (1.0 + rnd()); }
  char err[256];
  SpiceyTranSensReq req = request(SPICEY_TS_ONE_AT_A_TIME, nA);
  int32_t rc = spicey_ts_host_design(ni, nR, nC, nL, nR ? R.get() : nullptr, nC ? Cv.get() : nullptr, nL ? Lv.get() : nullptr, &req, act.get(), step.get(), nullptr, nullptr,
                                     nR ? oR.get() : nullptr, nC ? oC.get() : nullptr, nL ? oL.get() : nullptr, 1, -1, err, 256);
  expect(rc == SPICEY_OK, "one-at-a-time design accepted");
  int64_t changed = 0;
  for (size_t i = 0; i < (size_t)ni * nR; i++) changed += oR[i] != R[i];
  for (size_t i = 0; i < (size_t)ni * nC; i++) changed += oC[i] != Cv[i];
  for (size_t i = 0; i < (size_t)ni * nL; i++) changed += oL[i] != Lv[i];
  expect(changed == 2 * (int64_t)nA, "one-at-a-time changes exactly one value per perturbed instance");
  // levels
  auto lvl = heap<int8_t>((size_t)ni * nE);
  auto tol = heap<double>((size_t)nE);
  for (size_t i = 0; i < (size_t)ni * nE; i++) lvl[i] = (int8_t)((int)(3.0 * rnd()) - 1);
  for (int32_t e = 0; e < nE; e++) { lvl[e] = 0; tol[e] = 0.2 * rnd(); }
  req = request(SPICEY_TS_LEVELS, 0);
  rc = spicey_ts_host_design(ni, nR, nC, nL, nR ? R.get() : nullptr, nC ? Cv.get() : nullptr, nL ? Lv.get() : nullptr, &req, nullptr, nullptr, lvl.get(), tol.get(),
                             nR ? oR.get() : nullptr, nC ? oC.get() : nullptr, nL ? oL.get() : nullptr, 1, -1, err, 256);
  expect(rc == SPICEY_OK, "levels design accepted");
  for (int32_t e = 0; e < nR; e++) expect(oR[e] == R[e], "a row of zero levels is the nominal circuit");
  for (size_t i = 0; i < (size_t)ni * nR; i++) expect(oR[i] >= 0.8 * R[i] && oR[i] <= 1.2 * R[i], "a levelled resistance stays within its tolerance");
  lvl[(size_t)ni * nE - 1] = 2;
  oL[0] = oC[0] = oR[0] = -7.0;
  rc = spicey_ts_host_design(ni, nR, nC, nL, R.get(), Cv.get(), Lv.get(), &req, nullptr, nullptr, lvl.get(), tol.get(), oR.get(), oC.get(), oL.get(), 1, -1, err, 256);
  expect(rc == SPICEY_ERR_BAD_DESC && strncmp(err, "tran sens: ", 11) == 0 && oR[0] == -7.0 && oC[0] == -7.0 && oL[0] == -7.0, "a level of 2 is refused and writes nothing");
}

void reduce_case(int32_t nA, int32_t n_scalar, int32_t threads, int mode) {
  const int32_t ni = 1 + 2 * nA;
  const SpiceyMcRows shape[3] = {{nullptr, 2, 8}, {nullptr, 1, 8}, {nullptr, 1, SPICEY_POWER_ROW}};
  std::unique_ptr<double[]> buf[3];
  SpiceyMcRows rows[3];
  for (int p = 0; p < 3; p++) {
    const size_t n = (size_t)ni * shape[p].n_rows * shape[p].stride;
    buf[p] = heap<double>(n);
    for (size_t i = 0; i < n; i++) buf[p][i] = 4.0 * rnd() - 2.0;
    rows[p] = SpiceyMcRows{buf[p].get(), shape[p].n_rows, shape[p].stride};
  }
  if (mode == 1)  // all NaN in what scalar 0 reads
    for (int32_t s = 0; s < ni; s++) buf[0][(size_t)s * 16 + 8 + 7] = NAN;
  auto sc = heap<SpiceyMcScalar>((size_t)n_scalar);
  memset(sc.get(), 0, sizeof(SpiceyMcScalar) * (size_t)n_scalar);
  for (int32_t j = 0; j < n_scalar; j++) {
    sc[j].n_ins = 1;
    sc[j].ins[0] = j % 3 == 0 ? SpiceyMcIns{SPICEY_MCOP_FIELD, 0, 1, 7, 0.0} : j % 3 == 1 ? SpiceyMcIns{SPICEY_MCOP_FIELD, 1, 0, 7, 0.0}
                                                                                          : SpiceyMcIns{SPICEY_MCOP_FIELD, 2, 0, SPICEY_POWER_ROW - 1, 0.0};
  }
  auto valid = heap<uint8_t>((size_t)ni);
  for (int32_t s = 0; s < ni; s++) valid[s] = mode == 2 ? (s % 5 != 3) : 1;
  auto step = heap<double>((size_t)nA), tol = heap<double>((size_t)nA);
  for (int32_t a = 0; a < nA; a++) { step[a] = 1e-3 * (1.0 + rnd()); tol[a] = 0.1 * rnd(); }
  auto x = heap<double>((size_t)ni * n_scalar), sens = heap<double>((size_t)n_scalar * nA * 2), bound = heap<double>((size_t)n_scalar * SPICEY_TS_BOUND_ROW);
  auto sign = heap<int8_t>((size_t)n_scalar * nA);
  char err[256];
  const int32_t rc = spicey_ts_host_reduce(ni, rows, sc.get(), n_scalar, mode == 2 ? valid.get() : nullptr, step.get(), tol.get(), nA, x.get(), sens.get(), sign.get(),
                                           bound.get(), 1, -1, threads, err, 256);
  expect(rc == SPICEY_OK, "reduce accepted");
  if (rc != SPICEY_OK) { fprintf(stderr, "  %s\n", err); return; }
  for (int32_t j = 0; j < n_scalar; j++) {
    const double *b = bound.get() + (size_t)j * SPICEY_TS_BOUND_ROW;
    int32_t n_num = 0;
    for (int32_t a = 0; a < nA; a++) {
      const double d = sens[2 * ((size_t)j * nA + a)];
      const int8_t s = sign[(size_t)j * nA + a];
      n_num += !std::isnan(d);
      expect(std::isnan(d) ? s == 0 : s == (d > 0) - (d < 0), "the sign is that of d");
    }
    expect(b[3] == (double)n_num && b[7] == 0.0 && b[6] >= 0 && b[6] <= b[3] && b[1] >= 0 && b[2] >= 0, "counts of a bound row");
    expect(n_num ? (b[4] >= 0 && b[4] < nA && b[5] >= 0) : (b[4] == -1.0 && b[5] == 0.0 && b[1] == 0.0), "the dominant element");
  }
  if (mode == 1) expect(bound[3] == 0.0 && std::isnan(bound[0]), "mode 1: scalar 0 has no number");
}

void refusals() {
  double rowbuf[3 * 16] = {0};
  const SpiceyMcRows rows[3] = {{rowbuf, 1, 8}, {nullptr, 0, 8}, {rowbuf, 1, SPICEY_POWER_ROW}};
  SpiceyMcScalar P;
  memset(&P, 0, sizeof(P));
  P.n_ins = 1;
  P.ins[0] = SpiceyMcIns{SPICEY_MCOP_FIELD, 0, 0, 0, 0.0};
  double x[3] = {-7.0, -7.0, -7.0}, sens[2] = {-7.0, -7.0}, bound[8] = {-7.0};
  int8_t sign[1] = {-7};
  double step[1] = {1e-3}, tol[1] = {0.1};
  char err[256];
  const auto call = [&](int32_t ni, int32_t nA, int64_t wb) {
    return spicey_ts_host_reduce(ni, rows, &P, 1, nullptr, step, tol, nA, x, sens, sign, bound, 1, wb, 0, err, 256);
  };
  const auto refused = [&](int32_t rc) { return rc == SPICEY_ERR_BAD_DESC && strncmp(err, "tran sens: ", 11) == 0 && x[0] == -7.0 && sens[0] == -7.0 && sign[0] == -7 && bound[0] == -7.0; };
  expect(refused(call(4, 1, -1)), "n_inst != 1 + 2 nA");
  expect(refused(call(3, 1, 8)), "small workspace");
  step[0] = 1.0;
  expect(refused(call(3, 1, -1)), "step = 1");
  step[0] = NAN;
  expect(refused(call(3, 1, -1)), "step NaN");
  step[0] = 1e-3; tol[0] = -0.1;
  expect(refused(call(3, 1, -1)), "negative tolerance");
  tol[0] = 0.1; P.ins[0].row = 3;
  expect(refused(call(3, 1, -1)), "a FIELD's row out of range");
  P.ins[0].row = 0;
  expect(call(3, 1, -1) == SPICEY_OK && x[0] == 0.0 && sens[0] == 0.0 && sign[0] == 0 && bound[3] == 1.0, "a good one");
}
}  // namespace

int main() {
  design_case(1, 0, 0, 1);
  design_case(3, 2, 1, 2);
  design_case(40, 30, 60, 130);
  design_case(0, 63, 2, 65);
  for (int32_t nA : {1, 2, 63, 64, 65, 130})
    for (int32_t ns : {1, 5})
      for (int32_t threads : {0, 64, 256})
        for (int mode : {0, 1, 2}) reduce_case(nA, ns, threads, mode);
  refusals();
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("tran_sens_asan: ok\n");
  return 0;
}
