// Stand-alone program (its own main, no Python, no GPU) that drives the CPU harness of the Monte Carlo of transient runs under
// the host sanitizers (`make asan`): every buffer is a heap allocation of exactly the size the interface states, so a read or
// write past an end — of the rows, the programs, the keys, the workspace head, the results — is reported.  It also checks what
// can be checked without a reference: counts, the order of the order statistics, sentinels after refusals.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../spicey_amd/csrc/tran_mc.h"

extern "C" int32_t spicey_tmc_host_draw(int32_t, int32_t, int32_t, int32_t, const double *, const double *, const double *, const double *, const double *,
                                        const SpiceyTranMcReq *, double *, double *, double *, int32_t, int64_t, char *, int32_t);
extern "C" int32_t spicey_tmc_host_reduce(int32_t, const SpiceyMcRows *, const SpiceyMcScalar *, int32_t, const uint8_t *, const double *, const double *,
                                          const double *, int32_t, double *, double *, int64_t *, int32_t, int64_t, int32_t, char *, int32_t);

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

SpiceyMcIns ins(int32_t op, int32_t pass = 0, int32_t row = 0, int32_t field = 0, double c = 0.0) { return SpiceyMcIns{op, pass, row, field, c}; }
SpiceyMcScalar program(const std::vector<SpiceyMcIns> &v) {
  SpiceyMcScalar P;
  memset(&P, 0, sizeof(P));
  P.n_ins = (int32_t)v.size();
  for (size_t i = 0; i < v.size() && i < SPICEY_MC_SCALAR_INS; i++) P.ins[i] = v[i];
  return P;
}

void draw_case(int32_t ni, int32_t nR, int32_t nC, int32_t nL, int32_t log2K) {
  const int32_t nE = nR + nC + nL;
  const size_t K = (size_t)1 << log2K;
  auto R = heap<double>((size_t)ni * nR), Cv = heap<double>((size_t)ni * nC), Lv = heap<double>((size_t)ni * nL);
  auto oR = heap<double>((size_t)ni * nR), oC = heap<double>((size_t)ni * nC), oL = heap<double>((size_t)ni * nL);
  auto tol = heap<double>((size_t)nE), icdf = heap<double>(K + 1);
  for (size_t i = 0; i < (size_t)ni * nR; i++) R[i] = 1.0 + 1e3 * rnd();
  for (size_t i = 0; i < (size_t)ni * nC; i++) Cv[i] = 1e-9 * (1.0 + rnd());
  for (size_t i = 0; i < (size_t)ni * nL; i++) Lv[i] = 1e-6 * (1.0 + rnd());
  for (int32_t e = 0; e < nE; e++) tol[e] = 0.1 * rnd();
  for (size_t j = 0; j <= K; j++) icdf[j] = -1.0 + 2.0 * (double)j / (double)K;
  const SpiceyTranMcReq req{(int64_t)sizeof(SpiceyTranMcReq), log2K, 1, 12345u, 0};
  char err[256];
  const int32_t rc = spicey_tmc_host_draw(ni, nR, nC, nL, nR ? R.get() : nullptr, nC ? Cv.get() : nullptr, nL ? Lv.get() : nullptr, tol.get(), icdf.get(), &req,
                                          nR ? oR.get() : nullptr, nC ? oC.get() : nullptr, nL ? oL.get() : nullptr, 1, -1, err, 256);
  expect(rc == SPICEY_OK, "draw accepted");
  for (int32_t e = 0; e < nR; e++) expect(oR[e] == R[e], "sample 0 keeps the nominal resistance (ohms)");
  for (size_t i = 0; i < (size_t)ni * nR; i++) expect(oR[i] > 0.89 * R[i] && oR[i] < 1.11 * R[i], "a drawn resistance stays within its tolerance");
  SpiceyTranMcReq bad = req;
  bad.reserved = 1;
  oR[0] = -7.0;
  expect(spicey_tmc_host_draw(ni, nR, nC, nL, R.get(), Cv.get(), Lv.get(), tol.get(), icdf.get(), &bad, oR.get(), oC.get(), oL.get(), 1, -1, err, 256) == SPICEY_ERR_BAD_DESC &&
             strncmp(err, "tran mc: ", 9) == 0 && oR[0] == -7.0, "a nonzero reserved word is refused and writes nothing");
}

void reduce_case(int32_t ni, int32_t n_scalar, int32_t threads, int mode) {
  // rows of every pass with exactly the stated sizes: measure 2 rows, timing 1, power 1
  const SpiceyMcRows shape[3] = {{nullptr, 2, 8}, {nullptr, 1, 8}, {nullptr, 1, SPICEY_POWER_ROW}};
  std::unique_ptr<double[]> buf[3];
  SpiceyMcRows rows[3];
  for (int p = 0; p < 3; p++) {
    const size_t n = (size_t)ni * shape[p].n_rows * shape[p].stride;
    buf[p] = heap<double>(n);
    for (size_t i = 0; i < n; i++) buf[p][i] = 4.0 * rnd() - 2.0;
    rows[p] = SpiceyMcRows{buf[p].get(), shape[p].n_rows, shape[p].stride};
  }
  if (ni > 2) { buf[0][(size_t)1 * 16 + 8 + 7] = -0.0; buf[0][(size_t)2 * 16 + 8 + 7] = INFINITY; }
  if (mode == 1)  // all NaN in what scalar 0 reads
    for (int32_t s = 0; s < ni; s++) buf[0][(size_t)s * 16 + 8 + 7] = NAN;
  auto sc = heap<SpiceyMcScalar>((size_t)n_scalar);
  for (int32_t j = 0; j < n_scalar; j++) {
    switch (j % 5) {
      case 0: sc[j] = program({ins(SPICEY_MCOP_FIELD, 0, 1, 7)}); break;
      case 1: sc[j] = program({ins(SPICEY_MCOP_FIELD, 1, 0, 0), ins(SPICEY_MCOP_GUARD), ins(SPICEY_MCOP_FIELD, 1, 0, 7)}); break;
      case 2: sc[j] = program({ins(SPICEY_MCOP_FIELD, 2, 0, 15), ins(SPICEY_MCOP_FIELD, 2, 0, 0), ins(SPICEY_MCOP_DIV)}); break;
      case 3: sc[j] = program({ins(SPICEY_MCOP_FIELD, 0, 0, 0), ins(SPICEY_MCOP_FIELD, 0, 0, 1), ins(SPICEY_MCOP_FIELD, 0, 0, 2), ins(SPICEY_MCOP_FIELD, 0, 0, 3),
                               ins(SPICEY_MCOP_ADD), ins(SPICEY_MCOP_MUL), ins(SPICEY_MCOP_SUB), ins(SPICEY_MCOP_CONST, 0, 0, 0, 0.5), ins(SPICEY_MCOP_MUL)}); break;
      default: {
        std::vector<SpiceyMcIns> v{ins(SPICEY_MCOP_FIELD, 2, 0, 4)};
        while (v.size() + 2 <= SPICEY_MC_SCALAR_INS) { v.push_back(ins(SPICEY_MCOP_CONST, 0, 0, 0, 1.0)); v.push_back(ins(SPICEY_MCOP_ADD)); }
        sc[j] = program(v);  // the longest program
      }
    }
  }
  auto valid = heap<uint8_t>((size_t)ni);
  for (int32_t s = 0; s < ni; s++) valid[s] = mode == 2 ? (s == ni / 2) : (s % 7 != 3);
  int32_t n_valid = 0;
  for (int32_t s = 0; s < ni; s++) n_valid += valid[s] != 0;
  auto lo = heap<double>((size_t)n_scalar), hi = heap<double>((size_t)n_scalar);
  for (int32_t j = 0; j < n_scalar; j++) { lo[j] = -1.0; hi[j] = j % 2 ? INFINITY : 1.0; }
  const int32_t n_prob = 3;
  auto probs = heap<double>(n_prob);
  probs[0] = 0.0; probs[1] = 0.5; probs[2] = 1.0;
  const size_t row = SPICEY_TMC_STAT_HEAD + 2 * n_prob;
  auto x = heap<double>((size_t)ni * n_scalar), stat = heap<double>((size_t)n_scalar * row);
  auto sample = heap<int64_t>((size_t)ni * 2);
  char err[256];
  const int32_t rc = spicey_tmc_host_reduce(ni, rows, sc.get(), n_scalar, mode == 3 ? nullptr : valid.get(), lo.get(), mode == 3 ? nullptr : hi.get(), probs.get(), n_prob,
                                            x.get(), stat.get(), sample.get(), 1, -1, threads, err, 256);
  expect(rc == SPICEY_OK, "reduce accepted");
  if (rc != SPICEY_OK) { fprintf(stderr, "  %s\n", err); return; }
  if (mode == 3) n_valid = ni;
  for (int32_t j = 0; j < n_scalar; j++) {
    const double *r = stat.get() + (size_t)j * row;
    expect(r[0] == (double)n_valid && r[1] <= r[0] && r[2] <= r[0] && r[7] == 0.0, "counts of a stat row");
    if (r[1] > 0) {
      expect(r[8] <= r[10] && r[10] <= r[12] && r[8] <= r[9] && r[12] == r[13], "order statistics ascend");
      expect(r[5] >= 0 && r[5] < ni && r[6] >= 0 && r[6] < ni, "worst samples are sample indices");
      expect(x[(size_t)r[5] * n_scalar + j] == r[8] && x[(size_t)r[6] * n_scalar + j] == r[12], "the worst samples hold the extremes");
    } else expect(r[5] == -1.0 && r[6] == -1.0 && std::isnan(r[8]) && r[3] == 0.0 && !std::signbit(r[3]), "an all-NaN scalar");
  }
  if (mode == 1) expect(stat[1] == 0.0, "mode 1: scalar 0 has no number");
  for (int32_t s = 0; s < ni; s++) {
    const bool ok = mode == 3 || valid[s];
    expect(ok ? (sample[2 * s] >= 0 && sample[2 * s + 1] < n_scalar) : (sample[2 * s] == -1 && sample[2 * s + 1] == -1), "a sample's row");
  }
}

void refusals() {
  double rowbuf[16] = {0};
  const SpiceyMcRows rows[3] = {{rowbuf, 1, 8}, {nullptr, 0, 8}, {rowbuf, 1, SPICEY_POWER_ROW}};
  double x[1] = {-7.0}, stat[8] = {-7.0};
  int64_t sample[2] = {-99, -99};
  char err[256];
  const std::vector<std::vector<SpiceyMcIns>> bad = {
      {ins(SPICEY_MCOP_ADD)},                                                                      // underflow
      {ins(SPICEY_MCOP_FIELD, 0, 0, 0), ins(SPICEY_MCOP_FIELD, 0, 0, 0)},                          // depth 2 at the end
      {ins(SPICEY_MCOP_FIELD, 0, 0, 0), ins(SPICEY_MCOP_GUARD)},                                   // depth 0 at the end
      {ins(SPICEY_MCOP_CONST, 0, 0, 0, 1), ins(SPICEY_MCOP_CONST, 0, 0, 0, 1), ins(SPICEY_MCOP_CONST, 0, 0, 0, 1), ins(SPICEY_MCOP_CONST, 0, 0, 0, 1),
       ins(SPICEY_MCOP_CONST, 0, 0, 0, 1)},                                                        // overflow
      {ins(8)}, {ins(0)},                                                                          // unknown opcodes
      {ins(SPICEY_MCOP_FIELD, 1, 0, 0)},                                                           // empty pass
      {ins(SPICEY_MCOP_FIELD, 3, 0, 0)}, {ins(SPICEY_MCOP_FIELD, 0, 1, 0)}, {ins(SPICEY_MCOP_FIELD, 0, 0, 8)}, {ins(SPICEY_MCOP_FIELD, 2, 0, 16)},
      {ins(SPICEY_MCOP_CONST, 0, 0, 0, INFINITY)}, {ins(SPICEY_MCOP_CONST, 0, 0, 0, NAN)},
      {ins(SPICEY_MCOP_CONST, 0, 1, 0, 1.0)},                                                      // an unused word
  };
  for (const auto &v : bad) {
    const SpiceyMcScalar P = program(v);
    const int32_t rc = spicey_tmc_host_reduce(1, rows, &P, 1, nullptr, nullptr, nullptr, nullptr, 0, x, stat, sample, 1, -1, 0, err, 256);
    expect(rc == SPICEY_ERR_BAD_DESC && strncmp(err, "tran mc: ", 9) == 0 && x[0] == -7.0 && stat[0] == -7.0 && sample[0] == -99, "a bad program is refused and writes nothing");
  }
  SpiceyMcScalar P = program({ins(SPICEY_MCOP_FIELD, 0, 0, 0)});
  P.reserved = 1;
  expect(spicey_tmc_host_reduce(1, rows, &P, 1, nullptr, nullptr, nullptr, nullptr, 0, x, stat, sample, 1, -1, 0, err, 256) == SPICEY_ERR_BAD_DESC, "reserved");
  P.reserved = 0;
  P.n_ins = SPICEY_MC_SCALAR_INS + 1;
  expect(spicey_tmc_host_reduce(1, rows, &P, 1, nullptr, nullptr, nullptr, nullptr, 0, x, stat, sample, 1, -1, 0, err, 256) == SPICEY_ERR_BAD_DESC, "too long");
  P.n_ins = 1;
  expect(spicey_tmc_host_reduce(16385, rows, &P, 1, nullptr, nullptr, nullptr, nullptr, 0, x, stat, sample, 1, -1, 0, err, 256) == SPICEY_ERR_BAD_DESC, "n_inst > 16384");
  expect(spicey_tmc_host_reduce(1, rows, &P, 1, nullptr, nullptr, nullptr, nullptr, 0, x, stat, sample, 1, 8, 0, err, 256) == SPICEY_ERR_BAD_DESC, "small workspace");
  expect(spicey_tmc_host_reduce(1, rows, &P, 1, nullptr, nullptr, nullptr, nullptr, 0, x, stat, sample, 1, -1, 0, err, 256) == SPICEY_OK && x[0] == 0.0, "a good one");
}
}  // namespace

int main() {
  draw_case(1, 1, 0, 0, 0);
  draw_case(3, 2, 1, 1, 1);
  draw_case(65, 3, 2, 0, 10);
  for (int32_t ni : {1, 2, 63, 64, 65, 1000, 1024, 1025})
    for (int32_t ns : {1, 5})
      for (int32_t threads : {0, 64, 192, 1024})
        for (int mode : {0, 1, 2, 3}) reduce_case(ni, ns, threads, mode);
  reduce_case(16384, 2, 0, 0);
  reduce_case(8193, 2, 192, 0);
  refusals();
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("tran_mc_asan: ok\n");
  return 0;
}
