// Stand-alone program for the host sanitizers (`make asan`): the harness's draw, sort and reduction on buffers of exactly the
// stated sizes — the Philox known answers; draws at nE = 1 and 130 with tables of 2 and 1025 entries; the sort at n_pad = 1, 2,
// 64, 128 and 2048 with 64, 192 (no power of two) and 1024 threads against std::sort; reductions at n_inst = 1, 63, 65 and 1025
// (n_pad = 1, 64, 128, 2048) with invalid samples, a NaN and a mask — and every refusal of the two judges, after which the results
// must still hold their sentinel.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spicey_hip.h"

extern "C" void spicey_mc_host_philox(uint32_t *, uint32_t, uint32_t);
extern "C" int32_t spicey_mc_host_draw(int32_t, int32_t, int32_t, int32_t, const double *, const double *, const double *, const double *, const double *,
                                       const SpiceyAcMcReq *, double *, double *, double *, int32_t, int64_t, char *, int32_t);
extern "C" void spicey_mc_host_sort(uint64_t *, int32_t, int32_t);
extern "C" int32_t spicey_mc_host_reduce(int32_t, int64_t, const double *, int32_t, const uint8_t *, const double *, const double *, const int64_t *, int32_t,
                                         const SpiceyAcMcReq *, int64_t *, double *, int32_t, int64_t, int32_t, char *, int32_t);

namespace {
uint64_t g_state = 88172645463325252ull;
uint64_t rnd64() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return g_state;
}
double rnd() { return ((double)(rnd64() >> 11) + 0.5) / 4503599627370496.0 - 1.0; }  // in (-1, 1) without 0
std::vector<double> positive(size_t n, double scale) {
  std::vector<double> v(n);
  for (double &x : v) x = scale * (1.5 + rnd());
  return v;
}
const double SENTINEL = -7.25;
SpiceyAcMcReq request(int32_t out_p, int32_t out_n, int32_t log2K, int32_t keep, uint64_t seed) {
  SpiceyAcMcReq q{};
  q.struct_bytes = (int64_t)sizeof(q);
  q.out_p = out_p; q.out_n = out_n; q.log2K = log2K; q.keep_first = keep; q.seed = seed;
  return q;
}
}  // namespace

int main() {
  char err[200];
  // Philox4x32-10: the three known answers
  {
    const uint32_t in[3][6] = {{0, 0, 0, 0, 0, 0},
                               {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                               {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
    const uint32_t want[3][4] = {{0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
                                 {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
                                 {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
    for (int i = 0; i < 3; i++) {
      uint32_t c[4] = {in[i][0], in[i][1], in[i][2], in[i][3]};
      spicey_mc_host_philox(c, in[i][4], in[i][5]);
      if (memcmp(c, want[i], sizeof(c)) != 0) return 1;
    }
  }
  // the draw
  int draws = 0, refused = 0;
  const int shapes[2][3] = {{1, 0, 0}, {60, 40, 30}};
  for (const auto &sh : shapes)
    for (int32_t log2K : {0, 10}) {
      const int32_t ni = 5, nR = sh[0], nC = sh[1], nL = sh[2], nE = nR + nC + nL;
      const int64_t K = (int64_t)1 << log2K;
      const std::vector<double> R = positive((size_t)ni * nR, 1e3), Cv = positive((size_t)ni * nC, 1e-9), Lv = positive((size_t)ni * nL, 1e-3);
      std::vector<double> tol = positive((size_t)nE, 0.03), icdf((size_t)K + 1);
      tol[(size_t)nE / 2] = 0.0;
      for (int64_t j = 0; j <= K; j++) icdf[(size_t)j] = -1.0 + 2.0 * (double)j / (double)K;
      for (int keep = 0; keep < 2; keep++) {
        const SpiceyAcMcReq q = request(0, -1, log2K, keep, 0x123456789abcdef0ull);
        std::vector<double> oR((size_t)ni * nR, SENTINEL), oC((size_t)ni * nC, SENTINEL), oL((size_t)ni * nL, SENTINEL);
        if (spicey_mc_host_draw(ni, nR, nC, nL, nR ? R.data() : nullptr, nC ? Cv.data() : nullptr, nL ? Lv.data() : nullptr, tol.data(), icdf.data(), &q,
                                nR ? oR.data() : nullptr, nC ? oC.data() : nullptr, nL ? oL.data() : nullptr, 1, -1, err, 200) != SPICEY_OK) {
          fprintf(stderr, "%s\n", err);
          return 2;
        }
        draws++;
        for (size_t i = 0; i < oR.size(); i++) {
          const double r = 1.0 / oR[i];
          if (!(r > 0.9 * R[i] && r < 1.1 * R[i])) return 3;
          if (keep && i < (size_t)nR && oR[i] != 1.0 / R[i]) return 4;
        }
        for (size_t i = 0; i < oC.size(); i++)
          if (!(oC[i] > 0.9 * Cv[i] && oC[i] < 1.1 * Cv[i]) || (keep && i < (size_t)nC && oC[i] != Cv[i])) return 3;
        for (size_t i = 0; i < oL.size(); i++)
          if (!(oL[i] > 0.9 * Lv[i] && oL[i] < 1.1 * Lv[i]) || (keep && i < (size_t)nL && oL[i] != Lv[i])) return 3;
      }
      // the refusals: nothing is written
      auto refuse = [&](SpiceyAcMcReq q, const double *tl, const double *tab, int32_t n_inst, int32_t n_r, int32_t have_work, int64_t wb, const char *text) {
        std::vector<double> oR((size_t)ni * nR + 1, SENTINEL), oC((size_t)ni * nC + 1, SENTINEL), oL((size_t)ni * nL + 1, SENTINEL);
        err[0] = 0;
        const int32_t rc = spicey_mc_host_draw(n_inst, n_r, nC, nL, R.data(), Cv.data(), Lv.data(), tl, tab, &q, oR.data(), oC.data(), oL.data(), have_work, wb, err, 200);
        bool clean = rc == SPICEY_ERR_BAD_DESC && strstr(err, "mc") && strstr(err, text);
        for (double x : oR) clean = clean && x == SENTINEL;
        for (double x : oC) clean = clean && x == SENTINEL;
        for (double x : oL) clean = clean && x == SENTINEL;
        if (!clean) fprintf(stderr, "refusal '%s' went wrong: rc %d, text '%s'\n", text, rc, err);
        refused += clean;
      };
      const SpiceyAcMcReq ok = request(0, -1, log2K, 0, 7);
      SpiceyAcMcReq q;
      q = ok; q.struct_bytes = 8; refuse(q, tol.data(), icdf.data(), ni, nR, 1, -1, "struct_bytes");
      q = ok; q.reserved = 1; refuse(q, tol.data(), icdf.data(), ni, nR, 1, -1, "reserved");
      q = ok; q.log2K = 13; refuse(q, tol.data(), icdf.data(), ni, nR, 1, -1, "log2K");
      q = ok; q.log2K = -1; refuse(q, tol.data(), icdf.data(), ni, nR, 1, -1, "log2K");
      refuse(ok, tol.data(), icdf.data(), 0, nR, 1, -1, "bad counts");
      refuse(ok, tol.data(), icdf.data(), 16385, nR, 1, -1, "16384");
      refuse(ok, tol.data(), icdf.data(), ni, -1, 1, -1, "bad counts");
      refuse(ok, nullptr, icdf.data(), ni, nR, 1, -1, "null buffer");
      refuse(ok, tol.data(), nullptr, ni, nR, 1, -1, "null buffer");
      refuse(ok, tol.data(), icdf.data(), ni, nR, 0, -1, "null buffer");
      refuse(ok, tol.data(), icdf.data(), ni, nR, 1, 8, "workspace");
      std::vector<double> bad = tol;
      bad[(size_t)nE - 1] = -1e-3; refuse(ok, bad.data(), icdf.data(), ni, nR, 1, -1, "tolerance");
      bad[(size_t)nE - 1] = NAN; refuse(ok, bad.data(), icdf.data(), ni, nR, 1, -1, "tolerance");
      bad[(size_t)nE - 1] = INFINITY; refuse(ok, bad.data(), icdf.data(), ni, nR, 1, -1, "tolerance");
      bad[(size_t)nE - 1] = 1.0; refuse(ok, bad.data(), icdf.data(), ni, nR, 1, -1, ">= 1");
      std::vector<double> tab = icdf;
      tab[(size_t)K] = NAN; refuse(ok, tol.data(), tab.data(), ni, nR, 1, -1, "table");
      tab[(size_t)K] = INFINITY; refuse(ok, tol.data(), tab.data(), ni, nR, 1, -1, "table");
      tab[(size_t)K] = -2.0; refuse(ok, tol.data(), tab.data(), ni, nR, 1, -1, "table");
    }
  if (refused != 4 * 18) return 5;
  // the sort, against std::sort
  int sorts = 0;
  for (int32_t n_pad : {1, 2, 64, 128, 2048})
    for (int32_t threads : {64, 192, 1024}) {
      std::vector<uint64_t> x((size_t)n_pad);
      for (uint64_t &k : x) k = rnd64() >> (rnd64() & 31);
      if (n_pad > 2) { x[1] = x[0]; x[(size_t)n_pad - 1] = 0xffffffffffffffffull; x[2] = 0; }
      std::vector<uint64_t> want = x;
      std::sort(want.begin(), want.end());
      spicey_mc_host_sort(x.data(), n_pad, threads);
      if (x != want) return 6;
      sorts++;
    }
  // the reduction
  int reductions = 0, refused2 = 0;
  for (int32_t ni : {1, 63, 65, 1025}) {
    const int64_t nf = 5;
    const int32_t n_v = 3;
    std::vector<double> v((size_t)ni * nf * n_v * 2);
    for (double &x : v) x = 3.0 * rnd();
    std::vector<uint8_t> valid((size_t)ni, 1);
    if (ni > 2) { valid[1] = 0; valid[(size_t)ni - 1] = 0; v[(((size_t)2 * nf + 1) * n_v + 1) * 2] = NAN; }
    int32_t n_valid = 0;
    for (uint8_t b : valid) n_valid += b;
    const std::vector<double> lo((size_t)nf, 0.5), hi((size_t)nf, 20.0);
    const std::vector<int64_t> ranks = {0, n_valid - 1, n_valid / 2, n_valid / 2};
    const int32_t n_rank = (int32_t)ranks.size();
    std::vector<double> ref;
    for (int32_t threads : {0, 64, 192}) {
      const SpiceyAcMcReq q = request(1, 2, 0, 0, 0);
      std::vector<int64_t> sample((size_t)ni * 2, -99);
      std::vector<double> freq((size_t)nf * (4 + n_rank), SENTINEL);
      if (spicey_mc_host_reduce(ni, nf, v.data(), n_v, valid.data(), lo.data(), hi.data(), ranks.data(), n_rank, &q, sample.data(), freq.data(), 1, -1, threads, err,
                                200) != SPICEY_OK) {
        fprintf(stderr, "%s\n", err);
        return 7;
      }
      reductions++;
      for (int64_t x : sample) if (x == -99) return 8;
      for (double x : freq) if (x == SENTINEL) return 8;
      for (int32_t s = 0; s < ni; s++)
        if ((sample[2 * (size_t)s] == -1) != (valid[(size_t)s] == 0)) return 9;
      for (int64_t k = 0; k < nf; k++) {
        const double *row = &freq[(size_t)k * (4 + n_rank)];
        if (row[0] != (double)n_valid || !(row[4] <= row[6] || std::isnan(row[5])) || memcmp(&row[6], &row[7], 8) != 0) return 10;
      }
      // the result does not depend on the sorting workgroup's size
      if (ref.empty()) ref = freq;
      else if (memcmp(ref.data(), freq.data(), freq.size() * sizeof(double)) != 0) return 11;
    }
    auto refuse = [&](SpiceyAcMcReq q, int32_t n_inst, int32_t n_vv, const int64_t *rk, int32_t have_out, int64_t wb, const char *text) {
      std::vector<int64_t> sample((size_t)ni * 2, -99);
      std::vector<double> freq((size_t)nf * (4 + n_rank), SENTINEL);
      err[0] = 0;
      const int32_t rc = spicey_mc_host_reduce(n_inst, nf, v.data(), n_vv, valid.data(), lo.data(), hi.data(), rk, n_rank, &q, sample.data(), freq.data(), have_out, wb, 0,
                                               err, 200);
      bool clean = rc == SPICEY_ERR_BAD_DESC && strstr(err, "mc") && strstr(err, text);
      for (int64_t x : sample) clean = clean && x == -99;
      for (double x : freq) clean = clean && x == SENTINEL;
      if (!clean) fprintf(stderr, "refusal '%s' went wrong: rc %d, text '%s'\n", text, rc, err);
      refused2 += clean;
    };
    const SpiceyAcMcReq ok = request(0, -1, 0, 0, 0);
    SpiceyAcMcReq q;
    q = ok; q.out_p = n_v; refuse(q, ni, n_v, ranks.data(), 1, -1, "column out of range");
    q = ok; q.out_n = 0; refuse(q, ni, n_v, ranks.data(), 1, -1, "one node twice");
    q = ok; q.struct_bytes = 8; refuse(q, ni, n_v, ranks.data(), 1, -1, "struct_bytes");
    q = ok; q.reserved = -1; refuse(q, ni, n_v, ranks.data(), 1, -1, "reserved");
    refuse(ok, 0, n_v, ranks.data(), 1, -1, "bad counts");
    refuse(ok, ni, 0, ranks.data(), 1, -1, "bad counts");
    refuse(ok, ni, n_v, nullptr, 1, -1, "null buffer");
    refuse(ok, ni, n_v, ranks.data(), 0, -1, "null buffer");
    refuse(ok, ni, n_v, ranks.data(), 1, 8, "workspace");
    std::vector<int64_t> bad = ranks;
    bad[3] = n_valid; refuse(ok, ni, n_v, bad.data(), 1, -1, "rank");
    bad[3] = -1; refuse(ok, ni, n_v, bad.data(), 1, -1, "rank");
  }
  if (refused2 != 4 * 11) return 12;
  printf("mc_asan ok: 3 known answers, %d draws, %d sorts, %d reductions, %d refusals\n", draws, sorts, reductions, refused + refused2);
  return 0;
}
