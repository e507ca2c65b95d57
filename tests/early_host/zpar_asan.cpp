// tests/early_host/zpar_asan.cpp — a stand-alone program (TEST INFRASTRUCTURE ONLY) for the address and undefined-behaviour
// sanitizers: the host code that decides on and sizes Z's parameter record (launch_plan.cpp: spicey_plan, spicey_zpar_doubles)
// and the device code that fills and reads it (tran_exec.h, on the emulator's sequential executor), run over a heap buffer
// of exactly the planned size.  An access outside the record, or a size that overflows, ends the program with the
// sanitizer's report.  Built and run by `make asan`; no GPU and no python involved.
#include "../emul/emul.cpp"

#include <cstdio>
#include <memory>

namespace {

struct Chain {  // V1 n1 0, then per stage k: R n_k n_k+1, C n_k+1 0, D n_k+1 0 — every instance its own values
  int n, ni;
  std::vector<int32_t> Rn1, Rn2, Cn1, Cn2, Vn1, Vn2, Dp, Dm;
  std::vector<double> Rv, Cv, Cvp, Dis, Dn, Dvd;
  SpiceyDesc d{};
  Chain(int n_, int ni_) : n(n_), ni(ni_) {
    const int m = n - 1;
    for (int k = 1; k <= m; k++) {
      Rn1.push_back(k); Rn2.push_back(k + 1);
      Cn1.push_back(k + 1); Cn2.push_back(0);
      Dp.push_back(k + 1); Dm.push_back(0);
    }
    Vn1 = {1}; Vn2 = {0};
    for (int g = 0; g < ni; g++)
      for (int k = 0; k < m; k++) {
        Rv.push_back(100.0 * (1.0 + 0.01 * g + 0.001 * (k % 7)));
        Cv.push_back(1e-9 * (1.0 + 0.02 * g));
        Cvp.push_back(0.0);
        Dis.push_back(1e-14 * (1.0 + 0.1 * g));
        Dn.push_back(1.0 + 0.05 * (k % 3));
        Dvd.push_back(0.0);
      }
    d.abi_version = SPICEY_ABI_VERSION; d.n_nodes = n; d.n_inst = ni;
    d.nR = m; d.nC = m; d.nL = 0; d.nV = 1; d.nS = 0; d.nD = m;
    d.R_n1 = Rn1.data(); d.R_n2 = Rn2.data(); d.R_val = Rv.data();
    d.C_n1 = Cn1.data(); d.C_n2 = Cn2.data(); d.C_val = Cv.data(); d.C_vprev = Cvp.data();
    d.V_n1 = Vn1.data(); d.V_n2 = Vn2.data();
    d.D_np = Dp.data(); d.D_nm = Dm.data(); d.D_is = Dis.data(); d.D_n = Dn.data(); d.D_vdprev = Dvd.data();
    d.n_out = 0; d.out_nodes = nullptr;
  }
};

struct SeqExecIdle : SeqExec {
  static constexpr bool idle_waves = true;
  template <class F, class G>
  void wave_lockstep_keep_then(int nlanes, int nsteps, F f, G g) {
    for (int t = 64; t < T; t++) g(t);
    wave_lockstep_keep(nlanes, nsteps, f);
    for (int t = 0; t < (T < 64 ? T : 64); t++) g(t);
  }
};

int fail(const char *what) { fprintf(stderr, "zpar_asan: %s\n", what); return 1; }

// plan the handle as spicey_create does, own a record of the planned size, run `steps` steps over it on both placements
int one(int n, int ni, bool knob_off, int64_t steps) {
  if (knob_off) setenv("SPICEY_NO_EARLY_PREFETCH", "1", 1);
  else unsetenv("SPICEY_NO_EARLY_PREFETCH");
  Chain ch(n, ni);
  SpiceyOptions opt{};
  opt.geometry = 2; opt.want_currents = 1;
  const PlanDevice dev{[](int, int *ncu, std::string &) { *ncu = 256; return (int32_t)SPICEY_OK; }, [](const SpiceyProg &, int, int) { return 1; }};
  HostProgram hp;
  HostResident hres;
  LaunchPlan plan;
  std::string msg;
  if (spicey_plan(&ch.d, opt, spicey_read_knobs(), dev, hp, hres, plan, msg) != SPICEY_OK) return fail(msg.c_str());
  const size_t nz = spicey_zpar_doubles(plan, hp);
  printf("chain(%d) x %d: packed %d fresh %d early %d threads %d, record %zu doubles\n", n, ni, (int)plan.packed, (int)plan.fresh, (int)plan.early, plan.T, nz);
  if (!plan.packed || !plan.fresh) return fail("the plan did not take the packed fresh build");
  if (knob_off) return (plan.early || nz != 0) ? fail("SPICEY_NO_EARLY_PREFETCH left a record") : 0;
  if (!plan.early || nz != (size_t)ni * 2 * (size_t)plan.T * 5) return fail("record size");
  const int T = plan.T;
  SpiceyProg P = hp.bind(hp.blob.data());
  SpiceyResident Q = hres.bind(hres.blob.data());
  for (int idle = 0; idle < 2; idle++) {
    std::unique_ptr<double[]> zpar(new double[nz]);  // exactly the planned size: the sanitizer guards both ends
    std::vector<double> src((size_t)(steps + 1), 1.0), out_v((size_t)ni * (steps + 1) * ch.d.n_nodes), out_i((size_t)ni * (steps + 1) * (ch.d.nR + ch.d.nC + ch.d.nV + ch.d.nD));
    std::vector<double> Cvp(ch.Cvp), Dvd(ch.Dvd);
    std::vector<double> gstat((size_t)ni * P.nGstat), statv((size_t)ni * P.nLU), rcoef((size_t)ni * (P.nRhsIdx + 1)), dpar((size_t)ni * (P.nD + 1) * 2);
    std::vector<int32_t> status((size_t)ni * 4);
    std::vector<unsigned long long> solves(ni);
    SpiceyRun R{};
    R.n_inst = ni; R.want_currents = 1; R.steps = steps; R.dt = 1e-6;
    R.R_val = ch.d.R_val; R.C_val = ch.d.C_val; R.D_is = ch.d.D_is; R.D_n = ch.d.D_n;
    R.C_vprev = Cvp.data(); R.D_vdprev = Dvd.data();
    R.gstat = gstat.data(); R.statv = statv.data(); R.rcoef = rcoef.data(); R.dpar = dpar.data();
    R.src = src.data(); R.out_v = out_v.data(); R.out_i = out_i.data();
    R.status = status.data(); R.solves = solves.data();
    R.zpar = zpar.get();
    for (int g = 0; g < ni; g++) {
      std::vector<double> W((size_t)P.nW), u((size_t)P.nU + 1), gd((size_t)P.nGdyn + 1);
      std::vector<int32_t> ison((size_t)P.nS + 1), fl(4);
      std::vector<uint32_t> tail((size_t)(hres.tail_n + 6) * 64 * 4);
      std::vector<ResRegs<1, 4, 2, 2>> regs(T);
      WgCtx<1> c;
      c.W = W.data(); c.u = u.data(); c.gd = gd.data(); c.ison = ison.data(); c.flags = fl.data(); c.tail = tail.data(); c.G = nullptr;
      c.valid[0] = true; c.inst[0] = g;
      if (idle) {
        SeqExecIdle ex;
        ex.T = T; ex.reverse = false; ex.rr = &regs;
        spicey_tran_run_v2<1, 4, 2, 2, false, -1, true>(ex, P, Q, R, c, g);
      } else {
        SeqExec ex{T, false};
        ex.rr = &regs;
        spicey_tran_run_v2<1, 4, 2, 2, false, -1, true>(ex, P, Q, R, c, g);
      }
      if (status[(size_t)g * 4]) return fail("singular");
    }
    double sum = 0.0;
    for (double v : out_v) sum += v;
    if (!(sum == sum)) return fail("NaN in the result");
    printf("  %s placement: %lld steps, checksum %.17g\n", idle ? "idle-wave" : "last-factor-phase", (long long)steps, sum);
  }
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad |= one(100, 3, false, 4);   // items without a record entry: zero-filled slots
  bad |= one(1000, 2, false, 3);  // the bench circuit's shape
  bad |= one(1023, 1, false, 2);  // every resident item exists
  bad |= one(1000, 2, true, 0);   // the knob: no record
  printf(bad ? "zpar_asan: FAILED\n" : "zpar_asan: ok\n");
  return bad;
}
