// exact_plan.cpp — see exact_plan.h.
#include "exact_plan.h"

#include <map>
#include <utility>

void spicey_build_exact(const SpiceyDesc &d, const SpiceyExactWs &ws, HostExactProg &xp) {
  xp = HostExactProg();
  SpiceyExactProg &H = xp.hdr;
  const int nN = d.n_nodes, n = d.n_nodes + d.nV;
  H.n = n; H.nN = nN;
  H.nR = d.nR; H.nC = d.nC; H.nL = d.nL; H.nV = d.nV; H.nS = d.nS; H.nD = d.nD;
  H.nOut = (d.n_out > 0 && d.out_nodes) ? d.n_out : nN;
  H.nCur = d.nR + d.nC + d.nL + d.nV + d.nS + d.nD;
  H.ld = ws.ld; H.mw = ws.mw; H.nq = ws.nq;
  H.qR = ws.qR; H.qGc = ws.qGc; H.qIc = ws.qIc; H.qGl = ws.qGl; H.qIl = ws.qIl; H.qS = ws.qS; H.qV = ws.qV; H.qGd = ws.qGd;
  H.qIeq = ws.qIeq; H.qOne = ws.qOne;
  H.oA = ws.A; H.ox = ws.x; H.oq = ws.q; H.ovdlin = ws.vdlin; H.oact_f = ws.act_f; H.operm = ws.perm; H.oact_r = ws.act_r;
  H.omask = ws.mask; H.ws_doubles = ws.doubles;

  // (row, column) -> contributions in stamping order; column n = the right-hand side
  std::map<std::pair<int, int>, std::vector<uint32_t>> lists;
  auto put = [&](int r, int c, uint32_t slot, bool sub) { lists[{r, c}].push_back(slot | (sub ? SPICEY_EXACT_SUB : 0u)); };
  auto adm = [&](int n1, int n2, uint32_t slot) {  // stampAdmittanceReal.ts:3-29
    const int i1 = n1 - 1, i2 = n2 - 1;
    if (i1 >= 0) put(i1, i1, slot, false);
    if (i2 >= 0) put(i2, i2, slot, false);
    if (i1 >= 0 && i2 >= 0) {
      put(i1, i2, slot, true);
      put(i2, i1, slot, true);
    }
  };
  auto cur = [&](int np, int nm, uint32_t slot) {  // stampCurrentReal.ts:3-14
    if (np - 1 >= 0) put(np - 1, n, slot, true);
    if (nm - 1 >= 0) put(nm - 1, n, slot, false);
  };
  for (int i = 0; i < d.nR; i++) adm(d.R_n1[i], d.R_n2[i], ws.qR + i);
  for (int i = 0; i < d.nC; i++) {
    adm(d.C_n1[i], d.C_n2[i], ws.qGc + i);
    cur(d.C_n1[i], d.C_n2[i], ws.qIc + i);
  }
  for (int i = 0; i < d.nL; i++) {
    adm(d.L_n1[i], d.L_n2[i], ws.qGl + i);
    cur(d.L_n1[i], d.L_n2[i], ws.qIl + i);
  }
  for (int i = 0; i < d.nS; i++) adm(d.S_n1[i], d.S_n2[i], ws.qS + i);
  for (int k = 0; k < d.nV; k++) {  // stampVoltageSourceReal.ts:4-32
    const int i1 = d.V_n1[k] - 1, i2 = d.V_n2[k] - 1, j = nN + k;
    if (i1 >= 0) put(i1, j, ws.qOne, false);
    if (i2 >= 0) put(i2, j, ws.qOne, true);
    if (i1 >= 0) put(j, i1, ws.qOne, false);
    if (i2 >= 0) put(j, i2, ws.qOne, true);
    put(j, n, ws.qV + k, false);
  }
  for (int i = 0; i < d.nD; i++) {
    adm(d.D_np[i], d.D_nm[i], ws.qGd + i);
    cur(d.D_np[i], d.D_nm[i], ws.qIeq + i);
  }
  xp.ent_ptr.push_back(0);
  for (const auto &kv : lists) {
    xp.ent_pos.push_back((uint32_t)((int64_t)kv.first.first * ws.ld + kv.first.second));
    xp.ent_src.insert(xp.ent_src.end(), kv.second.begin(), kv.second.end());
    xp.ent_ptr.push_back((uint32_t)xp.ent_src.size());
  }
  H.nEnt = (int32_t)xp.ent_pos.size();

  auto pairs = [](std::vector<int32_t> &out, const int32_t *a, const int32_t *b, int cnt) {
    for (int i = 0; i < cnt; i++) { out.push_back(a[i]); out.push_back(b[i]); }
  };
  pairs(xp.R_nd, d.R_n1, d.R_n2, d.nR);
  pairs(xp.C_nd, d.C_n1, d.C_n2, d.nC);
  pairs(xp.L_nd, d.L_n1, d.L_n2, d.nL);
  pairs(xp.V_nd, d.V_n1, d.V_n2, d.nV);
  pairs(xp.S_nd, d.S_n1, d.S_n2, d.nS);
  pairs(xp.S_ctl, d.S_cp, d.S_cn, d.nS);
  pairs(xp.D_nd, d.D_np, d.D_nm, d.nD);
  for (int i = 0; i < H.nOut; i++) xp.out_nodes.push_back((d.n_out > 0 && d.out_nodes) ? d.out_nodes[i] : i + 1);

  // one blob of 32-bit words, sections on 16-byte boundaries
  auto add = [&](const void *p, size_t words) {
    while (xp.blob.size() % 4) xp.blob.push_back(0);
    xp.offsets.push_back(xp.blob.size());
    const uint32_t *w = static_cast<const uint32_t *>(p);
    xp.blob.insert(xp.blob.end(), w, w + words);
  };
  add(xp.ent_pos.data(), xp.ent_pos.size());
  add(xp.ent_ptr.data(), xp.ent_ptr.size());
  add(xp.ent_src.data(), xp.ent_src.size());
  for (const std::vector<int32_t> *v : {&xp.R_nd, &xp.C_nd, &xp.L_nd, &xp.V_nd, &xp.S_nd, &xp.S_ctl, &xp.D_nd, &xp.out_nodes}) add(v->data(), v->size());
  while (xp.blob.size() % 4) xp.blob.push_back(0);
}

SpiceyExactProg HostExactProg::bind(const void *base) const {
  SpiceyExactProg P = hdr;
  const uint32_t *b = static_cast<const uint32_t *>(base);
  P.ent_pos = b + offsets[0];
  P.ent_ptr = b + offsets[1];
  P.ent_src = b + offsets[2];
  const int32_t **nd[] = {&P.R_nd, &P.C_nd, &P.L_nd, &P.V_nd, &P.S_nd, &P.S_ctl, &P.D_nd, &P.out_nodes};
  for (int i = 0; i < 8; i++) *nd[i] = reinterpret_cast<const int32_t *>(b + offsets[3 + i]);
  return P;
}

SpiceyExactTerm HostExactProg::decode(uint32_t word) const {
  const SpiceyExactProg &H = hdr;
  const int s = (int)(word & ~SPICEY_EXACT_SUB), sub = (word & SPICEY_EXACT_SUB) ? 1 : 0;
  const struct { int at, cnt, kind, which; } kinds[] = {{H.qR, H.nR, 0, 0},   {H.qGc, H.nC, 1, 0}, {H.qIc, H.nC, 1, 1}, {H.qGl, H.nL, 2, 0},
                                                      {H.qIl, H.nL, 2, 1},  {H.qS, H.nS, 3, 0},  {H.qV, H.nV, 4, 0},  {H.qGd, H.nD, 5, 0},
                                                      {H.qIeq, H.nD, 5, 1}, {H.qOne, 1, 4, 2}};
  for (const auto &k : kinds)
    if (s >= k.at && s < k.at + k.cnt) return {k.kind, k.which == 2 ? -1 : s - k.at, k.which, sub};
  return {-1, -1, -1, sub};
}
