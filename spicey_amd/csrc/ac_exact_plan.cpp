// ac_exact_plan.cpp — see ac_exact_plan.h.
#include "ac_exact_plan.h"

#include <map>
#include <utility>

void spicey_build_ac_exact(const SpiceyDesc &d, const SpiceyAcExactWs &ws, HostAcExactProg &xp) {
  xp = HostAcExactProg();
  SpiceyAcExactProg &H = xp.hdr;
  const int nN = d.n_nodes, n = d.n_nodes + d.nV;
  H.n = n; H.nN = nN;
  H.nR = d.nR; H.nC = d.nC; H.nL = d.nL; H.nV = d.nV;
  H.nOut = (d.n_out > 0 && d.out_nodes) ? d.n_out : nN;
  H.nCur = d.nR + d.nC + d.nL + d.nV;
  H.ld = ws.ld; H.nq = ws.nq; H.qR = ws.qR; H.qC = ws.qC; H.qL = ws.qL; H.qV = ws.qV; H.qOne = ws.qOne;
  H.oA = ws.A; H.ox = ws.x; H.oq = ws.q; H.of = ws.f; H.operm = ws.perm; H.oact = ws.act; H.ws_cx = ws.cx;

  // (row, column) -> contributions in stamping order; column n = the right-hand side
  std::map<std::pair<int, int>, std::vector<uint32_t>> lists;
  auto put = [&](int r, int c, uint32_t slot, bool sub) { lists[{r, c}].push_back(slot | (sub ? SPICEY_AC_EXACT_SUB : 0u)); };
  auto adm = [&](int n1, int n2, uint32_t slot) {  // stampAdmittanceComplex.ts:4-30
    const int i1 = n1 - 1, i2 = n2 - 1;
    if (i1 >= 0) put(i1, i1, slot, false);
    if (i2 >= 0) put(i2, i2, slot, false);
    if (i1 >= 0 && i2 >= 0) {
      put(i1, i2, slot, true);
      put(i2, i1, slot, true);
    }
  };
  for (int i = 0; i < d.nR; i++) adm(d.R_n1[i], d.R_n2[i], ws.qR + i);
  for (int i = 0; i < d.nC; i++) adm(d.C_n1[i], d.C_n2[i], ws.qC + i);
  for (int i = 0; i < d.nL; i++) adm(d.L_n1[i], d.L_n2[i], ws.qL + i);
  for (int k = 0; k < d.nV; k++) {  // stampVoltageSourceComplex.ts:5-35
    const int i1 = d.V_n1[k] - 1, i2 = d.V_n2[k] - 1, j = nN + k;
    if (i1 >= 0) put(i1, j, ws.qOne, false);
    if (i2 >= 0) put(i2, j, ws.qOne, true);
    if (i1 >= 0) put(j, i1, ws.qOne, false);
    if (i2 >= 0) put(j, i2, ws.qOne, true);
    put(j, n, ws.qV + k, false);
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
  for (const std::vector<int32_t> *v : {&xp.R_nd, &xp.C_nd, &xp.L_nd, &xp.out_nodes}) add(v->data(), v->size());
  while (xp.blob.size() % 4) xp.blob.push_back(0);
}

SpiceyAcExactProg HostAcExactProg::bind(const void *base) const {
  SpiceyAcExactProg P = hdr;
  const uint32_t *b = static_cast<const uint32_t *>(base);
  P.ent_pos = b + offsets[0];
  P.ent_ptr = b + offsets[1];
  P.ent_src = b + offsets[2];
  const int32_t **nd[] = {&P.R_nd, &P.C_nd, &P.L_nd, &P.out_nodes};
  for (int i = 0; i < 4; i++) *nd[i] = reinterpret_cast<const int32_t *>(b + offsets[3 + i]);
  return P;
}

SpiceyExactTerm HostAcExactProg::decode(uint32_t word) const {
  const SpiceyAcExactProg &H = hdr;
  const int s = (int)(word & ~SPICEY_AC_EXACT_SUB), sub = (word & SPICEY_AC_EXACT_SUB) ? 1 : 0;
  const struct { int at, cnt, kind, which; } kinds[] = {{H.qR, H.nR, 0, 0}, {H.qC, H.nC, 1, 0}, {H.qL, H.nL, 2, 0}, {H.qV, H.nV, 3, 0}, {H.qOne, 1, 3, 2}};
  for (const auto &k : kinds)
    if (s >= k.at && s < k.at + k.cnt) return {k.kind, k.which == 2 ? -1 : s - k.at, k.which, sub};
  return {-1, -1, -1, sub};
}
