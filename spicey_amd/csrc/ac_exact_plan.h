// ac_exact_plan.h — host side of the reference-order AC engine (spicey_ac_create with SpiceyOptions.interpreter = 3,
// ac_exact_exec.h): the stamp list of every entry of the complex A | b and the element terminals, packed into one blob.
// No HIP header: the CPU test harness builds the very lists the product uploads.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/spicey_hip.h"
#include "exact_plan.h"  // (SpiceyExactTerm)
#include "launch_plan.h"

// Device-side constant data of an exact AC handle (built below; the kernel takes it by pointer).
struct SpiceyAcExactProg {
  int32_t n, nN, nR, nC, nL, nV, nOut, nCur;
  int32_t nEnt;                            // stamped entries of A | b
  int32_t ld, nq, qR, qC, qL, qV, qOne;    // SpiceyAcExactWs (launch_plan.h)
  int64_t oA, ox, oq, of, operm, oact, ws_cx;
  // entry e sits at A[ent_pos[e]] (row * ld + column, column n = b) and is the complex sum over
  // ent_src[ent_ptr[e] .. ent_ptr[e + 1]) of +-q[word & 0x7fffffff] (bit 31: subtract), in that order, from (+0, +0)
  const uint32_t *ent_pos, *ent_ptr, *ent_src;
  const int32_t *R_nd, *C_nd, *L_nd;  // [2 count] node ids (0 = ground) of every element (the currents)
  const int32_t *out_nodes;           // [nOut] recorded node ids
};

#define SPICEY_AC_EXACT_SUB 0x80000000u

struct HostAcExactProg {
  SpiceyAcExactProg hdr{};  // counts and offsets; pointers filled by bind()
  std::vector<uint32_t> ent_pos, ent_ptr, ent_src;
  std::vector<int32_t> R_nd, C_nd, L_nd, out_nodes;
  std::vector<uint32_t> blob;  // every array above, 16-byte aligned sections
  std::vector<size_t> offsets;
  SpiceyAcExactProg bind(const void *base) const;
  // one contribution, decoded (tests): kind 0..3 = R, C, L, V; elem = element index within its kind (-1 for the voltage
  // sources' constant +-1); which = 0: the admittance or the source phasor, 2: the constant (1, 0); sub = subtracted
  SpiceyExactTerm decode(uint32_t word) const;
};

// Replays buildLinearSystemForAC (simulateAC.ts:25-62, the checker spicey_ref_ac.c) symbolically: every stamp appends its
// quantity slot, with its sign, to the list of the entry it touches — R, C, L (stampAdmittanceComplex), then V
// (stampVoltageSourceComplex), each by element index.  Entries in row-major order.  `d` was validated.
void spicey_build_ac_exact(const SpiceyDesc &d, const SpiceyAcExactWs &ws, HostAcExactProg &xp);
