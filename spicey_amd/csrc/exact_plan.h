// exact_plan.h — host side of the reference-order engine (SpiceyOptions.interpreter = 3, exact_exec.h): the stamp list of
// every entry of A | b and the element terminals, packed into one blob.  No HIP header: the CPU test harness builds the
// very lists the product uploads.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/spicey_hip.h"
#include "launch_plan.h"

// Device-side constant data of an exact handle (built below; the kernel takes it by pointer).
struct SpiceyExactProg {
  int32_t n, nN, nR, nC, nL, nV, nS, nD, nOut, nCur;
  int32_t nEnt;  // stamped entries of A | b
  int32_t ld, mw, nq, qR, qGc, qIc, qGl, qIl, qS, qV, qGd, qIeq, qOne;  // SpiceyExactWs (launch_plan.h)
  int32_t pad_;
  int64_t oA, ox, oq, ovdlin, oact_f, operm, oact_r, omask, ws_doubles;
  // entry e sits at A[ent_pos[e]] (row * ld + column, column n = b) and is the sum over ent_src[ent_ptr[e] .. ent_ptr[e + 1])
  // of +-q[word & 0x7fffffff] (bit 31: subtract), in that order
  const uint32_t *ent_pos, *ent_ptr, *ent_src;
  const int32_t *R_nd, *C_nd, *L_nd, *V_nd, *S_nd, *S_ctl, *D_nd;  // [2 count] node ids (0 = ground) of every element
  const int32_t *out_nodes;                                          // [nOut] recorded node ids
};

#define SPICEY_EXACT_SUB 0x80000000u

// One contribution of a stamp list, decoded (tests, diagnostics): kind 0..5 = R, C, L, S, V, D; elem = element index within
// its kind (-1 for the voltage sources' constant +-1); which = 0: the admittance / conductance (1/R, Gc, Gl, 1/R_switch, gd)
// or the source value, 1: the current (C Ieq, L iPrev, D ieq), 2: the constant 1.0; sub = subtracted.
struct SpiceyExactTerm {
  int32_t kind, elem, which, sub;
};

struct HostExactProg {
  SpiceyExactProg hdr{};  // counts and offsets; pointers filled by bind()
  std::vector<uint32_t> ent_pos, ent_ptr, ent_src;
  std::vector<int32_t> R_nd, C_nd, L_nd, V_nd, S_nd, S_ctl, D_nd, out_nodes;
  std::vector<uint32_t> blob;  // every array above, 16-byte aligned sections
  std::vector<size_t> offsets;
  SpiceyExactProg bind(const void *base) const;
  SpiceyExactTerm decode(uint32_t word) const;
};

// Replays stampAllElementsAtTime (simulateTRAN.ts:25-102, the checker spicey_ref.c) symbolically: every stamp appends its
// quantity slot, with its sign, to the list of the entry it touches.  Entries in row-major order.  `d` was validated.
void spicey_build_exact(const SpiceyDesc &d, const SpiceyExactWs &ws, HostExactProg &xp);
