// ac_sweep.h — what a sweep of either AC engine (ac_abi.cpp) hands to the entry points that follow it: the results still
// on the device, the status word of every (instance, frequency) slot, and the per-instance summary of
// spicey_ac_last_inst_status.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/spicey_hip.h"
#include "devbuf.h"

// One finished sweep: d_ov [n_inst][n_freq][n_out][2], d_oi [n_inst][n_freq][n_cur][2] (only when currents were wanted),
// status [n_inst][n_freq] (0, 1 = singular, anything else = complex divide by ~0) already on the host.
struct SpiceyAcSweep {
  DevBuf<double> d_ov, d_oi;
  std::vector<int32_t> status;
};

// Per instance: the code of its lowest failing frequency index and that index (-1: fine).
struct SpiceyAcInstStatus {
  std::vector<int32_t> code;
  std::vector<int64_t> first;
  bool valid = false;

  void forget() { valid = false; }
  void fill(int32_t n_inst, int32_t c, int64_t f) {
    code.assign((size_t)n_inst, c);
    first.assign((size_t)n_inst, f);
    valid = true;
  }
  // From the slots of a sweep.  Returns what the sweep's entry point returns — the reference stops at the first frequency
  // that throws (simulateAC.ts:80-83), so the first failing slot decides — with its text in `err`.
  int32_t from_slots(const std::vector<int32_t> &status, int32_t n_inst, int64_t n_freq, std::string &err) {
    fill(n_inst, 0, -1);
    int32_t rc = SPICEY_OK;
    for (size_t s = 0; s < status.size(); s++) {
      if (status[s] == 0) continue;
      const size_t inst = s / (size_t)n_freq;
      if (code[inst] != 0) continue;
      const bool sing = status[s] == 1;
      code[inst] = sing ? SPICEY_ERR_SINGULAR : SPICEY_ERR_COMPLEX_DIV;
      first[inst] = (int64_t)(s % (size_t)n_freq);
      if (rc == SPICEY_OK) {
        rc = code[inst];
        err = std::string(sing ? "Singular matrix (complex)" : "Complex divide by ~0") + " at inst " + std::to_string(inst) + " frequency index " +
              std::to_string(s % (size_t)n_freq);
      }
    }
    return rc;
  }
};
