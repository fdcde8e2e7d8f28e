// The step kernel of the turbo mode (turbo.hip; include/mimo_engine.h mimo_engine_turbo_points,
// mimo_engine_cnc_step): one pass of the decoder-aided CNC receiver on the received vectors the turbo
// instances left (trial_params.h MIMO_MODE_TURBO).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "trial_launch.h"

namespace mimo {

// What a step reads and writes besides the launch's parameter table.  stream = S log2 M; position
// p = j S + k of block b (bit j of sub-carrier k, the I axis MSB first, then Q) is at b stream + p in
// hard, chan_in and chan_out.
struct StepArgs {
  const double2* z;       // [blocks][S]: the turbo instances' received vectors, sub-carrier order
  // The decisions of the pass before (not read by the first pass), one of:
  //  labels != null: the decided labels themselves, [blocks][S] (the seam);
  //  else the transmitted label XOR the error bits: hard[p] != 0 for p < n_dec (the decoder's decision,
  //  ldpc.h launch_ldpc), chan_in[p] < 0 for the undecoded tail (the demapper's decision).
  const int32_t* labels;
  const int8_t* hard;
  const int8_t* chan_in;
  int n_dec;              // n_cw N: the decoded positions of a stream
  // Outputs, each optional: the channel values of v (softbits.h coded_value at `scale`, signed by
  // the transmitted bits, as the coded instances write them) and v itself, [blocks][S].
  // chan_out may be chan_in: a thread reads the positions of its own sub-carriers before it writes them.
  int8_t* chan_out;
  double scale;           // 32 / rho_max
  double2* v_out;
};

// One step over `blocks` trials, one workgroup per trial, on the instance's FFT and slot map
// (key: engine.hip select_instance; float64 only).  p: the parameters of the trial launch the
// vectors came from -- its point table, twiddle tables and sizes.  first: the pass-0 step, v = z (no
// CNC part).  *found = the key names a built instance.
hipError_t launch_turbo_step(const InstanceKey& key, bool first, unsigned blocks, hipStream_t st,
                             const TrialParams<double>& p, const StepArgs& a, bool* found);

}  // namespace mimo
