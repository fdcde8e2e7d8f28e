// The beamforming kernel of the beam mode (beam.hip; include/mimo_engine.h mimo_engine_beam_points).
#pragma once
#include <hip/hip_runtime.h>

namespace mimo {

constexpr int kBeamFixed = 5;  // MIMO_BEAM_FIXED

// Per trial t < n_trials and probe q < n_probes the five sums of mimo_engine_beam_points into
// rows[t][q][0 .. 4], from the beam instances' cells of one launch (trial_kernel.h BEAM):
//   cells   [2][n_trials][n_ant][n_fft] complex128: the chain outputs Y sqrt(F), then the precoder
//           inputs X / sqrt(F)
//   dist    [n_probes][n_ant] probe-antenna distances d_qa [m];  inv_dist their reciprocals
//   f_over_c [n_fft] f_k / c of every FFT bin
// Every row cell is written once, by plain stores, in an order that depends on the sizes alone.
hipError_t launch_beam(hipStream_t st, const double* cells, const double* dist, const double* inv_dist,
                       const double* f_over_c, int n_trials, int n_ant, int n_fft, int n_sub_carr, int n_probes,
                       double* rows);

}  // namespace mimo
