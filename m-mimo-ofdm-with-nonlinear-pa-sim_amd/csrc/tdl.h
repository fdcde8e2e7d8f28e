// The generator kernel of the tapped-delay-line channel (tdl.hip; include/mimo_engine.h
// mimo_engine_set_tdl, mimo_tdl_channels): per trial and antenna the taps of a power-delay profile
// and their frequency response, written into the channel bank the table instances read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mimo_engine.h"

namespace mimo {

constexpr int kTdlMaxTaps = 64;  // MIMO_TDL_MAX_TAPS

// A checked profile and its host tables.
struct TdlHost {
  int n_taps = 0, n_ant = 0, n_fft = 0;
  std::vector<int32_t> delays;   // [L]
  std::vector<double> sqrt_pow;  // [L] sqrt(powers[l]), rounded once on the host
  std::vector<double> ant_amp;   // [A]
  // the device blob: W [n_fft] double2 | sqrt_pow [L] | ant_amp [A] | delays [L] int32 (in doubles' space)
  std::vector<double> blob() const;
};

// Checks every rule of include/mimo_engine.h's mimo_tdl for n_ant antennas and n_fft bins (host
// only) and copies the profile.  -> true, or false with the message that names the field.
bool tdl_prepare(const mimo_tdl* prof, int n_ant, int n_fft, TdlHost* out, std::string* err);

// One contiguous block range of a launch: its blocks run trials first_trial, first_trial + 1, ...
// under the key seed.
struct TdlSeg {
  uint64_t seed, first_trial;
};

// Fills out[b][a][c] for blocks b < n_blocks, antennas a < n_ant and columns c < n_cols with the
// response of block b's (seed, trial): block b belongs to segment i with seg_start[i] <= b <
// seg_start[i + 1] and runs trial (first_trial[i] + b - seg_start[i]) mod 2^32.
//  n_sc > 0: the in-band columns, n_cols = n_sc, column k at FFT bin b(k) (modulation.py:266-267);
//  n_sc = 0: every bin, n_cols = n_fft.
//  out64 or out32 (the other null): complex128, or complex64 rounded to nearest.
//  taps  null, or [n_blocks][n_ant][L] complex128: the taps themselves.
//  blob  the device copy of TdlHost::blob().
// Every cell is written once, by plain vector stores; no atomics.
hipError_t launch_tdl(hipStream_t st, const TdlHost& prof, const double* blob, const TdlSeg* segs,
                      const uint32_t* seg_start, int n_seg, uint32_t n_blocks, int n_sc, double2* out64, float2* out32,
                      double2* taps);

}  // namespace mimo
