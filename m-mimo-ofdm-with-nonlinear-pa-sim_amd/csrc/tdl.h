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

// The ray-cluster profile (include/mimo_engine.h mimo_rays, mimo_engine_set_rays,
// mimo_rays_channels): the same generator with another first stage.  The workgroup draws the R ray
// gains of its trial, multiplies them by row a of steer into LDS and sums the L taps of its antenna
// from there; the response is tdl_response, unchanged.
//
// The arithmetic of a tap, fixed (the engine and the seam run the one kernel template).  Ray r's
// term is p_r = c_r steer[a][r], formed as tdl_response forms a product: four fused multiply-adds
// onto an accumulator that starts at (0, 0) -- re = fma(c.x, s.x, 0), re = fma(-c.y, s.y, re),
// im = fma(c.x, s.y, 0), im = fma(c.y, s.x, im).  With r0 the tap's first ray and n its ray count,
// lane j < 16 of the group of 16 adjacent lanes that owns the tap adds the terms of the rays
// r = r0 + j, r0 + j + 16, ... < r0 + n in ascending r onto (0, 0) by plain additions; the 16
// partial sums are then added pairwise over the lane distances 8, 4, 2 and 1 (lane j takes
// p[j] + p[j ^ d]; IEEE addition commutes, so all lanes hold the same bits).  A tap of up to 16 rays
// is therefore a binary tree over its terms, a longer one 16 ascending chains and the tree; a tap of
// one ray is that ray's term, and with steer = 1 + 0j the gain itself, bit for bit.
constexpr int kRaysMax = 1024;  // MIMO_RAYS_MAX

struct RaysHost {
  TdlHost tdl;  // delays and W; sqrt_pow and ant_amp are 1 and not read
  int n_rays = 0;
  std::vector<int32_t> ray_tap;    // [R]
  std::vector<int32_t> tap_first;  // [L + 1] tap l's rays are tap_first[l] ... tap_first[l + 1] - 1
  std::vector<double> ray_amp;     // [R]
  std::vector<uint8_t> ray_kind;   // [R]
  std::vector<double> steer;       // [A][R] (re, im)
  // The device blob: TdlHost::blob() | pad to 16 bytes | steer [A][R] double2 | ray_amp [R] |
  // tap_first [L + 1] int32 | ray_tap [R] int32 | ray_kind [R] uint8 (the last three in doubles' space).
  std::vector<double> blob() const;
  // offsets of the appended tables in doubles
  size_t off_steer() const;
  size_t off_amp() const { return off_steer() + 2 * (size_t)tdl.n_ant * n_rays; }
  size_t off_first() const { return off_amp() + n_rays; }
  size_t off_tap() const { return off_first() + (tdl.n_taps + 2) / 2; }
  size_t off_kind() const { return off_tap() + (n_rays + 1) / 2; }
};

// Checks every rule of include/mimo_engine.h's mimo_rays (host only) and copies the profile.
bool rays_prepare(const mimo_rays* prof, int n_ant, int n_fft, RaysHost* out, std::string* err);

// launch_tdl for a ray-cluster profile.  gains: null, or [n_blocks][R] complex128, the ray gains of
// block b's trial (written by the workgroups of antenna 0, every cell once).
hipError_t launch_rays(hipStream_t st, const RaysHost& prof, const double* blob, const TdlSeg* segs,
                       const uint32_t* seg_start, int n_seg, uint32_t n_blocks, int n_sc, double2* out64,
                       float2* out32, double2* taps, double2* gains);

}  // namespace mimo
