// libmimo_engine: C-ABI host side of the MI355X Monte-Carlo BER engine.
//
// Coarse seam = mp_model.Link (mp_model.py:32-329).  mimo_engine_run launches the fused
// trial kernel (trial_kernel.h) over a batch of trials, reduces the per-trial counts on
// the device and adds the totals into the caller's counters, like Link.simulate adds
// into its shared mp.Array counters (mp_model.py:217-222).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mimo_engine.h"
#include "trial_launch.h"
#include "host_tables.h"
#ifndef MIMO_ONLY_F  // the single-size diagnostic builds link neither beam instances nor beam.o
#include "beam.h"
#endif

namespace {

using mimo::AlphaFit;
using mimo::fit_alpha;

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) return fail(MIMO_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

constexpr double kSpeedOfLight = 299792458.0;  // scipy.constants.c

bool is_pow2(long v) { return v > 0 && (v & (v - 1)) == 0; }

// Per-point sums of the per-trial counts of one launch: block (k, idx) adds the counts of
// trial blocks [first[k], first[k + 1]) -- a slice of at most kSlice trials of one point --
// into tot[point_of[k]][idx] (integer sums: the order does not matter; one 64-bit atomic
// per wave).
constexpr uint32_t kSlice = 4096;
__global__ void reduce_counts(const uint32_t* __restrict__ c, const uint32_t* __restrict__ first,
                              const int32_t* __restrict__ point_of, int n_idx, unsigned long long* __restrict__ tot) {
  const int k = blockIdx.x, idx = blockIdx.y;
  unsigned long long acc = 0;
  for (uint32_t t = first[k] + threadIdx.x; t < first[k + 1]; t += blockDim.x) acc += c[(size_t)t * n_idx + idx];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(&tot[(size_t)point_of[k] * n_idx + idx], acc);
}

// Per-slice sums of the measure instances' per-trial rows (doubles: the order matters, so it is
// fixed).  Block (k, col) sums column col over trial blocks [first[k], first[k + 1]): each thread
// its strided partial in trial order, a fixed shuffle tree per wave, the wave sums in wave order;
// one partial per (slice, column) into part[k][col], no atomics.  The host adds the slice
// partials of a point in slice order, so equal calls give bit-identical totals.
constexpr int kReduceMeasThreads = 256;
__global__ __launch_bounds__(kReduceMeasThreads) void reduce_meas(const double* __restrict__ rows,
                                                                  const uint32_t* __restrict__ first, int n_meas,
                                                                  double* __restrict__ part) {
  __shared__ double wsum[kReduceMeasThreads / 64];
  const int k = blockIdx.x, col = blockIdx.y;
  double acc = 0.0;
  for (uint32_t t = first[k] + threadIdx.x; t < first[k + 1]; t += kReduceMeasThreads)
    acc += rows[(size_t)t * n_meas + col];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wsum[0];
#pragma unroll
    for (int w = 1; w < kReduceMeasThreads / 64; ++w) s += wsum[w];
    part[(size_t)k * n_meas + col] = s;
  }
}

// Per-slice sums of the spectrum instances' per-trial rows (n_spec = F + MIMO_SPEC_FIXED columns,
// thousands of them, and at most kSlice rows per slice): block (k, tile) gives each thread one
// column, which it sums over trial blocks [first[k], first[k + 1]) in trial order -- the loads of
// a row coalesce across the threads' columns; one partial per (slice, column), no atomics.  The
// host adds the slice partials of a point in launch and slice order, as for reduce_meas.
constexpr int kReduceSpecThreads = 256;
__global__ __launch_bounds__(kReduceSpecThreads) void reduce_spec(const double* __restrict__ rows,
                                                                  const uint32_t* __restrict__ first, int n_spec,
                                                                  double* __restrict__ part) {
  const int k = blockIdx.x, col = blockIdx.y * kReduceSpecThreads + threadIdx.x;
  if (col >= n_spec) return;
  double acc = 0.0;
  for (uint32_t t = first[k]; t < first[k + 1]; ++t) acc += rows[(size_t)t * n_spec + col];
  part[(size_t)k * n_spec + col] = acc;
}

}  // namespace

namespace mimo {
void set_error(const std::string& m) { g_err = m; }
}  // namespace mimo

struct mimo_engine {
  mimo_config cfg{};
  std::vector<double> tx_pos, freqs;
  std::vector<double> chan_inband;        // MIMO_CH_TABLE: [A][S] (re, im), sub-carrier order k
  mimo_point pt{};
  bool have_point = false;
  // device state (created lazily on the first run: fork safety)
  bool ready = false;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float2* d_tw[2] = {nullptr, nullptr};  // fp32 stage twiddles for team_size(F), alt_team_size(F)
  double2* d_tw64 = nullptr;              // fp64 stage twiddles for team_size64(F)
  double2* d_twave64 = nullptr;           // wave-split FFT twiddles (wave_fft.h) where the instance uses it
  float2* d_twave32 = nullptr;
  double2* d_lut64 = nullptr;             // fp64 Box-Muller tables (lut64_table)
  float2* d_tab32 = nullptr;              // MIMO_CH_TABLE channel, fp32 / fp64 copies
  double2* d_tab64 = nullptr;
  float* d_ant_rel = nullptr;
  float* d_f_rel = nullptr;
  double* d_ant_rel64 = nullptr;
  double* d_f_rel64 = nullptr;
  double* d_f_over_c = nullptr;
  double* d_tx_pos = nullptr;
  uint32_t* d_counts = nullptr;
  size_t counts_cap = 0;
  unsigned long long* d_tot = nullptr;    // [points][n_idx] totals of one run
  size_t tot_cap = 0;
  // measure calls (mimo_engine_measure_points): per-trial rows of one launch, per-slice partials
  double* d_meas = nullptr;               // [launch blocks][n_meas]
  size_t meas_cap = 0;
  double* d_mpart = nullptr;              // [launch slices][n_meas]
  size_t mpart_cap = 0;
  // spectrum calls (mimo_engine_spectrum_points): the same pair, rows of n_fft + MIMO_SPEC_FIXED;
  // d_spec holds at most MIMO_SPEC_BUFFER_BYTES (it bounds the trials of a spectrum launch)
  double* d_spec = nullptr;               // [launch blocks][n_spec]
  size_t spec_cap = 0;
  double* d_spart = nullptr;              // [launch slices][n_spec]
  size_t spart_cap = 0;
  // beam calls (mimo_engine_beam_points): the beam instances' cells of one launch (at most the
  // beam buffer's bytes: it bounds the trials of a beam launch), the probe geometry, and the
  // same pair of per-trial rows and slice partials, rows of n_probes MIMO_BEAM_FIXED
  double* d_bcell = nullptr;              // [2][launch blocks][A][F] complex128
  size_t bcell_cap = 0;
  double* d_bgeo = nullptr;               // dist [n_probes][A] | 1 / dist [n_probes][A] | f / c [F]
  size_t bgeo_cap = 0;
  double* d_beam = nullptr;               // [launch blocks][n_probes][MIMO_BEAM_FIXED]
  size_t beam_cap = 0;
  double* d_bpart = nullptr;              // [launch slices][n_probes][MIMO_BEAM_FIXED]
  size_t bpart_cap = 0;
  hipEvent_t ev2 = nullptr;               // after the beamforming kernel of a launch
  double last_beam_ms = 0.0;
  // per-launch tables in one device blob, filled by one copy from a pinned host buffer:
  // TrialParams<R>[segments] | uint32 block offsets [segments + 1] |
  // uint32 reduction-slice starts [slices + 1] (<= kSlice trials, one point each) | int32 point of slice [slices]
  char* d_blob = nullptr;
  char* h_blob = nullptr;
  size_t blob_cap = 0, hblob_cap = 0;
  double d0 = 1.0;
  double last_ms = 0.0;
  // fit_alpha results per IBO (bit pattern of 10^(IBO/10)): the long-double fit costs
  // ~0.3 ms, paid once per IBO instead of once per point and batch of a sweep
  std::unordered_map<uint64_t, AlphaFit> alpha_fits;
  std::string desc;
};

namespace {

int team_for(int F) { return mimo::team_size(F); }

mimo::InstanceKey select_instance(const mimo_engine* e, bool csi) {
  mimo::InstanceKey k{};
  k.F = e->cfg.n_fft;
  k.f64 = e->cfg.precision != MIMO_PREC_F32;
  const int S = e->cfg.n_sub_carr;
  auto aligned_at = [&](int T) {
    const int P = k.F / T;
    return (S % (4 * T) == 0) && S < k.F && (S / T == 8 || S / T == 4) && (S / T) < P;
  };
  k.T = k.f64 ? mimo::team_size64(k.F) : team_for(k.F);
  if (k.f64) {  // one team size per fp64 instance
    const int P = k.F / k.T;
    k.aligned = aligned_at(k.T);
    k.nslot = k.aligned ? S / k.T : P;
    k.ch = e->cfg.channel_kind;
    k.csi = csi;
    return k;
  }
  // Unaligned bands (S % 4T != 0) run the generic predicated path with P slots per
  // thread; the alternative team has half the points per thread, which measured 1.5x
  // faster there (60.7 vs 40.7 ms at S = 1000, F = 2048; profiles/r01/ab_generic.json).
  if (!aligned_at(k.T) && mimo::alt_team_size(k.F) != k.T) k.T = mimo::alt_team_size(k.F);
  if (const char* env = std::getenv("MIMO_TEAM")) {  // A/B override: MIMO_TEAM=<threads per trial>
    const int t = std::atoi(env);
    if (t == mimo::alt_team_size(k.F) || t == mimo::team_size(k.F)) k.T = t;
  }
  const int P = k.F / k.T;
  k.aligned = aligned_at(k.T);
  k.nslot = k.aligned ? S / k.T : P;
  k.ch = e->cfg.channel_kind;
  k.csi = csi;
  return k;
}

template <typename R>
hipError_t launch(const mimo::InstanceKey& k, dim3 grid, hipStream_t st, const mimo::TrialParams<R>& p, bool* found,
                  hipFuncAttributes* attr = nullptr) {
  constexpr bool F64 = sizeof(R) == 8;
#define MIMO_LAUNCH_F(FV)                                                                    \
  if constexpr (F64) return mimo::launch_trial_F##FV##_f64(k, grid, st, p, found, attr);     \
  else return mimo::launch_trial_F##FV##_f32(k, grid, st, p, found, attr);
#ifdef MIMO_ONLY_F  // single-size diagnostic / A-B builds (Makefile targets ablation, variant)
  if (k.F == MIMO_ONLY_F) {
#if MIMO_ONLY_F == 2048
    MIMO_LAUNCH_F(2048)
#elif MIMO_ONLY_F == 4096
    MIMO_LAUNCH_F(4096)
#elif MIMO_ONLY_F == 8192
    MIMO_LAUNCH_F(8192)
#endif
  }
  *found = false;
  return hipSuccess;
#else
  switch (k.F) {
    case 128: MIMO_LAUNCH_F(128)
    case 256: MIMO_LAUNCH_F(256)
    case 512: MIMO_LAUNCH_F(512)
    case 1024: MIMO_LAUNCH_F(1024)
    case 2048: MIMO_LAUNCH_F(2048)
    case 4096: MIMO_LAUNCH_F(4096)
    case 8192: MIMO_LAUNCH_F(8192)
    default: *found = false; return hipSuccess;
  }
#endif
#undef MIMO_LAUNCH_F
}

// The measure instance of the key (float64 only); rows: [grid.x][n_meas] doubles.
hipError_t launch_meas(const mimo::InstanceKey& k, dim3 grid, hipStream_t st, const mimo::TrialParams<double>& p,
                       double* rows, bool* found) {
  *found = false;
#ifndef MIMO_ONLY_F  // the single-size diagnostic builds link no measure instances
  switch (k.F) {
    case 128: return mimo::launch_trial_F128_f64_meas(k, grid, st, p, found, nullptr, rows);
    case 256: return mimo::launch_trial_F256_f64_meas(k, grid, st, p, found, nullptr, rows);
    case 512: return mimo::launch_trial_F512_f64_meas(k, grid, st, p, found, nullptr, rows);
    case 1024: return mimo::launch_trial_F1024_f64_meas(k, grid, st, p, found, nullptr, rows);
    case 2048: return mimo::launch_trial_F2048_f64_meas(k, grid, st, p, found, nullptr, rows);
    case 4096: return mimo::launch_trial_F4096_f64_meas(k, grid, st, p, found, nullptr, rows);
    case 8192: return mimo::launch_trial_F8192_f64_meas(k, grid, st, p, found, nullptr, rows);
    default: break;
  }
#endif
  return hipSuccess;
}

// The spectrum instance of the key (float64 only); rows: [grid.x][F + MIMO_SPEC_FIXED] doubles.
hipError_t launch_spec(const mimo::InstanceKey& k, dim3 grid, hipStream_t st, const mimo::TrialParams<double>& p,
                       double* rows, bool* found) {
  *found = false;
#ifndef MIMO_ONLY_F  // the single-size diagnostic builds link no spectrum instances
  switch (k.F) {
    case 128: return mimo::launch_trial_F128_f64_spec(k, grid, st, p, found, nullptr, rows);
    case 256: return mimo::launch_trial_F256_f64_spec(k, grid, st, p, found, nullptr, rows);
    case 512: return mimo::launch_trial_F512_f64_spec(k, grid, st, p, found, nullptr, rows);
    case 1024: return mimo::launch_trial_F1024_f64_spec(k, grid, st, p, found, nullptr, rows);
    case 2048: return mimo::launch_trial_F2048_f64_spec(k, grid, st, p, found, nullptr, rows);
    case 4096: return mimo::launch_trial_F4096_f64_spec(k, grid, st, p, found, nullptr, rows);
    case 8192: return mimo::launch_trial_F8192_f64_spec(k, grid, st, p, found, nullptr, rows);
    default: break;
  }
#endif
  return hipSuccess;
}

// The beam instance of the key (float64 only); cells: [2][grid.x][A][F] complex128.
hipError_t launch_beam_inst(const mimo::InstanceKey& k, dim3 grid, hipStream_t st, const mimo::TrialParams<double>& p,
                            double* cells, bool* found) {
  *found = false;
#ifndef MIMO_ONLY_F  // the single-size diagnostic builds link no beam instances
  switch (k.F) {
    case 128: return mimo::launch_trial_F128_f64_beam(k, grid, st, p, found, nullptr, cells);
    case 256: return mimo::launch_trial_F256_f64_beam(k, grid, st, p, found, nullptr, cells);
    case 512: return mimo::launch_trial_F512_f64_beam(k, grid, st, p, found, nullptr, cells);
    case 1024: return mimo::launch_trial_F1024_f64_beam(k, grid, st, p, found, nullptr, cells);
    case 2048: return mimo::launch_trial_F2048_f64_beam(k, grid, st, p, found, nullptr, cells);
    case 4096: return mimo::launch_trial_F4096_f64_beam(k, grid, st, p, found, nullptr, cells);
    case 8192: return mimo::launch_trial_F8192_f64_beam(k, grid, st, p, found, nullptr, cells);
    default: break;
  }
#endif
  return hipSuccess;
}

// A beam call's probes, checked and turned into the beamforming kernel's tables by the caller
// (mimo_engine_beam_points): geo = dist [n_probes][A] | 1 / dist [n_probes][A] | f / c [F].
struct BeamCall {
  int n_probes;
  std::vector<double> geo;
  uint64_t max_trials;  // of one launch: the cells of so many trials fit the beam buffer, their rows the rows buffer
};

int validate_config(const mimo_config* c) {
  if (!c) return fail(MIMO_EINVAL, "null config");
  if (!is_pow2(c->n_fft) || c->n_fft < 128 || c->n_fft > 8192)
    return fail(MIMO_EINVAL, "n_fft must be a power of two in [128, 8192]");
  if (c->n_sub_carr < 4 || c->n_sub_carr % 4 || c->n_sub_carr > c->n_fft - 2)
    return fail(MIMO_EINVAL, "n_sub_carr must be a multiple of 4 in [4, n_fft - 2] (modulation.py:266-267 overlap)");
  const int L = (int)std::lround(std::sqrt((double)c->constel_size));
  if (L * L != c->constel_size || !is_pow2(c->constel_size) || c->constel_size < 4 || c->constel_size > 4096)
    return fail(MIMO_EINVAL, "Constellation size must be a power of some number, only square QAM supported.");
  if (c->n_ant < 1 || c->n_ant > 4096) return fail(MIMO_EINVAL, "n_ant must be in [1, 4096]");
  if (c->channel_kind < MIMO_CH_RAYLEIGH || c->channel_kind > MIMO_CH_TABLE)
    return fail(MIMO_EINVAL, "unknown channel_kind");
  if (c->channel_kind == MIMO_CH_TABLE && !c->chan_table)
    return fail(MIMO_EINVAL, "chan_table is required for MIMO_CH_TABLE");
  if (c->receiver_kind != MIMO_RX_CNC && c->receiver_kind != MIMO_RX_MCNC)
    return fail(MIMO_EINVAL, "unknown receiver_kind");
  if (!c->tx_pos) return fail(MIMO_EINVAL, "tx_pos is required");
  if (c->precision != MIMO_PREC_F64 && c->precision != MIMO_PREC_F32)
    return fail(MIMO_EINVAL, "precision must be MIMO_PREC_F64 or MIMO_PREC_F32");
  if (c->chan_replay_period < 0) return fail(MIMO_EINVAL, "chan_replay_period must be >= 0");
  if (c->chan_replay_period > 0 && c->channel_kind != MIMO_CH_RAYLEIGH)
    return fail(MIMO_EINVAL, "chan_replay_period applies to the Rayleigh channel only");
  // the geometry (the rules stand next to mimo_config in mimo_engine.h); every test fails for NaN
  for (int i = 0; i < 3 * c->n_ant; ++i)
    if (!std::isfinite(c->tx_pos[i]))
      return fail(MIMO_EINVAL, "tx_pos must be finite (antenna " + std::to_string(i / 3) + ")");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(c->rx_pos[i])) return fail(MIMO_EINVAL, "rx_pos must be finite");
  if (!(c->rx_loc_var >= 0) || !std::isfinite(c->rx_loc_var))
    return fail(MIMO_EINVAL, "rx_loc_var must be finite and >= 0");
  if (!c->carrier_freqs) return fail(MIMO_EINVAL, "carrier_freqs is required");
  for (int k = 0; k < c->n_fft; ++k)
    if (!(c->carrier_freqs[k] > 0) || !std::isfinite(c->carrier_freqs[k]))
      return fail(MIMO_EINVAL, "carrier_freqs must be finite and > 0 (bin " + std::to_string(k) + ")");
  if (c->channel_kind == MIMO_CH_TABLE)
    for (size_t i = 0; i < (size_t)c->n_ant * c->n_fft * 2; ++i)
      if (!std::isfinite(c->chan_table[i]))
        return fail(MIMO_EINVAL, "chan_table must be finite (antenna " + std::to_string(i / 2 / c->n_fft) + ")");
  return MIMO_OK;
}

// The distances the channel divides by, checked by every run call before its first HIP call (an
// engine that is only created, described or given points may hold any finite positions): the
// Rayleigh attenuation's, from the nominal RX, and for LoS / two-path the centre the jitter is
// drawn around, (rx_pos[0], rx_pos[0], rx_pos[2]) (mp_model.py:192-199 uses rx_loc_x for the y
// coordinate too).  Table channels read no position.
int validate_distances(const mimo_engine* e) {
  const mimo_config& c = e->cfg;
  if (c.channel_kind == MIMO_CH_TABLE) return MIMO_OK;
  const bool moves = c.channel_kind == MIMO_CH_LOS || c.channel_kind == MIMO_CH_TWOPATH;
  // (the distance as ensure_device forms it: one that rounds to 0 or overflows is refused too)
  auto no_distance = [](const double* t, double x, double y, double z) {
    const double dx = t[0] - x, dy = t[1] - y, dz = t[2] - z, d = std::sqrt(dx * dx + dy * dy + dz * dz);
    return !(d > 0) || !std::isfinite(d);
  };
  for (int a = 0; a < c.n_ant; ++a) {
    const double* t = e->tx_pos.data() + 3 * a;
    if (no_distance(t, c.rx_pos[0], c.rx_pos[1], c.rx_pos[2]))
      return fail(MIMO_EINVAL, "rx_pos is no finite distance > 0 from antenna " + std::to_string(a) + " (tx_pos)");
    if (moves && no_distance(t, c.rx_pos[0], c.rx_pos[0], c.rx_pos[2]))
      return fail(MIMO_EINVAL, "rx_pos: the jitter's centre (rx_pos[0], rx_pos[0], rx_pos[2]) is no finite distance > 0 "
                               "from antenna " + std::to_string(a) + " (tx_pos)");
  }
  return MIMO_OK;
}

int validate_point(const mimo_engine* e, const mimo_point* pt) {
  auto bad_kind = [](int k) { return k < MIMO_PA_NONE || k > MIMO_PA_TOI; };
  auto saturates = [](int k) { return k == MIMO_PA_SOFTLIM || k == MIMO_PA_RAPP; };
  if (bad_kind(pt->pa_kind) || bad_kind(pt->cnc_pa_kind)) return fail(MIMO_EINVAL, "unknown PA kind");
  // every test below is written to fail for NaN (the rules stand next to mimo_point in mimo_engine.h)
  if (!std::isfinite(pt->ibo_db)) return fail(MIMO_EINVAL, "ibo_db must be finite");
  if (!std::isfinite(pt->snr_db)) return fail(MIMO_EINVAL, "snr_db must be finite");
  if (!(pt->avg_symbol_power > 0) || !std::isfinite(pt->avg_symbol_power))
    return fail(MIMO_EINVAL, "avg_symbol_power must be finite and > 0");
  if (!std::isfinite(pt->avg_symbol_power / std::pow(10.0, pt->snr_db / 10.0)))
    return fail(MIMO_EINVAL, "snr_db leaves no finite noise power avg_symbol_power / 10^(snr_db / 10)");
  if (saturates(pt->pa_kind) && !(pt->sat_pow > 0)) return fail(MIMO_EINVAL, "sat_pow must be > 0");
  if (pt->pa_kind == MIMO_PA_TOI && !std::isfinite(pt->toi_coeff)) return fail(MIMO_EINVAL, "toi_coeff must be finite");
  // the receiver's own PA copy: read by the CNC loop only (MCNC re-transmits through the array's PA)
  const bool cnc = e->cfg.receiver_kind == MIMO_RX_CNC;
  if (cnc && saturates(pt->cnc_pa_kind) && !(pt->cnc_sat_pow > 0)) return fail(MIMO_EINVAL, "cnc_sat_pow must be > 0");
  if (cnc && pt->cnc_pa_kind == MIMO_PA_TOI && !std::isfinite(pt->cnc_toi_coeff))
    return fail(MIMO_EINVAL, "cnc_toi_coeff must be finite");
  // one hardness for both Rapp models
  if ((pt->pa_kind == MIMO_PA_RAPP || (cnc && pt->cnc_pa_kind == MIMO_PA_RAPP)) &&
      (!(pt->p_hardness > 0) || !std::isfinite(pt->p_hardness)))
    return fail(MIMO_EINVAL, "p_hardness must be finite and > 0");
  if (!(pt->cnc_alpha != 0) || !std::isfinite(pt->cnc_alpha))
    return fail(MIMO_EINVAL, "cnc_alpha must be finite and non-zero");
  if (std::isnan(pt->csi_eps)) return fail(MIMO_EINVAL, "csi_eps must be a number (< 0: perfect CSI)");
  if (pt->csi_eps >= 1.0) return fail(MIMO_EINVAL, "csi_eps must be < 1");
  if (pt->csi_eps >= 0 && e->cfg.n_ant > mimo::kMaxCsiAnt) return fail(MIMO_EINVAL, "CSI error supports n_ant <= 512");
  if (!(pt->array_alpha >= 0) || !std::isfinite(pt->array_alpha))
    return fail(MIMO_EINVAL, "array_alpha must be finite and >= 0");
  // the float32 F 8192 instance forms alpha by the library formula only (no polynomial to hold a constant)
  if (pt->array_alpha > 0 && e->cfg.precision == MIMO_PREC_F32 && e->cfg.n_fft == 8192)
    return fail(MIMO_EINVAL, "array_alpha needs float64 or n_fft <= 4096");
  return MIMO_OK;
}

// Per-point fields of the kernel parameters (the reference's per-point object state).
template <typename R>
void fill_point(mimo_engine* e, const mimo_point& pt, uint64_t seed, uint64_t first_trial,
                mimo::TrialParams<R>& p) {
  const mimo_config& c = e->cfg;
  const bool csi = pt.csi_eps >= 0;
  p.seed = seed;
  p.csi_seed = c.csi_seed ? c.csi_seed : seed;  // used by CH_TABLE + CSI only
  p.first_trial = first_trial;
  p.pa_kind = pt.pa_kind;
  p.cnc_pa_kind = pt.cnc_pa_kind;
  p.sat_tx = (R)pt.sat_pow;
  p.sqrt_sat_tx = (R)std::sqrt(std::max(pt.sat_pow, 0.0));
  p.inv_sat_tx = pt.sat_pow > 0 ? (R)(1.0 / pt.sat_pow) : R(0);
  p.rapp_p = (R)pt.p_hardness;
  p.toi_tx = (R)pt.toi_coeff;
  p.sat_cnc = (R)pt.cnc_sat_pow;
  p.sqrt_sat_cnc = (R)std::sqrt(std::max(pt.cnc_sat_pow, 0.0));
  p.inv_sat_cnc = pt.cnc_sat_pow > 0 ? (R)(1.0 / pt.cnc_sat_pow) : R(0);
  p.toi_cnc = (R)pt.cnc_toi_coeff;
  p.inv_alpha_cnc = (R)(1.0 / pt.cnc_alpha);
  p.alpha_c = (R)(std::pow(10.0, pt.ibo_db / 10.0) * c.n_sub_carr / c.n_ant);
  {
    const double g0sq = std::pow(10.0, pt.ibo_db / 10.0);
    uint64_t key;
    std::memcpy(&key, &g0sq, sizeof key);
    auto it = e->alpha_fits.find(key);
    if (it == e->alpha_fits.end()) {
      if (e->alpha_fits.size() >= 4096) e->alpha_fits.clear();
      it = e->alpha_fits.emplace(key, fit_alpha(g0sq)).first;
    }
    const AlphaFit& af = it->second;
    for (int i = 0; i < 9; ++i) p.apoly[i] = (R)af.apoly[i];
    p.alpha_xlim = (R)af.xlim;
    for (int k = 0; k < 19; ++k) p.amono64[k] = af.amono[k];
  }
  if (pt.array_alpha > 0) {
    // one fixed gain for every antenna: the kernel's alpha polynomial made the constant over
    // the whole range (the Horner sums then return it exactly)
    for (int i = 0; i < 9; ++i) p.apoly[i] = i == 0 ? (R)pt.array_alpha : R(0);
    for (int k = 0; k < 19; ++k) p.amono64[k] = k == 0 ? pt.array_alpha : 0.0;
    p.alpha_xlim = std::numeric_limits<R>::max();
  }
  p.es_over_snr = (R)(pt.avg_symbol_power / std::pow(10.0, pt.snr_db / 10.0));
  p.csi_a = csi ? (R)std::sqrt(1.0 - pt.csi_eps * pt.csi_eps) : R(1);
  p.csi_b = csi ? (R)pt.csi_eps : R(0);
}

template <typename T>
int ensure_cap(T*& ptr, size_t& cap, size_t need) {
  if (need <= cap) return MIMO_OK;
  if (ptr) HIP_TRY(hipFree(ptr));
  ptr = nullptr;
  HIP_TRY(hipMalloc(&ptr, need * sizeof(T)));
  cap = need;
  return MIMO_OK;
}

int ensure_device(mimo_engine* e) {
  if (e->ready) return MIMO_OK;
  if (e->cfg.device >= 0) HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipGetDevice(&e->device));
  HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&e->ev0));
  HIP_TRY(hipEventCreate(&e->ev1));
  HIP_TRY(hipEventCreate(&e->ev2));
  const int F = e->cfg.n_fft, S = e->cfg.n_sub_carr, A = e->cfg.n_ant;
  // the FFT tables (host_tables.h): the team FFT's per team size, the split FFT's in place of
  // the fp64 team's where the instance runs it, the wave-split FFT's where used
  const mimo::TwToF32 to_f32;
  const mimo::TwToF64 to_f64;
  std::vector<float2> tws[2] = {mimo::team_twiddles(F, mimo::team_size(F), to_f32),
                                mimo::team_twiddles(F, mimo::alt_team_size(F), to_f32)};
  std::vector<double2> tw64 = mimo::team_twiddles(F, mimo::team_size64(F), to_f64);
  if (mimo::split_fft_used(F, mimo::team_size64(F), true)) {
    const int T = mimo::team_size64(F);
    tw64 = mimo::split_twiddles(F, T);
    if ((int)tw64.size() != mimo::split_fft_tw_total(F, T)) return MIMO_ENOKERNEL;  // table and kernel disagree
  }
  std::vector<double2> twave64;
  std::vector<float2> twave32;
  if (mimo::wave_fft_used(F, mimo::team_size64(F), true)) twave64 = mimo::wave_twiddles(F, mimo::team_size64(F), to_f64);
  if (mimo::wave_fft_used(F, mimo::team_size(F), false)) twave32 = mimo::wave_twiddles(F, mimo::team_size(F), to_f32);
  // in-band sub-carrier k -> bin (modulation.py:266-267)
  std::vector<float> f_rel(S);
  std::vector<double> f_rel64(S), f_over_c(S);
  const double fc = e->freqs[0];  // bin 0 = centre frequency
  for (int k = 0; k < S; ++k) {
    const int bin = k < S / 2 ? F - S / 2 + k : k - S / 2 + 1;
    const double f = e->freqs[bin];
    // table channels carry their full attenuation: nothing is factored out of the loops
    f_rel64[k] = e->cfg.channel_kind == MIMO_CH_TABLE ? 1.0 : fc / f;
    f_rel[k] = (float)f_rel64[k];
    f_over_c[k] = f / kSpeedOfLight;
  }
  // Rayleigh FSPL at the nominal RX (channel.py:216-225), relative to the nearest antenna
  std::vector<double> dist(A);
  double dmin = 1e300;
  for (int a = 0; a < A; ++a) {
    const double dx = e->tx_pos[3 * a] - e->cfg.rx_pos[0], dy = e->tx_pos[3 * a + 1] - e->cfg.rx_pos[1],
                 dz = e->tx_pos[3 * a + 2] - e->cfg.rx_pos[2];
    dist[a] = std::sqrt(dx * dx + dy * dy + dz * dz);
    dmin = std::min(dmin, dist[a]);
  }
  e->d0 = dmin > 0 ? dmin : 1.0;
  std::vector<float> ant_rel(A);
  std::vector<double> ant_rel64(A);
  for (int a = 0; a < A; ++a) {
    ant_rel64[a] = e->d0 / dist[a];
    ant_rel[a] = (float)ant_rel64[a];
  }

  for (int v = 0; v < 2; ++v) {
    HIP_TRY(hipMalloc(&e->d_tw[v], sizeof(float2) * tws[v].size()));
    HIP_TRY(hipMemcpy(e->d_tw[v], tws[v].data(), sizeof(float2) * tws[v].size(), hipMemcpyHostToDevice));
  }
  if (!e->chan_inband.empty()) {
    const size_t n = e->chan_inband.size() / 2;
    std::vector<float2> t32(n);
    for (size_t i = 0; i < n; ++i) t32[i] = make_float2((float)e->chan_inband[2 * i], (float)e->chan_inband[2 * i + 1]);
    HIP_TRY(hipMalloc(&e->d_tab32, sizeof(float2) * n));
    HIP_TRY(hipMalloc(&e->d_tab64, sizeof(double2) * n));
    HIP_TRY(hipMemcpy(e->d_tab32, t32.data(), sizeof(float2) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_tab64, e->chan_inband.data(), sizeof(double2) * n, hipMemcpyHostToDevice));
  }
  const std::vector<double2> lut = mimo::lut64_table();
  HIP_TRY(hipMalloc(&e->d_lut64, sizeof(double2) * lut.size()));
  HIP_TRY(hipMemcpy(e->d_lut64, lut.data(), sizeof(double2) * lut.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&e->d_tw64, sizeof(double2) * tw64.size()));
  HIP_TRY(hipMemcpy(e->d_tw64, tw64.data(), sizeof(double2) * tw64.size(), hipMemcpyHostToDevice));
  if (!twave64.empty()) {
    HIP_TRY(hipMalloc(&e->d_twave64, sizeof(double2) * twave64.size()));
    HIP_TRY(hipMemcpy(e->d_twave64, twave64.data(), sizeof(double2) * twave64.size(), hipMemcpyHostToDevice));
  }
  if (!twave32.empty()) {
    HIP_TRY(hipMalloc(&e->d_twave32, sizeof(float2) * twave32.size()));
    HIP_TRY(hipMemcpy(e->d_twave32, twave32.data(), sizeof(float2) * twave32.size(), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMalloc(&e->d_f_rel64, sizeof(double) * S));
  HIP_TRY(hipMalloc(&e->d_ant_rel64, sizeof(double) * A));
  HIP_TRY(hipMemcpy(e->d_f_rel64, f_rel64.data(), sizeof(double) * S, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_ant_rel64, ant_rel64.data(), sizeof(double) * A, hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&e->d_f_rel, sizeof(float) * S));
  HIP_TRY(hipMalloc(&e->d_f_over_c, sizeof(double) * S));
  HIP_TRY(hipMalloc(&e->d_ant_rel, sizeof(float) * A));
  HIP_TRY(hipMalloc(&e->d_tx_pos, sizeof(double) * 3 * A));
  HIP_TRY(hipMemcpy(e->d_f_rel, f_rel.data(), sizeof(float) * S, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_f_over_c, f_over_c.data(), sizeof(double) * S, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_ant_rel, ant_rel.data(), sizeof(float) * A, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_tx_pos, e->tx_pos.data(), sizeof(double) * 3 * A, hipMemcpyHostToDevice));
  e->ready = true;
  return MIMO_OK;
}

}  // namespace

extern "C" {

int32_t mimo_abi_version(void) { return MIMO_ABI_VERSION; }
const char* mimo_last_error(void) { return g_err.c_str(); }

int32_t mimo_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

mimo_engine* mimo_engine_create(const mimo_config* cfg) {
  if (validate_config(cfg) != MIMO_OK) return nullptr;
  auto* e = new mimo_engine();
  e->cfg = *cfg;
  const int A = cfg->n_ant, F = cfg->n_fft;
  e->tx_pos.assign(cfg->tx_pos, cfg->tx_pos + 3 * A);
  e->freqs.assign(cfg->carrier_freqs, cfg->carrier_freqs + F);
  e->cfg.tx_pos = nullptr;
  e->cfg.carrier_freqs = nullptr;
  if (cfg->channel_kind == MIMO_CH_TABLE) {  // keep the in-band columns, bins b(k) (modulation.py:266-267)
    const int S = cfg->n_sub_carr;
    e->chan_inband.resize((size_t)A * S * 2);
    for (int a = 0; a < A; ++a)
      for (int k = 0; k < S; ++k) {
        const int bin = k < S / 2 ? F - S / 2 + k : k - S / 2 + 1;
        e->chan_inband[((size_t)a * S + k) * 2] = cfg->chan_table[((size_t)a * F + bin) * 2];
        e->chan_inband[((size_t)a * S + k) * 2 + 1] = cfg->chan_table[((size_t)a * F + bin) * 2 + 1];
      }
  }
  e->cfg.chan_table = nullptr;
  return e;
}

int32_t mimo_engine_set_point(mimo_engine* e, const mimo_point* pt) {
  if (!e || !pt) return fail(MIMO_EINVAL, "null argument");
  if (int rc = validate_point(e, pt)) return rc;
  e->pt = *pt;
  e->have_point = true;
  return MIMO_OK;
}

}  // extern "C"

namespace {

// Runs n_points grid points of one system in as few launches as possible: every point's
// trials become a contiguous range of blocks of one launch (split across launches only
// beyond kChunk blocks), and a segmented reduction sums each point's counts.
// meas_out != null (mimo_engine_measure_points): the measure instance runs instead, and its
// per-trial rows of n_meas = MIMO_MEAS_FIXED + n_idx sums are reduced per slice on the device
// (reduce_meas) and per point, in slice order, here.
// spec (mimo_engine_spectrum_points): meas_out / per_trial_meas are the spectrum rows instead, of
// n_fft + MIMO_SPEC_FIXED sums; the spectrum instance runs, reduce_spec forms the slice partials,
// and a launch holds no more trials than its rows fit MIMO_SPEC_BUFFER_BYTES.
// beam (mimo_engine_beam_points): the rows are n_probes MIMO_BEAM_FIXED sums; the beam instance
// runs and fills the launch's cells, the beamforming kernel (beam.hip) forms the per-trial rows
// from them, reduce_spec the slice partials; a launch holds beam->max_trials trials at most.
int run_points(mimo_engine* e, int n_points, const mimo_point* pts, const uint64_t* seeds,
               const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters, int32_t n_iters,
               int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out, uint32_t* per_trial,
               double* meas_out = nullptr, double* per_trial_meas = nullptr, bool spec = false,
               const BeamCall* beam = nullptr) {
  if (n_points < 0) return fail(MIMO_EINVAL, "n_points must be >= 0");
  if (n_iters < 1 || !iters) return fail(MIMO_EINVAL, "at least one iteration index is required");
  uint32_t rec_mask = 0;
  int max_iter = -1;
  for (int i = 0; i < n_iters; ++i) {
    if (iters[i] < 0 || iters[i] > 31) return fail(MIMO_EINVAL, "iterations must be in [0, 31]");
    if (i && iters[i] <= iters[i - 1]) return fail(MIMO_EINVAL, "iterations must be sorted and unique");
    rec_mask |= 1u << iters[i];
    max_iter = std::max(max_iter, (int)iters[i]);
  }
  if (!err_out || !bits_out) return fail(MIMO_EINVAL, "null counters");
  if (n_points == 0) return MIMO_OK;
  if (!pts || !seeds || !first_trial || !n_trials) return fail(MIMO_EINVAL, "null point arrays");
  const int n_idx = n_iters + (incl_clean ? 1 : 0);
  const mimo_config& c = e->cfg;
  const int n_meas = beam   ? beam->n_probes * MIMO_BEAM_FIXED  // row width of the mode
                     : spec ? c.n_fft + MIMO_SPEC_FIXED
                            : MIMO_MEAS_FIXED + n_idx;
  const bool csi = pts[0].csi_eps >= 0;
  for (int i = 0; i < n_points; ++i) {
    if (int rc = validate_point(e, &pts[i])) return rc;
    if ((pts[i].csi_eps >= 0) != csi) return fail(MIMO_EINVAL, "all points of one run must agree on CSI error on/off");
    if (n_trials[i] + first_trial[i] > (1ull << 32) || first_trial[i] >= (1ull << 32))
      return fail(MIMO_EINVAL, "trial index must fit 32 bits");
  }
  if (int rc = validate_distances(e)) return rc;
  const mimo::InstanceKey key = select_instance(e, csi);
  if (int rc = ensure_device(e)) return rc;
  if (csi) {
    // the CSI instances add n_ant reals of dynamic LDS (the per-antenna power table) to their
    // static LDS: check the sum against the CU's LDS before launching (F 8192 holds
    // ~157 KiB statically, so A = 512 (4 KiB) is the edge)
    hipFuncAttributes fa{};
    bool found = false;
    hipError_t qe = key.f64 ? launch(key, dim3(0), e->stream, mimo::TrialParams<double>{}, &found, &fa)
                            : launch(key, dim3(0), e->stream, mimo::TrialParams<float>{}, &found, &fa);
    int lds_max = 0;
    if (found && qe == hipSuccess &&
        hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, e->device) == hipSuccess &&
        lds_max > 0) {
      const size_t need = fa.sharedSizeBytes + (size_t)c.n_ant * (key.f64 ? sizeof(double) : sizeof(float));
      if (need > (size_t)lds_max)
        return fail(MIMO_EINVAL, "CSI error at n_ant = " + std::to_string(c.n_ant) + " needs " + std::to_string(need) +
                                     " B of LDS per team (static " + std::to_string(fa.sharedSizeBytes) +
                                     " + the per-antenna table), the device has " + std::to_string(lds_max));
    }
  }
  if (!c.reroll_chan && (c.channel_kind == MIMO_CH_LOS || c.channel_kind == MIMO_CH_TWOPATH)) {
    // fixed RX: jitter span 0 around (x0, x0); only consistent when rx_y == rx_x
    // (table channels never use the RX position)
    if (c.rx_pos[1] != c.rx_pos[0]) return fail(MIMO_EINVAL, "reroll_chan=0 requires rx_pos[1] == rx_pos[0]");
  }
  char buf[160];
  snprintf(buf, sizeof buf, "F=%d T=%d slots=%d %s ch=%d csi=%d %s", key.F, key.T, key.nslot,
           key.aligned ? "aligned" : "generic", key.ch, (int)key.csi, key.f64 ? "f64" : "f32");
  e->desc = buf;

  // segments (point, first trial, count) packed into launches of <= kChunk blocks
  // Trials per launch: 2^20 (MIMO_MAX_LAUNCH_TRIALS lowers it, for tests of the splitting).
  uint64_t kChunk = 1ull << 20;
  if (const char* env = std::getenv("MIMO_MAX_LAUNCH_TRIALS")) {
    const uint64_t v = std::strtoull(env, nullptr, 10);
    if (v >= 1 && v < kChunk) kChunk = v;
  }
  if (spec) kChunk = std::min<uint64_t>(kChunk, MIMO_SPEC_BUFFER_BYTES / (sizeof(double) * (size_t)n_meas));
  if (beam) kChunk = std::min<uint64_t>(kChunk, beam->max_trials);
  double*& d_rows = beam ? e->d_beam : spec ? e->d_spec : e->d_meas;  // per-trial rows and slice partials of the mode
  size_t& rows_cap = beam ? e->beam_cap : spec ? e->spec_cap : e->meas_cap;
  double*& d_part = beam ? e->d_bpart : spec ? e->d_spart : e->d_mpart;
  size_t& part_cap = beam ? e->bpart_cap : spec ? e->spart_cap : e->mpart_cap;
  struct Seg {
    int point;
    uint64_t first, n;
  };
  std::vector<std::vector<Seg>> launches(1);
  uint64_t fill = 0;
  for (int i = 0; i < n_points; ++i) {
    uint64_t done = 0;
    while (done < n_trials[i]) {
      if (fill == kChunk) {
        launches.emplace_back();
        fill = 0;
      }
      const uint64_t n = std::min(n_trials[i] - done, kChunk - fill);
      launches.back().push_back(Seg{i, first_trial[i] + done, n});
      done += n;
      fill += n;
    }
  }
  size_t max_seg = 0;
  for (auto& l : launches) max_seg = std::max(max_seg, l.size());
  // measure calls: the slice partials of every launch, in launch and slice order, and their points
  std::vector<double> mpart;
  std::vector<int> mpart_point;
  if (meas_out) {
    size_t max_blocks = 0, max_sl = 0, tot_sl = 0;
    for (auto& l : launches) {
      size_t nb = 0, nsl = 0;
      for (auto& sg : l) {
        nb += (size_t)sg.n;
        nsl += (size_t)((sg.n + kSlice - 1) / kSlice);
      }
      max_blocks = std::max(max_blocks, nb);
      max_sl = std::max(max_sl, nsl);
      tot_sl += nsl;
    }
    if (int rc = ensure_cap(d_rows, rows_cap, std::max<size_t>(1, max_blocks * n_meas))) return rc;
    if (int rc = ensure_cap(d_part, part_cap, std::max<size_t>(1, max_sl * n_meas))) return rc;
    mpart.resize(tot_sl * n_meas);
    mpart_point.reserve(tot_sl);
    if (beam) {
      const size_t cells = 2 * max_blocks * (size_t)c.n_ant * (size_t)c.n_fft * 2;  // doubles
      if (int rc = ensure_cap(e->d_bcell, e->bcell_cap, std::max<size_t>(2, cells))) return rc;
      if (int rc = ensure_cap(e->d_bgeo, e->bgeo_cap, beam->geo.size())) return rc;
      HIP_TRY(hipMemcpyAsync(e->d_bgeo, beam->geo.data(), sizeof(double) * beam->geo.size(), hipMemcpyHostToDevice,
                             e->stream));
    }
  }
  size_t mpart_done = 0;
  if (int rc = ensure_cap(e->d_counts, e->counts_cap, (size_t)(1ull << 20) * n_idx)) return rc;
  if (int rc = ensure_cap(e->d_tot, e->tot_cap, (size_t)n_points * n_idx)) return rc;
  const size_t max_slices = max_seg + (size_t)(kChunk / kSlice) + 1;
  HIP_TRY(hipMemsetAsync(e->d_tot, 0, sizeof(unsigned long long) * n_points * n_idx, e->stream));
  double ms_total = 0.0, beam_ms_total = 0.0;
  uint64_t rows_done = 0;

  auto run_as = [&](auto zero) -> int {
    using R = decltype(zero);
    using TP = mimo::TrialParams<R>;
    constexpr bool F64 = sizeof(R) == 8;
    TP base{};
    if constexpr (F64) {
      base.tw = e->d_tw64;
      base.tw_wave = e->d_twave64;
      base.ant_rel = e->d_ant_rel64;
      base.f_rel = e->d_f_rel64;
      base.chan_tab = e->d_tab64;
    } else {
      base.tw = e->d_tw[key.T == mimo::team_size(c.n_fft) ? 0 : 1];
      base.tw_wave = key.T == mimo::team_size(c.n_fft) ? e->d_twave32 : nullptr;
      base.ant_rel = e->d_ant_rel;
      base.f_rel = e->d_f_rel;
      base.chan_tab = e->d_tab32;
    }
    base.f_over_c = e->d_f_over_c;
    base.tx_pos = e->d_tx_pos;
    base.lut = e->d_lut64;
    base.n_ant = c.n_ant;
    base.n_sc = c.n_sub_carr;
    const int L = (int)std::lround(std::sqrt((double)c.constel_size));
    base.qam_l = L;
    base.half_bits = (int)std::lround(std::log2((double)L));
    base.label_mask = (uint32_t)c.constel_size - 1u;
    base.inv_vk0 = (R)((double)c.n_ant / c.n_sub_carr);
    base.inv_vk0_f = (R)((double)c.n_ant * c.n_fft / c.n_sub_carr);
    base.inv_sqrt_f = (R)(1.0 / std::sqrt((double)c.n_fft));
    base.receiver = c.receiver_kind;
    base.max_iter = max_iter;
    base.rec_mask = rec_mask;
    base.incl_clean = incl_clean ? 1 : 0;
    base.n_idx = n_idx;
    base.rx_x0 = c.rx_pos[0];
    base.rx_z = c.rx_pos[2];
    base.rx_var = c.reroll_chan ? c.rx_loc_var : 0.0;
    base.d0 = e->d0;
    base.ablate = 0;
#ifdef MIMO_ABLATION
    if (const char* env = std::getenv("MIMO_ABLATE")) base.ablate = (uint32_t)std::strtoul(env, nullptr, 0);
#endif
    base.counts = e->d_counts;
    base.chan_period = (uint32_t)std::max(0, c.chan_replay_period);
    // per-point parameter table (host), built once
    std::vector<TP> ptab(n_points, base);
    for (int i = 0; i < n_points; ++i) fill_point(e, pts[i], seeds[i], 0, ptab[i]);
    auto up16 = [](size_t b) { return (b + 15) & ~size_t(15); };
    const size_t o_start = up16(max_seg * sizeof(TP)), o_slice = o_start + up16((max_seg + 1) * sizeof(uint32_t)),
                 o_pof = o_slice + up16((max_slices + 1) * sizeof(uint32_t)),
                 blob = o_pof + up16(max_slices * sizeof(int32_t));
    if (int rc = ensure_cap(e->d_blob, e->blob_cap, blob)) return rc;
    if (blob > e->hblob_cap) {
      if (e->h_blob) HIP_TRY(hipHostFree(e->h_blob));
      e->h_blob = nullptr;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->h_blob), blob, hipHostMallocDefault));
      e->hblob_cap = blob;
    }
    TP* seg_tab = reinterpret_cast<TP*>(e->h_blob);
    uint32_t* start = reinterpret_cast<uint32_t*>(e->h_blob + o_start);
    uint32_t* slice_first = reinterpret_cast<uint32_t*>(e->h_blob + o_slice);
    int32_t* point_of = reinterpret_cast<int32_t*>(e->h_blob + o_pof);
    for (auto& l : launches) {
      size_t nseg = 0, nsl = 0;
      start[0] = 0u;
      slice_first[0] = 0u;
      for (auto& sg : l) {
        TP q = ptab[sg.point];
        q.first_trial = sg.first;
        seg_tab[nseg] = q;
        const uint32_t b0 = start[nseg];
        start[++nseg] = b0 + (uint32_t)sg.n;
        for (uint32_t o = 0; o < (uint32_t)sg.n; o += kSlice) {
          slice_first[++nsl] = b0 + std::min<uint32_t>((uint32_t)sg.n, o + kSlice);
          point_of[nsl - 1] = sg.point;
        }
      }
      const uint32_t nb = start[nseg];
      if (nb == 0) continue;  // every point of the call has n_trials == 0: nothing to launch
      TP kp = base;
      kp.points = reinterpret_cast<const TP*>(e->d_blob);
      kp.point_start = reinterpret_cast<const uint32_t*>(e->d_blob + o_start);
      kp.n_points = (int)nseg;
      kp.seed = seg_tab[0].seed;  // unused by the kernel (read from the table)
      // the whole blob (unused tails included: one contiguous DMA)
      HIP_TRY(hipMemcpyAsync(e->d_blob, e->h_blob, o_pof + nsl * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
      HIP_TRY(hipEventRecord(e->ev0, e->stream));
      bool found = false;
      hipError_t le = hipSuccess;
      if constexpr (F64) {
        le = beam       ? launch_beam_inst(key, dim3(nb), e->stream, kp, e->d_bcell, &found)
             : spec     ? launch_spec(key, dim3(nb), e->stream, kp, d_rows, &found)
             : meas_out ? launch_meas(key, dim3(nb), e->stream, kp, d_rows, &found)
                        : launch(key, dim3(nb), e->stream, kp, &found);
      } else {
        le = launch(key, dim3(nb), e->stream, kp, &found);
      }
      if (!found) return fail(MIMO_ENOKERNEL, std::string("no kernel instance for ") + buf);
      if (le != hipSuccess) return fail(MIMO_EHIP, std::string("trial kernel launch: ") + hipGetErrorString(le));
      HIP_TRY(hipEventRecord(e->ev1, e->stream));
#ifndef MIMO_ONLY_F  // (the single-size diagnostic builds found no beam instance above)
      if (beam) {
        const size_t na = (size_t)beam->n_probes * (size_t)c.n_ant;
        const hipError_t be = mimo::launch_beam(e->stream, e->d_bcell, e->d_bgeo, e->d_bgeo + na, e->d_bgeo + 2 * na,
                                                (int)nb, c.n_ant, c.n_fft, c.n_sub_carr, beam->n_probes, d_rows);
        if (be != hipSuccess)
          return fail(MIMO_EHIP, std::string("beamforming kernel launch: ") + hipGetErrorString(be));
        HIP_TRY(hipEventRecord(e->ev2, e->stream));
      }
#endif
      hipLaunchKernelGGL(reduce_counts, dim3((unsigned)nsl, n_idx), dim3(256), 0, e->stream, e->d_counts,
                         reinterpret_cast<const uint32_t*>(e->d_blob + o_slice),
                         reinterpret_cast<const int32_t*>(e->d_blob + o_pof), n_idx, e->d_tot);
      HIP_TRY(hipGetLastError());
      if (per_trial)
        HIP_TRY(hipMemcpyAsync(per_trial + rows_done * n_idx, e->d_counts, (size_t)nb * n_idx * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, e->stream));
      if (meas_out) {
        if (spec || beam)
          hipLaunchKernelGGL(reduce_spec,
                             dim3((unsigned)nsl, (unsigned)((n_meas + kReduceSpecThreads - 1) / kReduceSpecThreads)),
                             dim3(kReduceSpecThreads), 0, e->stream, d_rows,
                             reinterpret_cast<const uint32_t*>(e->d_blob + o_slice), n_meas, d_part);
        else
          hipLaunchKernelGGL(reduce_meas, dim3((unsigned)nsl, n_meas), dim3(kReduceMeasThreads), 0, e->stream, d_rows,
                             reinterpret_cast<const uint32_t*>(e->d_blob + o_slice), n_meas, d_part);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(mpart.data() + mpart_done * n_meas, d_part, nsl * n_meas * sizeof(double),
                               hipMemcpyDeviceToHost, e->stream));
        for (size_t i = 0; i < nsl; ++i) mpart_point.push_back(point_of[i]);
        mpart_done += nsl;
        if (per_trial_meas)
          HIP_TRY(hipMemcpyAsync(per_trial_meas + rows_done * n_meas, d_rows, (size_t)nb * n_meas * sizeof(double),
                                 hipMemcpyDeviceToHost, e->stream));
      }
      rows_done += nb;
      // the host tables of the next launch are rewritten: wait for this one's copies
      HIP_TRY(hipEventSynchronize(e->ev1));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
      ms_total += ms;
      if (beam) {
        HIP_TRY(hipEventSynchronize(e->ev2));
        HIP_TRY(hipEventElapsedTime(&ms, e->ev1, e->ev2));
        beam_ms_total += ms;
      }
    }
    return MIMO_OK;
  };
  if (int rc = key.f64 ? run_as(0.0) : run_as(0.0f)) return rc;
  std::vector<unsigned long long> tot((size_t)n_points * n_idx);
  HIP_TRY(hipMemcpyAsync(tot.data(), e->d_tot, sizeof(unsigned long long) * tot.size(), hipMemcpyDeviceToHost,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const uint64_t bits_per_trial = (uint64_t)c.n_sub_carr * (uint64_t)std::lround(std::log2((double)c.constel_size));
  for (int i = 0; i < n_points; ++i)
    for (int j = 0; j < n_idx; ++j) {
      err_out[(size_t)i * n_idx + j] += tot[(size_t)i * n_idx + j];
      bits_out[(size_t)i * n_idx + j] += bits_per_trial * n_trials[i];
    }
  if (meas_out) {
    // per point, its slice partials in slice order (a fixed order: equal calls, equal bits),
    // then one add into the caller's row
    std::vector<double> ptot((size_t)n_points * n_meas, 0.0);
    for (size_t k = 0; k < mpart_point.size(); ++k)
      for (int j = 0; j < n_meas; ++j) ptot[(size_t)mpart_point[k] * n_meas + j] += mpart[k * n_meas + j];
    for (size_t i = 0; i < ptot.size(); ++i) meas_out[i] += ptot[i];
  }
  e->last_ms = ms_total;
  e->last_beam_ms = beam_ms_total;
  return MIMO_OK;
}

}  // namespace

extern "C" {

int32_t mimo_engine_run(mimo_engine* e, uint64_t seed, uint64_t first_trial, uint64_t n_trials, const int32_t* iters,
                        int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out, uint32_t* per_trial) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  if (!e->have_point) return fail(MIMO_EINVAL, "mimo_engine_set_point was not called");
  if (n_trials == 0) {  // validate the iteration list, add nothing
    return run_points(e, 0, nullptr, nullptr, nullptr, nullptr, iters, n_iters, incl_clean, err_out, bits_out,
                      per_trial);
  }
  return run_points(e, 1, &e->pt, &seed, &first_trial, &n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial);
}

int32_t mimo_engine_run_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                               const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                               int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                               uint32_t* per_trial) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  return run_points(e, n_points, points, seeds, first_trial, n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial);
}

int32_t mimo_measure_width(int32_t n_iters, int32_t incl_clean) {
  if (n_iters < 1 || n_iters > 32) return fail(MIMO_EINVAL, "n_iters must be in [1, 32]");
  return MIMO_MEAS_FIXED + n_iters + (incl_clean ? 1 : 0);
}

int32_t mimo_engine_measure_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                   const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                   int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                   uint32_t* per_trial, double* meas_out, double* per_trial_meas) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  if (e->cfg.precision != MIMO_PREC_F64)
    return fail(MIMO_EINVAL, "measure needs a float64 engine (no float32 measure instances are built)");
  if (!meas_out) return fail(MIMO_EINVAL, "null meas_out");
  return run_points(e, n_points, points, seeds, first_trial, n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial, meas_out, per_trial_meas);
}

int32_t mimo_spectrum_width(int32_t n_fft) {
  if (!is_pow2(n_fft) || n_fft < 128 || n_fft > 8192)
    return fail(MIMO_EINVAL, "n_fft must be a power of two in [128, 8192]");
  return n_fft + MIMO_SPEC_FIXED;
}

int32_t mimo_engine_spectrum_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                    const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                    int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                    uint32_t* per_trial, double* spec_out, double* per_trial_spec) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  if (e->cfg.precision != MIMO_PREC_F64)
    return fail(MIMO_EINVAL, "spectrum needs a float64 engine (no float32 spectrum instances are built)");
  if (!spec_out) return fail(MIMO_EINVAL, "null spec_out");
  return run_points(e, n_points, points, seeds, first_trial, n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial, spec_out, per_trial_spec, true);
}

int32_t mimo_beam_width(int32_t n_probes) {
  if (n_probes < 1 || n_probes > MIMO_BEAM_MAX_PROBES)
    return fail(MIMO_EINVAL, "n_probes must be in [1, " + std::to_string(MIMO_BEAM_MAX_PROBES) + "]");
  return n_probes * MIMO_BEAM_FIXED;
}

int32_t mimo_engine_beam_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                uint32_t* per_trial, const double* probes, int32_t n_probes, double* beam_out,
                                double* per_trial_beam) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  if (e->cfg.precision != MIMO_PREC_F64)
    return fail(MIMO_EINVAL, "beam needs a float64 engine (no float32 beam instances are built)");
  if (!probes) return fail(MIMO_EINVAL, "null probes");
  if (!beam_out) return fail(MIMO_EINVAL, "null beam_out");
  if (mimo_beam_width(n_probes) < 0) return MIMO_EINVAL;
  const int A = e->cfg.n_ant, F = e->cfg.n_fft;
  BeamCall bc;
  bc.n_probes = n_probes;
  // the launch's cells: Y and X of every antenna and bin, complex128
  const uint64_t per_trial_bytes = 2ull * (uint64_t)A * (uint64_t)F * 16ull;
  uint64_t buffer = MIMO_BEAM_BUFFER_BYTES;
  if (const char* env = std::getenv("MIMO_BEAM_BUFFER_BYTES")) {  // lowers it, for tests of the splitting
    const uint64_t v = std::strtoull(env, nullptr, 10);
    if (v >= 1 && v < buffer) buffer = v;
  }
  bc.max_trials = buffer / per_trial_bytes;
  if (bc.max_trials < 1)
    return fail(MIMO_EINVAL, "one trial's beam cells (" + std::to_string(per_trial_bytes) + " B at n_ant " +
                                 std::to_string(A) + ", n_fft " + std::to_string(F) +
                                 ") do not fit the beam buffer of " + std::to_string(buffer) + " B");
  // ... and its per-trial rows, as for the spectrum mode (one trial's 40 n_probes bytes always fit)
  bc.max_trials = std::min<uint64_t>(
      bc.max_trials, MIMO_BEAM_ROWS_BYTES / (sizeof(double) * (uint64_t)MIMO_BEAM_FIXED * (uint64_t)n_probes));
  const size_t na = (size_t)n_probes * (size_t)A;
  bc.geo.resize(2 * na + (size_t)F);
  for (int q = 0; q < n_probes; ++q) {
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(probes[3 * q + i])) return fail(MIMO_EINVAL, "probe " + std::to_string(q) + " is not finite");
    for (int a = 0; a < A; ++a) {
      const double dx = e->tx_pos[3 * a] - probes[3 * q], dy = e->tx_pos[3 * a + 1] - probes[3 * q + 1],
                   dz = e->tx_pos[3 * a + 2] - probes[3 * q + 2];
      // the squares rounded one by one and summed in this order, as oracle.refmath.los_channel does
      const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
      const double d = std::sqrt((xx + yy) + zz);
      if (!(d > 0) || !std::isfinite(d))
        return fail(MIMO_EINVAL, "probe " + std::to_string(q) + " coincides with antenna " + std::to_string(a) +
                                     " (or is too far): no LoS channel");
      bc.geo[(size_t)q * A + a] = d;
      bc.geo[na + (size_t)q * A + a] = 1.0 / d;
    }
  }
  for (int k = 0; k < F; ++k) bc.geo[2 * na + k] = e->freqs[k] / kSpeedOfLight;
  return run_points(e, n_points, points, seeds, first_trial, n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial, beam_out, per_trial_beam, false, &bc);
}

double mimo_engine_last_kernel_ms(const mimo_engine* e) { return e ? e->last_ms : 0.0; }
double mimo_engine_last_beam_ms(const mimo_engine* e) { return e ? e->last_beam_ms : 0.0; }

const char* mimo_engine_describe(const mimo_engine* e) {
  if (!e) return "";
  if (e->desc.empty()) {
    const mimo::InstanceKey k = select_instance(e, e->have_point && e->pt.csi_eps >= 0);
    char buf[160];
    snprintf(buf, sizeof buf, "F=%d T=%d slots=%d %s ch=%d csi=%d %s", k.F, k.T, k.nslot,
             k.aligned ? "aligned" : "generic", k.ch, (int)k.csi, k.f64 ? "f64" : "f32");
    const_cast<mimo_engine*>(e)->desc = buf;
  }
  return e->desc.c_str();
}

void mimo_engine_destroy(mimo_engine* e) {
  if (!e) return;
  if (e->ready) {
    (void)hipStreamSynchronize(e->stream);
    (void)hipFree(e->d_tw[0]);
    (void)hipFree(e->d_tw[1]);
    (void)hipFree(e->d_f_rel);
    (void)hipFree(e->d_tw64);
    if (e->d_twave64) (void)hipFree(e->d_twave64);
    if (e->d_twave32) (void)hipFree(e->d_twave32);
    (void)hipFree(e->d_lut64);
    if (e->d_tab32) (void)hipFree(e->d_tab32);
    if (e->d_tab64) (void)hipFree(e->d_tab64);
    (void)hipFree(e->d_f_rel64);
    (void)hipFree(e->d_ant_rel64);
    (void)hipFree(e->d_f_over_c);
    (void)hipFree(e->d_ant_rel);
    (void)hipFree(e->d_tx_pos);
    if (e->d_tot) (void)hipFree(e->d_tot);
    if (e->d_counts) (void)hipFree(e->d_counts);
    if (e->d_meas) (void)hipFree(e->d_meas);
    if (e->d_mpart) (void)hipFree(e->d_mpart);
    if (e->d_spec) (void)hipFree(e->d_spec);
    if (e->d_spart) (void)hipFree(e->d_spart);
    if (e->d_bcell) (void)hipFree(e->d_bcell);
    if (e->d_bgeo) (void)hipFree(e->d_bgeo);
    if (e->d_beam) (void)hipFree(e->d_beam);
    if (e->d_bpart) (void)hipFree(e->d_bpart);
    if (e->d_blob) (void)hipFree(e->d_blob);
    if (e->h_blob) (void)hipHostFree(e->h_blob);
    (void)hipEventDestroy(e->ev0);
    (void)hipEventDestroy(e->ev1);
    (void)hipEventDestroy(e->ev2);
    (void)hipStreamDestroy(e->stream);
  }
  delete e;
}

}  // extern "C"
