// libmimo_engine: C-ABI host side of the MI355X Monte-Carlo BER engine.
//
// Coarse seam = mp_model.Link (mp_model.py:32-329).  mimo_engine_run launches the fused
// trial kernel (trial_kernel.h; this file sees its contract alone, trial_params.h) over a batch
// of trials, reduces the per-trial counts on the device and adds the totals into the caller's
// counters, like Link.simulate adds into its shared mp.Array counters (mp_model.py:217-222).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/mimo_engine.h"
#include "host_util.h"
#include "trial_launch.h"
#include "host_tables.h"
#ifndef MIMO_ONLY_F  // the single-size diagnostic builds link neither beam instances nor beam.o
#include "beam.h"
#endif
#include "ldpc.h"
#include "tdl.h"
#include "turbo.h"

namespace {

using mimo::AlphaFit;
using mimo::fit_alpha;

using mimo::fail;

thread_local std::string g_err;  // behind mimo::set_error (below) and mimo_last_error()

constexpr double kSpeedOfLight = 299792458.0;  // scipy.constants.c

bool is_pow2(long v) { return v > 0 && (v & (v - 1)) == 0; }

// In-band sub-carrier k of S -> FFT bin of F (modulation.py:266-267).
int band_bin(int k, int S, int F) { return k < S / 2 ? F - S / 2 + k : k - S / 2 + 1; }

// An owned device (PINNED: pinned host) array that only grows; growing drops the contents.
// It makes no HIP call while it holds nothing, so an engine that never ran stays host-only.
template <typename T, bool PINNED = false>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { (void)release(); }
  hipError_t release() {
    T* old = p;
    p = nullptr;
    cap = 0;
    if (!old) return hipSuccess;
    if constexpr (PINNED) return hipHostFree(old);
    else return hipFree(old);
  }
  int ensure(size_t need) {
    if (need <= cap) return MIMO_OK;
    MIMO_HIP_TRY(release());
    if constexpr (PINNED)
      MIMO_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p), need * sizeof(T), hipHostMallocDefault));
    else MIMO_HIP_TRY(hipMalloc(&p, need * sizeof(T)));
    cap = need;
    return MIMO_OK;
  }
  int upload(const std::vector<T>& v) {  // a blocking copy; an empty table stays a null pointer
    if (v.empty()) return MIMO_OK;
    if (int rc = ensure(v.size())) return rc;
    MIMO_HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return MIMO_OK;
  }
};

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
  // MIMO_CH_TABLE with a channel bank (mimo_engine_set_channel_bank): the in-band columns of its
  // n_bank tables, [n_bank][A][S] in the engine's precision alone (a bank may fill 1 GiB), and
  // whether the device copy behind tab64 / tab32 is still to be replaced (at the next run)
  int n_bank = 0;
  std::vector<double2> bank64;
  std::vector<float2> bank32;
  bool tab_stale = false;
  // MIMO_CH_TDL: the profile (mimo_engine_set_tdl), its device tables (tdl.h TdlHost::blob) and
  // whether those are still to be uploaded.  The generator fills tab64 / tab32 launch by launch.
  // The profile is a power-delay profile (tdl) or, after mimo_engine_set_rays, a ray-cluster one
  // (rays, tdl_is_rays): whichever setter was called last.
  bool have_tdl = false;
  mimo::TdlHost tdl;
  bool tdl_is_rays = false;
  mimo::RaysHost rays;
  bool tdl_stale = false;
  Buf<double> tdl_blob;
  double last_chan_ms = 0.0;
  mimo_point pt{};
  bool have_point = false;
  // device state (created lazily on the first run: fork safety); whatever of it exists is released
  // with the engine, whether or not ensure_device came through
  bool ready = false;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev2 = nullptr;               // after the beamforming / decoder kernel of a launch
  hipEvent_t ev3 = nullptr;               // ahead of the TDL generator kernel of a launch (ev0 follows it)
  Buf<float2> tw[2];                      // fp32 stage twiddles for team_size(F), alt_team_size(F)
  Buf<double2> tw64;                      // fp64 stage twiddles for team_size64(F)
  Buf<double2> twave64;                   // wave-split FFT twiddles (wave_fft.h) where the instance uses it
  Buf<float2> twave32;
  Buf<double2> lut64;                     // fp64 Box-Muller tables (lut64_table)
  Buf<float2> tab32;                      // MIMO_CH_TABLE channel, fp32 / fp64 copies
  Buf<double2> tab64;
  Buf<float> ant_rel, f_rel;
  Buf<double> ant_rel64, f_rel64, f_over_c, tx_pos_dev;
  Buf<uint32_t> counts;
  Buf<unsigned long long> tot;            // [points][n_idx] totals of one run
  // row-mode calls (measure, spectrum, beam, envelope, soft: one mode per call, so one pair): the
  // per-trial rows of one launch and their per-slice partials.  Spectrum, beam, envelope and soft rows
  // hold at most MIMO_SPEC_BUFFER_BYTES / MIMO_BEAM_ROWS_BYTES / MIMO_ENV_BUFFER_BYTES /
  // MIMO_SOFT_BUFFER_BYTES (that bounds the trials of their launches).
  Buf<double> rows;                       // [launch blocks][row width]
  Buf<double> part;                       // [launch slices][row width]
  // beam calls: the beam instances' cells of one launch (at most the beam buffer's bytes: it bounds
  // the trials of a beam launch) and the probe geometry
  Buf<double> bcell;                      // [2][launch blocks][A][F] complex128
  Buf<double> bgeo;                       // dist [n_probes][A] | 1 / dist [n_probes][A] | f / c [F]
  double last_beam_ms = 0.0;
  // coded calls: the coded instances' channel values of one launch (at most MIMO_CODED_BUFFER_BYTES: it
  // bounds the trials of a coded launch) and the decoder's tables (ldpc.h LdpcHost::tables)
  Buf<int8_t> cchan;                      // [launch blocks][n_idx][S log2 M]
  Buf<int32_t> ctab;
  double last_decode_ms = 0.0;
  // turbo calls: the turbo instances' received vectors of one launch and the decoder's decisions; the
  // channel values (one pass's, or every pass's where the caller asks for them) are in cchan, the
  // decoder's tables in ctab.  Together at most MIMO_TURBO_BUFFER_BYTES (launch_trials).
  Buf<double2> tz;                        // [launch blocks][S]
  Buf<int8_t> thard;                      // [launch blocks][S log2 M]
  // per-launch tables in one device blob, filled by one copy from a pinned host buffer:
  // TrialParams<R>[segments] | uint32 block offsets [segments + 1] |
  // uint32 reduction-slice starts [slices + 1] (<= kSlice trials, one point each) | int32 point of slice [slices]
  Buf<char> blob;
  Buf<char, true> h_blob;
  double d0 = 1.0;
  double last_ms = 0.0;
  // fit_alpha results per IBO (bit pattern of 10^(IBO/10)): the long-double fit costs
  // ~0.3 ms, paid once per IBO instead of once per point and batch of a sweep
  std::unordered_map<uint64_t, AlphaFit> alpha_fits;
  std::string desc;

  // (the buffers free themselves after this; no HIP call for an engine that never ran)
  ~mimo_engine() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipEvent_t ev : {ev0, ev1, ev2, ev3})
      if (ev) (void)hipEventDestroy(ev);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

std::string describe(const mimo::InstanceKey& k) {
  char buf[160];
  snprintf(buf, sizeof buf, "F=%d T=%d slots=%d %s ch=%d csi=%d %s", k.F, k.T, k.nslot,
           k.aligned ? "aligned" : "generic", k.ch, (int)k.csi, k.f64 ? "f64" : "f32");
  return buf;
}

mimo::InstanceKey select_instance(const mimo_engine* e, bool csi) {
  mimo::InstanceKey k{};
  k.F = e->cfg.n_fft;
  k.f64 = e->cfg.precision != MIMO_PREC_F32;
  const int S = e->cfg.n_sub_carr;
  auto aligned_at = [&](int T) {
    const int P = k.F / T;
    return (S % (4 * T) == 0) && S < k.F && (S / T == 8 || S / T == 4) && (S / T) < P;
  };
  k.T = k.f64 ? mimo::team_size64(k.F) : mimo::team_size(k.F);  // one team size per fp64 instance
  if (!k.f64) {
    // Unaligned bands (S % 4T != 0) run the generic predicated path with P slots per
    // thread; the alternative team has half the points per thread, which measured 1.5x
    // faster there (60.7 vs 40.7 ms at S = 1000, F = 2048; profiles/r01/ab_generic.json).
    if (!aligned_at(k.T) && mimo::alt_team_size(k.F) != k.T) k.T = mimo::alt_team_size(k.F);
    if (const char* env = std::getenv("MIMO_TEAM")) {  // A/B override: MIMO_TEAM=<threads per trial>
      const int t = std::atoi(env);
      if (t == mimo::alt_team_size(k.F) || t == mimo::team_size(k.F)) k.T = t;
    }
  }
  const int P = k.F / k.T;
  k.aligned = aligned_at(k.T);
  k.nslot = k.aligned ? S / k.T : P;
  // (a TDL engine runs the table instances on the bank its generator fills)
  k.ch = e->cfg.channel_kind == MIMO_CH_TDL ? MIMO_CH_TABLE : e->cfg.channel_kind;
  k.csi = csi;
  return k;
}

// The mode arguments of a launch (trial_params.h ModeArgs), built here alone: the engine's buffer
// that the mode's instances fill -- the launch's rows; the beam instances its cells and the coded
// instances its channel values, from which the mode's second kernel forms the rows -- and the scale.
template <int MODE>
mimo::ModeArgs<MODE> mode_args(const mimo_engine* e, double scale) {
  if constexpr (MODE == MIMO_MODE_PLAIN) return {};
  else if constexpr (MODE == MIMO_MODE_BEAM) return {e->bcell.p};
  else if constexpr (MODE == MIMO_MODE_CODED) return {e->cchan.p, scale};
  else if constexpr (MODE == MIMO_MODE_TURBO) return {e->tz.p};
  else if constexpr (std::tuple_size_v<mimo::ModeArgs<MODE>> == 2) return {e->rows.p, scale};
  else return {e->rows.p};
}

// The launcher of the key's instance in the given mode (trial_launch.h launch_trial), on the engine's
// stream.  The only table over the FFT sizes; the combinations that are not built are not found.
template <typename R, int MODE>
hipError_t launch_sized(const mimo_engine* e, const mimo::InstanceKey& k, dim3 grid, const mimo::TrialParams<R>& p,
                        bool* found, hipFuncAttributes* attr, double scale) {
  *found = false;
#if defined(MIMO_ONLY_F) && defined(MIMO_ONLY_MEAS)  // A-B builds (Makefile target variant): plain and measure
  constexpr bool built = MODE == MIMO_MODE_PLAIN || (MODE == MIMO_MODE_MEAS && sizeof(R) == 8);
#elif defined(MIMO_ONLY_F)  // single-size diagnostic builds (Makefile target ablation): plain only
  constexpr bool built = MODE == MIMO_MODE_PLAIN;
#else
  constexpr bool built = MODE == MIMO_MODE_PLAIN || sizeof(R) == 8;
#endif
  if constexpr (built) {
#define MIMO_LAUNCH_F(FV) \
  case FV: return mimo::launch_trial<FV, R, MODE>(k, grid, e->stream, p, found, attr, mode_args<MODE>(e, scale));
    switch (k.F) {
#ifdef MIMO_ONLY_F
      MIMO_LAUNCH_F(MIMO_ONLY_F)
#else
      MIMO_LAUNCH_F(128)
      MIMO_LAUNCH_F(256)
      MIMO_LAUNCH_F(512)
      MIMO_LAUNCH_F(1024)
      MIMO_LAUNCH_F(2048)
      MIMO_LAUNCH_F(4096)
      MIMO_LAUNCH_F(8192)
#endif
      default: break;
    }
#undef MIMO_LAUNCH_F
  }
  return hipSuccess;
}

template <typename R>
hipError_t launch(int mode, const mimo_engine* e, const mimo::InstanceKey& k, dim3 grid, const mimo::TrialParams<R>& p,
                  bool* found, hipFuncAttributes* attr, double scale = 0.0) {
  switch (mode) {
#define MIMO_LAUNCH_MODE(M) \
  case M: return launch_sized<R, M>(e, k, grid, p, found, attr, scale);
    MIMO_LAUNCH_MODE(MIMO_MODE_MEAS)
    MIMO_LAUNCH_MODE(MIMO_MODE_SPEC)
    MIMO_LAUNCH_MODE(MIMO_MODE_BEAM)
    MIMO_LAUNCH_MODE(MIMO_MODE_ENV)
    MIMO_LAUNCH_MODE(MIMO_MODE_SOFT)
    MIMO_LAUNCH_MODE(MIMO_MODE_CODED)
    MIMO_LAUNCH_MODE(MIMO_MODE_TURBO)
#undef MIMO_LAUNCH_MODE
    default: return launch_sized<R, MIMO_MODE_PLAIN>(e, k, grid, p, found, attr, scale);
  }
}

// A beam call's probes, checked and turned into the beamforming kernel's tables by the caller
// (mimo_engine_beam_points): geo = dist [n_probes][A] | 1 / dist [n_probes][A] | f / c [F].
struct BeamCall {
  int n_probes;
  uint64_t buffer;  // bytes the cells of one launch may take: one trial's at least
  std::vector<double> geo;
};

// A coded call's code, checked and turned into the decoder's tables by the caller
// (mimo_engine_coded_points).
struct CodedCall {
  mimo::LdpcHost code;
  int n_cw = 0;                    // codewords of one trial and counter index
  size_t stream = 0;               // S log2 M: channel values of one trial and counter index
  int8_t* per_trial_chan = nullptr;  // [trials of the call][n_idx][stream], or null
};

// A turbo call: the coded call's code and stream, and the pass loop's own arguments
// (mimo_engine_turbo_points).
struct TurboCall {
  CodedCall cc;                    // cc.per_trial_chan: [trials of the call][n_passes][stream], or null
  int n_passes = 1;
  double* per_trial_z = nullptr;   // [trials of the call][S] complex128, or null
  // bytes of one trial in the buffers of a launch: z, the streams, the decisions
  uint64_t trial_bytes(int n_sub_carr) const {
    return 16ull * (uint64_t)n_sub_carr + (uint64_t)cc.stream * (uint64_t)(cc.per_trial_chan ? n_passes : 1) +
           (uint64_t)cc.stream;
  }
};

// What a row mode adds to a plain run, filled by the extern "C" entry point of the mode.  The mode's
// instances run and leave per-trial rows of row_width doubles, which are reduced per slice on the
// device (reduce_spec; measure: reduce_meas) and per point, in slice order, on the host; a launch
// holds no more trials than the mode's buffer fits (launch_trials).  Particular to a mode:
//  envelope, soft, coded: the instances take a scale;
//  beam, coded: the instances fill the launch's cells / channel values instead, and a second kernel
//   (beam.hip, ldpc.hip) forms the rows from them, from the call's tables (launch_second);
//  turbo: the instances leave the received vectors, and launch_second runs the pass loop on them
//   (turbo.hip's step kernel and the decoder, n_passes times), which forms the rows.
struct RowMode {
  int mode = MIMO_MODE_PLAIN;
  double* out = nullptr;                // [points][width], added into
  double* per_trial_out = nullptr;      // [trials of the call][width], or null
  double scale = 0.0;                   // envelope, soft, coded
  const BeamCall* beam = nullptr;       // beam only
  const CodedCall* coded = nullptr;     // coded only
  const TurboCall* turbo = nullptr;     // turbo only
  int width = 0;                        // row_width, once run_points has checked the iteration list
  bool rows() const { return mode != MIMO_MODE_PLAIN; }
  bool second() const { return beam || coded || turbo; }
};

// Doubles of one trial's row in a mode, and of one point's in the mode's output: what the
// mimo_*_width functions return and the callers allocate.
int row_width(int mode, int n_fft, int n_idx, int n_probes) {
  switch (mode) {
    case MIMO_MODE_MEAS: return MIMO_MEAS_FIXED + n_idx;
    case MIMO_MODE_SPEC: return n_fft + MIMO_SPEC_FIXED;
    case MIMO_MODE_BEAM: return n_probes * MIMO_BEAM_FIXED;
    case MIMO_MODE_ENV: return 2 * MIMO_ENV_BINS + MIMO_ENV_FIXED;
    case MIMO_MODE_SOFT: return MIMO_SOFT_BINS * n_idx;
    case MIMO_MODE_CODED: return MIMO_CODED_FIXED * n_idx;
    default: return 0;
  }
}

// A limit that an environment variable lowers, for measurements and tests of the splitting: the
// variable's value in units, where that is in [1, limit).
uint64_t env_lowered(const char* name, uint64_t limit, uint64_t unit = 1) {
  if (const char* env = std::getenv(name)) {
    const uint64_t v = std::strtoull(env, nullptr, 10) / unit;
    if (v >= 1 && v < limit) return v;
  }
  return limit;
}

// The cells of one trial of a beam launch: Y and X of every antenna and bin, complex128.
uint64_t beam_trial_bytes(const mimo_config& c) { return 2ull * (uint64_t)c.n_ant * (uint64_t)c.n_fft * 16ull; }

// The trials one launch may hold (0: not one fits): what the mode's buffer fits -- the rows'
// (measure: no bound), for beam the cells' too, for coded the channel values' instead -- and on a
// TDL engine the bank entries that fit MIMO_BANK_BUFFER_BYTES.
uint64_t launch_trials(const mimo_config& c, const RowMode& rm, int n_idx) {
  const uint64_t row = sizeof(double) * (uint64_t)rm.width;
  uint64_t n = UINT64_MAX;
  switch (rm.mode) {
    case MIMO_MODE_SPEC: n = MIMO_SPEC_BUFFER_BYTES / row; break;
    case MIMO_MODE_BEAM: n = std::min<uint64_t>(rm.beam->buffer / beam_trial_bytes(c), MIMO_BEAM_ROWS_BYTES / row); break;
    case MIMO_MODE_ENV: n = MIMO_ENV_BUFFER_BYTES / row; break;
    case MIMO_MODE_SOFT: n = MIMO_SOFT_BUFFER_BYTES / row; break;
    case MIMO_MODE_CODED: n = MIMO_CODED_BUFFER_BYTES / (rm.coded->stream * (size_t)n_idx); break;
    case MIMO_MODE_TURBO:
      n = env_lowered("MIMO_TURBO_BUFFER_BYTES", MIMO_TURBO_BUFFER_BYTES) / rm.turbo->trial_bytes(c.n_sub_carr);
      break;
    default: break;
  }
  if (c.channel_kind == MIMO_CH_TDL) {
    const uint64_t entry = (uint64_t)c.n_ant * (uint64_t)c.n_sub_carr *
                           (c.precision == MIMO_PREC_F32 ? sizeof(float2) : sizeof(double2));
    n = std::min(n, env_lowered("MIMO_BANK_BUFFER_BYTES", (uint64_t)mimo_bank_capacity(c.n_ant, c.n_sub_carr, c.precision),
                                entry));
  }
  return n;
}

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
  if (c->channel_kind < MIMO_CH_RAYLEIGH || c->channel_kind > MIMO_CH_TDL)
    return fail(MIMO_EINVAL, "unknown channel_kind");
  if (c->channel_kind == MIMO_CH_TDL && !c->reroll_chan)
    return fail(MIMO_EINVAL, "reroll_chan = 0 is not a MIMO_CH_TDL engine: a fixed channel is a table (MIMO_CH_TABLE)");
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
// coordinate too).  Table and TDL channels read no position.
int validate_distances(const mimo_engine* e) {
  const mimo_config& c = e->cfg;
  if (c.channel_kind == MIMO_CH_TABLE || c.channel_kind == MIMO_CH_TDL) return MIMO_OK;
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

// (A call after one that failed half-way keeps what that one created.)
int ensure_device(mimo_engine* e) {
  if (e->ready) return MIMO_OK;
  if (e->cfg.device >= 0) MIMO_HIP_TRY(hipSetDevice(e->cfg.device));
  MIMO_HIP_TRY(hipGetDevice(&e->device));
  if (!e->stream) MIMO_HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  for (hipEvent_t* ev : {&e->ev0, &e->ev1, &e->ev2, &e->ev3})
    if (!*ev) MIMO_HIP_TRY(hipEventCreate(ev));
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
    const double f = e->freqs[band_bin(k, S, F)];
    // table and TDL channels carry their full attenuation: nothing is factored out of the loops
    const bool whole = e->cfg.channel_kind == MIMO_CH_TABLE || e->cfg.channel_kind == MIMO_CH_TDL;
    f_rel64[k] = whole ? 1.0 : fc / f;
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

  std::vector<float2> tab32;
  std::vector<double2> tab64;
  for (size_t i = 0; i < e->chan_inband.size() / 2; ++i) {
    tab64.push_back(make_double2(e->chan_inband[2 * i], e->chan_inband[2 * i + 1]));
    tab32.push_back(make_float2((float)e->chan_inband[2 * i], (float)e->chan_inband[2 * i + 1]));
  }
  int rc = MIMO_OK;  // the first upload that fails ends them
  auto up = [&rc](auto& buf, const auto& v) {
    if (rc == MIMO_OK) rc = buf.upload(v);
  };
  up(e->tw[0], tws[0]);
  up(e->tw[1], tws[1]);
  up(e->tab32, tab32);
  up(e->tab64, tab64);
  up(e->lut64, mimo::lut64_table());
  up(e->tw64, tw64);
  up(e->twave64, twave64);
  up(e->twave32, twave32);
  up(e->f_rel64, f_rel64);
  up(e->ant_rel64, ant_rel64);
  up(e->f_rel, f_rel);
  up(e->f_over_c, f_over_c);
  up(e->ant_rel, ant_rel);
  up(e->tx_pos_dev, e->tx_pos);
  if (rc) return rc;
  e->ready = true;
  return MIMO_OK;
}

// What the setters changed since the last run, uploaded before this one (the setters make no HIP
// call): the channel bank of a table engine in the engine's precision -- or, back at n_bank = 0,
// the create-time table -- and a TDL engine's profile tables.
int refresh_channel_tables(mimo_engine* e) {
  if (!e->tab_stale && !e->tdl_stale) return MIMO_OK;
  MIMO_HIP_TRY(hipStreamSynchronize(e->stream));  // no launch of a call that failed half-way still reads them
  if (e->tab_stale) {
    if (e->n_bank > 0) {
      if (int rc = e->cfg.precision == MIMO_PREC_F32 ? e->tab32.upload(e->bank32) : e->tab64.upload(e->bank64)) return rc;
    } else {
      std::vector<float2> tab32;
      std::vector<double2> tab64;
      for (size_t i = 0; i < e->chan_inband.size() / 2; ++i) {
        tab64.push_back(make_double2(e->chan_inband[2 * i], e->chan_inband[2 * i + 1]));
        tab32.push_back(make_float2((float)e->chan_inband[2 * i], (float)e->chan_inband[2 * i + 1]));
      }
      if (int rc = e->tab32.upload(tab32)) return rc;
      if (int rc = e->tab64.upload(tab64)) return rc;
    }
    e->tab_stale = false;
  }
  if (e->tdl_stale) {
    if (int rc = e->tdl_blob.upload(e->tdl_is_rays ? e->rays.blob() : e->tdl.blob())) return rc;
    e->tdl_stale = false;
  }
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
        const int bin = band_bin(k, S, F);
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

// The iteration list of a call: the counter columns the kernel records.
struct Iters {
  uint32_t rec_mask = 0;
  int max_iter = -1;
};

int validate_iters(const int32_t* iters, int32_t n_iters, Iters* it) {
  if (n_iters < 1 || !iters) return fail(MIMO_EINVAL, "at least one iteration index is required");
  for (int i = 0; i < n_iters; ++i) {
    if (iters[i] < 0 || iters[i] > 31) return fail(MIMO_EINVAL, "iterations must be in [0, 31]");
    if (i && iters[i] <= iters[i - 1]) return fail(MIMO_EINVAL, "iterations must be sorted and unique");
    it->rec_mask |= 1u << iters[i];
    it->max_iter = std::max(it->max_iter, (int)iters[i]);
  }
  return MIMO_OK;
}

// Every point of a call (n_points >= 1), and what they must agree on: *csi = CSI error on.
int validate_points(const mimo_engine* e, int n_points, const mimo_point* pts, const uint64_t* first_trial,
                    const uint64_t* n_trials, bool* csi) {
  *csi = pts[0].csi_eps >= 0;
  for (int i = 0; i < n_points; ++i) {
    if (int rc = validate_point(e, &pts[i])) return rc;
    if ((pts[i].csi_eps >= 0) != *csi) return fail(MIMO_EINVAL, "all points of one run must agree on CSI error on/off");
    if (n_trials[i] + first_trial[i] > (1ull << 32) || first_trial[i] >= (1ull << 32))
      return fail(MIMO_EINVAL, "trial index must fit 32 bits");
  }
  return MIMO_OK;
}

// The CSI instances add n_ant reals of dynamic LDS (the per-antenna power table) to their
// static LDS: check the sum against the CU's LDS before launching (F 8192 holds
// ~157 KiB statically, so A = 512 (4 KiB) is the edge).  mode: the instance the call launches --
// the envelope and soft instances hold their histogram on top of the plain instance's static LDS
// (the measure, spectrum, beam, coded and turbo instances hold what the plain one holds).
int check_csi_lds(const mimo_engine* e, const mimo::InstanceKey& key, int mode) {
  hipFuncAttributes fa{};
  bool found = false;
  const hipError_t qe =
      key.f64 ? launch(mode, e, key, dim3(0), mimo::TrialParams<double>{}, &found, &fa)
              : launch(MIMO_MODE_PLAIN, e, key, dim3(0), mimo::TrialParams<float>{}, &found, &fa);
  int lds_max = 0;
  if (!found || qe != hipSuccess ||
      hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, e->device) != hipSuccess ||
      lds_max <= 0)
    return MIMO_OK;
  const int A = e->cfg.n_ant;
  const size_t need = fa.sharedSizeBytes + (size_t)A * (key.f64 ? sizeof(double) : sizeof(float));
  if (need > (size_t)lds_max)
    return fail(MIMO_EINVAL, "CSI error at n_ant = " + std::to_string(A) + " needs " + std::to_string(need) +
                                 " B of LDS per team (static " + std::to_string(fa.sharedSizeBytes) +
                                 " + the per-antenna table), the device has " + std::to_string(lds_max));
  return MIMO_OK;
}

// The launches of a call: every point's trials become a contiguous range of blocks of one launch,
// split across launches only beyond the chunk; a launch is a list of segments.  Per segment the
// reductions run over slices of at most kSlice trials.
struct Seg {
  int point;
  uint64_t first, n;
};
struct Plan {
  std::vector<std::vector<Seg>> launches{1};
  size_t max_seg = 0, max_blocks = 0, max_slices = 0;  // of one launch
  size_t tot_slices = 0;                               // of all
};

// max_trials: what the mode's buffers allow in one launch.  Without it a launch holds 2^20 trials
// (MIMO_MAX_LAUNCH_TRIALS lowers it, for tests of the splitting).
Plan plan_launches(int n_points, const uint64_t* first_trial, const uint64_t* n_trials, uint64_t max_trials) {
  const uint64_t chunk = std::min(env_lowered("MIMO_MAX_LAUNCH_TRIALS", 1ull << 20), max_trials);
  Plan plan;
  uint64_t fill = 0;
  for (int i = 0; i < n_points; ++i) {
    uint64_t done = 0;
    while (done < n_trials[i]) {
      if (fill == chunk) {
        plan.launches.emplace_back();
        fill = 0;
      }
      const uint64_t n = std::min(n_trials[i] - done, chunk - fill);
      plan.launches.back().push_back(Seg{i, first_trial[i] + done, n});
      done += n;
      fill += n;
    }
  }
  for (auto& l : plan.launches) {
    size_t nb = 0, nsl = 0;
    for (auto& sg : l) {
      nb += (size_t)sg.n;
      nsl += (size_t)((sg.n + kSlice - 1) / kSlice);
    }
    plan.max_seg = std::max(plan.max_seg, l.size());
    plan.max_blocks = std::max(plan.max_blocks, nb);
    plan.max_slices = std::max(plan.max_slices, nsl);
    plan.tot_slices += nsl;
  }
  return plan;
}

// The kernel parameters every point of the call shares (fill_point adds a point's own).
template <typename R>
mimo::TrialParams<R> base_params(const mimo_engine* e, const mimo::InstanceKey& key, const Iters& it,
                                 int32_t incl_clean, int n_idx) {
  const mimo_config& c = e->cfg;
  mimo::TrialParams<R> base{};
  if constexpr (sizeof(R) == 8) {
    base.tw = e->tw64.p;
    base.tw_wave = e->twave64.p;
    base.ant_rel = e->ant_rel64.p;
    base.f_rel = e->f_rel64.p;
    base.chan_tab = e->tab64.p;
  } else {
    base.tw = e->tw[key.T == mimo::team_size(c.n_fft) ? 0 : 1].p;
    base.tw_wave = key.T == mimo::team_size(c.n_fft) ? e->twave32.p : nullptr;
    base.ant_rel = e->ant_rel.p;
    base.f_rel = e->f_rel.p;
    base.chan_tab = e->tab32.p;
  }
  base.f_over_c = e->f_over_c.p;
  base.tx_pos = e->tx_pos_dev.p;
  base.lut = e->lut64.p;
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
  base.max_iter = it.max_iter;
  base.rec_mask = it.rec_mask;
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
  base.counts = e->counts.p;
  base.chan_period = (uint32_t)std::max(0, c.chan_replay_period);
  // table instances: the entries of the bank behind chan_tab (trial_kernel.h ch_trial); a TDL
  // engine's 0 gives every block of a launch the entry its generator filled for it
  if (c.channel_kind == MIMO_CH_TABLE) base.chan_period = (uint32_t)std::max(1, e->n_bank);
  return base;
}

// Byte offsets of the per-launch tables in the blob (mimo_engine::blob), each 16-byte aligned.
// (tdl: the TDL generator's segment table, TdlSeg [segments], behind the others on a TDL engine)
struct BlobLayout {
  size_t start, slice, point_of, tdl, bytes;
};
BlobLayout blob_layout(const Plan& plan, size_t params_bytes, bool tdl) {
  auto up16 = [](size_t b) { return (b + 15) & ~size_t(15); };
  BlobLayout o{};
  o.start = up16(plan.max_seg * params_bytes);
  o.slice = o.start + up16((plan.max_seg + 1) * sizeof(uint32_t));
  o.point_of = o.slice + up16((plan.max_slices + 1) * sizeof(uint32_t));
  o.tdl = o.point_of + up16(plan.max_slices * sizeof(int32_t));
  o.bytes = o.tdl + (tdl ? up16(plan.max_seg * sizeof(mimo::TdlSeg)) : 0);
  return o;
}

// What the launches of a call leave for its totals.
struct Progress {
  uint64_t trials_done = 0;
  // row modes: the slice partials of every launch, in launch and slice order, and their points
  std::vector<double> part;
  std::vector<int> part_point;
  double ms = 0.0, second_ms = 0.0, chan_ms = 0.0;  // trial kernel, second kernel (RowMode), TDL generator
};

// The tables of one launch, written into the host blob: the segments' parameters and block
// offsets, the reduction slices' starts and points.
struct LaunchTables {
  size_t nseg = 0, nsl = 0;  // segments, slices
  uint32_t nb = 0;           // blocks (trials)
  const int32_t* point_of = nullptr;  // [nsl], host
};
template <typename R>
LaunchTables fill_launch_tables(char* h_blob, const BlobLayout& o, const std::vector<mimo::TrialParams<R>>& ptab,
                                const std::vector<Seg>& segs) {
  using TP = mimo::TrialParams<R>;
  TP* seg_tab = reinterpret_cast<TP*>(h_blob);
  uint32_t* start = reinterpret_cast<uint32_t*>(h_blob + o.start);
  uint32_t* slice_first = reinterpret_cast<uint32_t*>(h_blob + o.slice);
  int32_t* point_of = reinterpret_cast<int32_t*>(h_blob + o.point_of);
  LaunchTables t;
  t.point_of = point_of;
  start[0] = 0u;
  slice_first[0] = 0u;
  for (auto& sg : segs) {
    TP q = ptab[sg.point];
    q.first_trial = sg.first;
    seg_tab[t.nseg] = q;
    const uint32_t b0 = start[t.nseg];
    start[++t.nseg] = b0 + (uint32_t)sg.n;
    for (uint32_t s = 0; s < (uint32_t)sg.n; s += kSlice) {
      slice_first[++t.nsl] = b0 + std::min<uint32_t>((uint32_t)sg.n, s + kSlice);
      point_of[t.nsl - 1] = sg.point;
    }
  }
  t.nb = start[t.nseg];
  return t;
}

// The second kernel of a beam or coded call (RowMode).  Before the first launch: its buffers for
// the largest launch of the plan, and the call's tables uploaded.
int prepare_second(mimo_engine* e, const RowMode& rm, const Plan& plan, int n_idx) {
  const mimo_config& c = e->cfg;
  if (rm.beam) {
    const size_t cells = 2 * plan.max_blocks * (size_t)c.n_ant * (size_t)c.n_fft * 2;  // doubles
    if (int rc = e->bcell.ensure(std::max<size_t>(2, cells))) return rc;
    if (int rc = e->bgeo.ensure(rm.beam->geo.size())) return rc;
    MIMO_HIP_TRY(hipMemcpyAsync(e->bgeo.p, rm.beam->geo.data(), sizeof(double) * rm.beam->geo.size(),
                                hipMemcpyHostToDevice, e->stream));
  } else {
    const CodedCall& cc = rm.turbo ? rm.turbo->cc : *rm.coded;
    const std::vector<int32_t>& tab = cc.code.tables;
    // streams of one trial: one per counter index; turbo: one, or one per pass where they are copied back
    const size_t per_trial = rm.turbo ? (cc.per_trial_chan ? (size_t)rm.turbo->n_passes : 1) : (size_t)n_idx;
    if (int rc = e->cchan.ensure(std::max<size_t>(1, plan.max_blocks * per_trial * cc.stream))) return rc;
    if (int rc = e->ctab.ensure(tab.size())) return rc;
    MIMO_HIP_TRY(hipMemcpyAsync(e->ctab.p, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, e->stream));
    if (rm.turbo) {
      if (int rc = e->tz.ensure(std::max<size_t>(1, plan.max_blocks * (size_t)c.n_sub_carr))) return rc;
      if (int rc = e->thard.ensure(std::max<size_t>(1, plan.max_blocks * cc.stream))) return rc;
    }
  }
  return MIMO_OK;
}

// The pass loop of a turbo launch, behind the trial kernel that left the nb received vectors in tz:
// step<first>, decode, step, decode ... (turbo.h, ldpc.h), pass q's cells to columns 4 q ... 4 q + 3
// of the trials' rows.  kp: the parameters of that trial launch (its point table is still in the blob).
hipError_t launch_turbo_passes(mimo_engine* e, const mimo::InstanceKey& key, const TurboCall& tc, double scale,
                               uint32_t nb, const mimo::TrialParams<double>& kp, bool* found) {
  const CodedCall& cc = tc.cc;
  const size_t pass_bytes = cc.per_trial_chan ? (size_t)nb * cc.stream : 0;  // between two passes' streams in cchan
  for (int q = 0; q < tc.n_passes; ++q) {
    mimo::StepArgs a{};
    a.z = e->tz.p;
    a.hard = e->thard.p;
    a.chan_in = e->cchan.p + (size_t)std::max(0, q - 1) * pass_bytes;
    a.n_dec = cc.n_cw * cc.code.n_bits();
    a.chan_out = e->cchan.p + (size_t)q * pass_bytes;
    a.scale = scale;
    if (hipError_t se = mimo::launch_turbo_step(key, q == 0, nb, e->stream, kp, a, found); se != hipSuccess || !*found)
      return se;
    const bool last = q + 1 == tc.n_passes;
    if (hipError_t de = mimo::launch_ldpc(e->stream, cc.code, e->ctab.p, a.chan_out, (int64_t)nb, (int64_t)cc.stream,
                                          cc.n_cw, cc.n_cw, e->rows.p + (size_t)q * MIMO_CODED_FIXED, nullptr,
                                          last ? nullptr : e->thard.p, (int64_t)tc.n_passes * MIMO_CODED_FIXED);
        de != hipSuccess)
      return de;
  }
  return hipSuccess;
}

// In a launch, behind the trial kernel: the rows of its nb trials from what the instances left, ev2
// behind it (run_launch times ev1 to ev2), and a coded call's channel values copied back where asked.
int launch_second(mimo_engine* e, const RowMode& rm, uint32_t nb, int n_idx, uint64_t trials_done,
                  const mimo::InstanceKey& key, const mimo::TrialParams<double>* kp) {
  hipError_t se = hipSuccess;
  if (rm.turbo) {
    bool found = false;
    if (!kp) return fail(MIMO_ENOKERNEL, "the turbo pass loop is float64 only");
    se = launch_turbo_passes(e, key, *rm.turbo, rm.scale, nb, *kp, &found);
    if (se == hipSuccess && !found) return fail(MIMO_ENOKERNEL, "no step kernel instance for " + e->desc);
  } else if (const CodedCall* cc = rm.coded) {
    se = mimo::launch_ldpc(e->stream, cc->code, e->ctab.p, e->cchan.p, (int64_t)nb * n_idx, (int64_t)cc->stream, cc->n_cw,
                           cc->n_cw, e->rows.p, nullptr);
  } else {
#ifndef MIMO_ONLY_F  // (the single-size diagnostic builds find no beam instance to launch before this)
    const mimo_config& c = e->cfg;
    const size_t na = (size_t)rm.beam->n_probes * (size_t)c.n_ant;
    se = mimo::launch_beam(e->stream, e->bcell.p, e->bgeo.p, e->bgeo.p + na, e->bgeo.p + 2 * na, (int)nb, c.n_ant, c.n_fft,
                           c.n_sub_carr, rm.beam->n_probes, e->rows.p);
#endif
  }
  if (se != hipSuccess)
    return fail(MIMO_EHIP, std::string(rm.turbo ? "turbo pass loop" : rm.coded ? "decoder" : "beamforming") +
                               " kernel launch: " + hipGetErrorString(se));
  MIMO_HIP_TRY(hipEventRecord(e->ev2, e->stream));
  if (rm.turbo) {
    const CodedCall& cc = rm.turbo->cc;
    const size_t np = (size_t)rm.turbo->n_passes;
    if (cc.per_trial_chan)  // [trial][pass][stream] from the device's [pass][trial][stream]
      for (size_t q = 0; q < np; ++q)
        MIMO_HIP_TRY(hipMemcpy2DAsync(cc.per_trial_chan + (trials_done * np + q) * cc.stream, np * cc.stream,
                                      e->cchan.p + q * (size_t)nb * cc.stream, cc.stream, cc.stream, nb,
                                      hipMemcpyDeviceToHost, e->stream));
    if (rm.turbo->per_trial_z) {
      const size_t row = 2 * (size_t)e->cfg.n_sub_carr;  // doubles
      MIMO_HIP_TRY(hipMemcpyAsync(rm.turbo->per_trial_z + trials_done * row, e->tz.p, (size_t)nb * row * sizeof(double),
                                  hipMemcpyDeviceToHost, e->stream));
    }
  }
  if (rm.coded && rm.coded->per_trial_chan) {
    const size_t per_trial = (size_t)n_idx * rm.coded->stream;
    MIMO_HIP_TRY(hipMemcpyAsync(rm.coded->per_trial_chan + trials_done * per_trial, e->cchan.p, (size_t)nb * per_trial,
                                hipMemcpyDeviceToHost, e->stream));
  }
  return MIMO_OK;
}

// One launch: its tables into the blob, the trial kernel of the mode, the mode's second kernel, the
// count and row reductions and the copies back; waits for the launch and times it.
template <typename R>
int run_launch(mimo_engine* e, const mimo::InstanceKey& key, const mimo::TrialParams<R>& base,
               const std::vector<mimo::TrialParams<R>>& ptab, const BlobLayout& o, const std::vector<Seg>& segs,
               const RowMode& rm, uint32_t* per_trial, Progress* pg) {
  using TP = mimo::TrialParams<R>;
  const int n_idx = base.n_idx;
  const LaunchTables t = fill_launch_tables(e->h_blob.p, o, ptab, segs);
  const size_t nsl = t.nsl;
  const uint32_t nb = t.nb;
  if (nb == 0) return MIMO_OK;  // every point of the call has n_trials == 0: nothing to launch
  const uint32_t* d_slice_first = reinterpret_cast<const uint32_t*>(e->blob.p + o.slice);
  TP kp = base;
  kp.points = reinterpret_cast<const TP*>(e->blob.p);
  kp.point_start = reinterpret_cast<const uint32_t*>(e->blob.p + o.start);
  kp.n_points = (int)t.nseg;
  kp.seed = ptab[segs[0].point].seed;  // unused by the kernel (read from the table)
  const bool tdl = e->cfg.channel_kind == MIMO_CH_TDL;
  if (tdl) {  // the generator's segments: the key and the first trial of every block range
    mimo::TdlSeg* ts = reinterpret_cast<mimo::TdlSeg*>(e->h_blob.p + o.tdl);
    for (size_t i = 0; i < t.nseg; ++i) ts[i] = mimo::TdlSeg{ptab[segs[i].point].seed, segs[i].first};
  }
  // the whole blob (unused tails included: one contiguous DMA)
  const size_t blob_bytes = tdl ? o.tdl + t.nseg * sizeof(mimo::TdlSeg) : o.point_of + nsl * sizeof(int32_t);
  MIMO_HIP_TRY(hipMemcpyAsync(e->blob.p, e->h_blob.p, blob_bytes, hipMemcpyHostToDevice, e->stream));
  if (tdl) {
    // the bank entries of this launch's blocks, in device memory (tdl.hip), ahead of the trial kernel
    // on the same stream and timed on an event of its own
    MIMO_HIP_TRY(hipEventRecord(e->ev3, e->stream));
    const mimo::TdlSeg* gsegs = reinterpret_cast<const mimo::TdlSeg*>(e->blob.p + o.tdl);
    double2* g64 = sizeof(R) == 8 ? e->tab64.p : nullptr;
    float2* g32 = sizeof(R) == 8 ? nullptr : e->tab32.p;
    const hipError_t ge =
        e->tdl_is_rays ? mimo::launch_rays(e->stream, e->rays, e->tdl_blob.p, gsegs, kp.point_start, (int)t.nseg, nb,
                                           e->cfg.n_sub_carr, g64, g32, nullptr, nullptr)
                       : mimo::launch_tdl(e->stream, e->tdl, e->tdl_blob.p, gsegs, kp.point_start, (int)t.nseg, nb,
                                          e->cfg.n_sub_carr, g64, g32, nullptr);
    if (ge != hipSuccess) return fail(MIMO_EHIP, std::string("TDL generator kernel launch: ") + hipGetErrorString(ge));
  }
  MIMO_HIP_TRY(hipEventRecord(e->ev0, e->stream));
  bool found = false;
  const hipError_t le = launch(rm.mode, e, key, dim3(nb), kp, &found, nullptr, rm.scale);
  if (!found) return fail(MIMO_ENOKERNEL, "no kernel instance for " + e->desc);
  if (le != hipSuccess) return fail(MIMO_EHIP, std::string("trial kernel launch: ") + hipGetErrorString(le));
  MIMO_HIP_TRY(hipEventRecord(e->ev1, e->stream));
  if (rm.second()) {
    const mimo::TrialParams<double>* kp64 = nullptr;
    if constexpr (sizeof(R) == 8) kp64 = &kp;
    if (int rc = launch_second(e, rm, nb, n_idx, pg->trials_done, key, kp64)) return rc;
  }
  hipLaunchKernelGGL(reduce_counts, dim3((unsigned)nsl, n_idx), dim3(256), 0, e->stream, e->counts.p, d_slice_first,
                     reinterpret_cast<const int32_t*>(e->blob.p + o.point_of), n_idx, e->tot.p);
  MIMO_HIP_TRY(hipGetLastError());
  if (per_trial)
    MIMO_HIP_TRY(hipMemcpyAsync(per_trial + pg->trials_done * n_idx, e->counts.p, (size_t)nb * n_idx * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, e->stream));
  if (rm.rows()) {
    const int w = rm.width;
    if (rm.mode == MIMO_MODE_MEAS)
      hipLaunchKernelGGL(reduce_meas, dim3((unsigned)nsl, w), dim3(kReduceMeasThreads), 0, e->stream, e->rows.p,
                         d_slice_first, w, e->part.p);
    else
      hipLaunchKernelGGL(reduce_spec, dim3((unsigned)nsl, (unsigned)((w + kReduceSpecThreads - 1) / kReduceSpecThreads)),
                         dim3(kReduceSpecThreads), 0, e->stream, e->rows.p, d_slice_first, w, e->part.p);
    MIMO_HIP_TRY(hipGetLastError());
    MIMO_HIP_TRY(hipMemcpyAsync(pg->part.data() + pg->part_point.size() * w, e->part.p, nsl * w * sizeof(double),
                                hipMemcpyDeviceToHost, e->stream));
    pg->part_point.insert(pg->part_point.end(), t.point_of, t.point_of + nsl);
    if (rm.per_trial_out)
      MIMO_HIP_TRY(hipMemcpyAsync(rm.per_trial_out + pg->trials_done * w, e->rows.p, (size_t)nb * w * sizeof(double),
                                  hipMemcpyDeviceToHost, e->stream));
  }
  pg->trials_done += nb;
  // the host tables of the next launch are rewritten: wait for this one's copies
  MIMO_HIP_TRY(hipEventSynchronize(e->ev1));
  float ms = 0.f;
  MIMO_HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  pg->ms += ms;
  if (tdl) {
    MIMO_HIP_TRY(hipEventElapsedTime(&ms, e->ev3, e->ev0));
    pg->chan_ms += ms;
  }
  if (rm.second()) {
    MIMO_HIP_TRY(hipEventSynchronize(e->ev2));
    MIMO_HIP_TRY(hipEventElapsedTime(&ms, e->ev1, e->ev2));
    pg->second_ms += ms;
  }
  return MIMO_OK;
}

// Every launch of the plan in the engine's arithmetic type R.
template <typename R>
int run_launches(mimo_engine* e, const mimo::InstanceKey& key, const mimo::TrialParams<R>& base, const Plan& plan,
                 int n_points, const mimo_point* pts, const uint64_t* seeds, const RowMode& rm, uint32_t* per_trial,
                 Progress* pg) {
  // per-point parameter table (host), built once
  std::vector<mimo::TrialParams<R>> ptab(n_points, base);
  for (int i = 0; i < n_points; ++i) fill_point(e, pts[i], seeds[i], 0, ptab[i]);
  const BlobLayout o = blob_layout(plan, sizeof(mimo::TrialParams<R>), e->cfg.channel_kind == MIMO_CH_TDL);
  if (int rc = e->blob.ensure(o.bytes)) return rc;
  if (int rc = e->h_blob.ensure(o.bytes)) return rc;
  for (auto& segs : plan.launches)
    if (int rc = run_launch(e, key, base, ptab, o, segs, rm, per_trial, pg)) return rc;
  return MIMO_OK;
}

// Runs n_points grid points of one system in as few launches as possible (plan_launches), and a
// segmented reduction sums each point's counts; rm: the rows a mode adds (RowMode; none: plain).
// The row's width and the trials of a launch come from the iteration list once it is checked.
int run_points(mimo_engine* e, int n_points, const mimo_point* pts, const uint64_t* seeds,
               const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters, int32_t n_iters,
               int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out, uint32_t* per_trial, RowMode rm) {
  if (n_points < 0) return fail(MIMO_EINVAL, "n_points must be >= 0");
  Iters it;
  if (int rc = validate_iters(iters, n_iters, &it)) return rc;
  if (!err_out || !bits_out) return fail(MIMO_EINVAL, "null counters");
  if (n_points == 0) return MIMO_OK;
  if (!pts || !seeds || !first_trial || !n_trials) return fail(MIMO_EINVAL, "null point arrays");
  const int n_idx = n_iters + (incl_clean ? 1 : 0);
  const mimo_config& c = e->cfg;
  rm.width = rm.turbo ? MIMO_CODED_FIXED * rm.turbo->n_passes
                      : row_width(rm.mode, c.n_fft, n_idx, rm.beam ? rm.beam->n_probes : 0);
  bool csi = false;
  if (int rc = validate_points(e, n_points, pts, first_trial, n_trials, &csi)) return rc;
  if (int rc = validate_distances(e)) return rc;
  const bool tdl = c.channel_kind == MIMO_CH_TDL;
  // one shared erroneous estimate per table is the table engine's rule; per-entry estimates are not built
  if (csi && e->n_bank > 1)
    return fail(MIMO_EINVAL, "csi_eps >= 0 is not supported with a channel bank of n_bank > 1 (one estimate per table)");
  if (csi && tdl) return fail(MIMO_EINVAL, "csi_eps >= 0 is not supported on a MIMO_CH_TDL engine");
  if (tdl && !e->have_tdl)
    return fail(MIMO_EINVAL, "a MIMO_CH_TDL engine needs a profile before it runs: neither mimo_engine_set_tdl nor "
                             "mimo_engine_set_rays was called");
  const mimo::InstanceKey key = select_instance(e, csi);
  if (int rc = ensure_device(e)) return rc;
  if (int rc = refresh_channel_tables(e)) return rc;
  if (csi)
    if (int rc = check_csi_lds(e, key, rm.mode)) return rc;
  if (!c.reroll_chan && (c.channel_kind == MIMO_CH_LOS || c.channel_kind == MIMO_CH_TWOPATH)) {
    // fixed RX: jitter span 0 around (x0, x0); only consistent when rx_y == rx_x
    // (table channels never use the RX position)
    if (c.rx_pos[1] != c.rx_pos[0]) return fail(MIMO_EINVAL, "reroll_chan=0 requires rx_pos[1] == rx_pos[0]");
  }
  e->desc = describe(key);

  const uint64_t max_trials = launch_trials(c, rm, n_idx);
  if (max_trials < 1)
    return fail(MIMO_EINVAL, rm.turbo ? "one trial's turbo buffers do not fit MIMO_TURBO_BUFFER_BYTES"
                                      : "n_ant, n_sub_carr: one trial's channel does not fit the bank buffer");
  const Plan plan = plan_launches(n_points, first_trial, n_trials, max_trials);
  if (tdl) {
    const size_t cells = std::max<size_t>(1, plan.max_blocks * (size_t)c.n_ant * (size_t)c.n_sub_carr);
    if (int rc = key.f64 ? e->tab64.ensure(cells) : e->tab32.ensure(cells)) return rc;
  }
  Progress pg;
  if (rm.rows()) {
    if (int rc = e->rows.ensure(std::max<size_t>(1, plan.max_blocks * rm.width))) return rc;
    if (int rc = e->part.ensure(std::max<size_t>(1, plan.max_slices * rm.width))) return rc;
    pg.part.resize(plan.tot_slices * rm.width);
    pg.part_point.reserve(plan.tot_slices);
  }
  if (rm.second())
    if (int rc = prepare_second(e, rm, plan, n_idx)) return rc;
  if (int rc = e->counts.ensure((size_t)(1ull << 20) * n_idx)) return rc;
  if (int rc = e->tot.ensure((size_t)n_points * n_idx)) return rc;
  MIMO_HIP_TRY(hipMemsetAsync(e->tot.p, 0, sizeof(unsigned long long) * n_points * n_idx, e->stream));
  if (int rc = key.f64 ? run_launches(e, key, base_params<double>(e, key, it, incl_clean, n_idx), plan, n_points, pts,
                                      seeds, rm, per_trial, &pg)
                       : run_launches(e, key, base_params<float>(e, key, it, incl_clean, n_idx), plan, n_points, pts,
                                      seeds, rm, per_trial, &pg))
    return rc;

  std::vector<unsigned long long> tot((size_t)n_points * n_idx);
  MIMO_HIP_TRY(hipMemcpyAsync(tot.data(), e->tot.p, sizeof(unsigned long long) * tot.size(), hipMemcpyDeviceToHost,
                              e->stream));
  MIMO_HIP_TRY(hipStreamSynchronize(e->stream));
  const uint64_t bits_per_trial = (uint64_t)c.n_sub_carr * (uint64_t)std::lround(std::log2((double)c.constel_size));
  for (int i = 0; i < n_points; ++i)
    for (int j = 0; j < n_idx; ++j) {
      err_out[(size_t)i * n_idx + j] += tot[(size_t)i * n_idx + j];
      bits_out[(size_t)i * n_idx + j] += bits_per_trial * n_trials[i];
    }
  if (rm.rows()) {
    // per point, its slice partials in slice order (a fixed order: equal calls, equal bits),
    // then one add into the caller's row
    const int w = rm.width;
    std::vector<double> ptot((size_t)n_points * w, 0.0);
    for (size_t k = 0; k < pg.part_point.size(); ++k)
      for (int j = 0; j < w; ++j) ptot[(size_t)pg.part_point[k] * w + j] += pg.part[k * w + j];
    for (size_t i = 0; i < ptot.size(); ++i) rm.out[i] += ptot[i];
  }
  e->last_ms = pg.ms;
  e->last_beam_ms = rm.beam ? pg.second_ms : 0.0;
  e->last_decode_ms = rm.coded || rm.turbo ? pg.second_ms : 0.0;
  e->last_chan_ms = pg.chan_ms;
  return MIMO_OK;
}

// What every row-mode entry point checks first: the engine, its precision and the mode's output (or
// first required) argument; mode and arg are their names in the refusals.
int row_call(const mimo_engine* e, const char* mode, const void* arg, const char* arg_name) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  if (e->cfg.precision != MIMO_PREC_F64)
    return fail(MIMO_EINVAL, std::string(mode) + " needs a float64 engine (no float32 " + mode + " instances are built)");
  if (!arg) return fail(MIMO_EINVAL, std::string("null ") + arg_name);
  return MIMO_OK;
}

// The instances' scale num / x of a call's x (name: ref_pow, rho_max), or why it has none; what: the
// scale in the refusal's words.
int scale_of(const char* name, double x, double num, const char* what, double* scale) {
  if (!(x > 0) || !std::isfinite(x)) return fail(MIMO_EINVAL, std::string(name) + " must be finite and > 0");
  *scale = num / x;
  if (!(*scale > 0) || !std::isfinite(*scale))
    return fail(MIMO_EINVAL, std::string(name) + " leaves no finite " + what + " > 0");
  return MIMO_OK;
}

// n_idx of a width function's arguments, or its refusal.
int width_n_idx(int32_t n_iters, int32_t incl_clean) {
  if (n_iters < 1 || n_iters > 32) return fail(MIMO_EINVAL, "n_iters must be in [1, 32]");
  return n_iters + (incl_clean ? 1 : 0);
}

}  // namespace

extern "C" {

int32_t mimo_engine_run(mimo_engine* e, uint64_t seed, uint64_t first_trial, uint64_t n_trials, const int32_t* iters,
                        int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out, uint32_t* per_trial) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  if (!e->have_point) return fail(MIMO_EINVAL, "mimo_engine_set_point was not called");
  if (n_trials == 0) {  // validate the iteration list, add nothing
    return run_points(e, 0, nullptr, nullptr, nullptr, nullptr, iters, n_iters, incl_clean, err_out, bits_out,
                      per_trial, RowMode{});
  }
  return run_points(e, 1, &e->pt, &seed, &first_trial, &n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial, RowMode{});
}

int32_t mimo_engine_run_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                               const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                               int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                               uint32_t* per_trial) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  return run_points(e, n_points, points, seeds, first_trial, n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial, RowMode{});
}

int32_t mimo_measure_width(int32_t n_iters, int32_t incl_clean) {
  const int n_idx = width_n_idx(n_iters, incl_clean);
  return n_idx < 0 ? n_idx : row_width(MIMO_MODE_MEAS, 0, n_idx, 0);
}

int32_t mimo_engine_measure_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                   const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                   int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                   uint32_t* per_trial, double* meas_out, double* per_trial_meas) {
  if (int rc = row_call(e, "measure", meas_out, "meas_out")) return rc;
  return run_points(e, n_points, points, seeds, first_trial, n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial, RowMode{MIMO_MODE_MEAS, meas_out, per_trial_meas});
}

int32_t mimo_spectrum_width(int32_t n_fft) {
  if (!is_pow2(n_fft) || n_fft < 128 || n_fft > 8192)
    return fail(MIMO_EINVAL, "n_fft must be a power of two in [128, 8192]");
  return row_width(MIMO_MODE_SPEC, n_fft, 0, 0);
}

int32_t mimo_engine_spectrum_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                    const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                    int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                    uint32_t* per_trial, double* spec_out, double* per_trial_spec) {
  if (int rc = row_call(e, "spectrum", spec_out, "spec_out")) return rc;
  return run_points(e, n_points, points, seeds, first_trial, n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial, RowMode{MIMO_MODE_SPEC, spec_out, per_trial_spec});
}

int32_t mimo_beam_width(int32_t n_probes) {
  if (n_probes < 1 || n_probes > MIMO_BEAM_MAX_PROBES)
    return fail(MIMO_EINVAL, "n_probes must be in [1, " + std::to_string(MIMO_BEAM_MAX_PROBES) + "]");
  return row_width(MIMO_MODE_BEAM, 0, 0, n_probes);
}

int32_t mimo_engine_beam_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                uint32_t* per_trial, const double* probes, int32_t n_probes, double* beam_out,
                                double* per_trial_beam) {
  if (int rc = row_call(e, "beam", probes, "probes")) return rc;
  if (!beam_out) return fail(MIMO_EINVAL, "null beam_out");
  if (mimo_beam_width(n_probes) < 0) return MIMO_EINVAL;
  const int A = e->cfg.n_ant, F = e->cfg.n_fft;
  BeamCall bc;
  bc.n_probes = n_probes;
  bc.buffer = env_lowered("MIMO_BEAM_BUFFER_BYTES", MIMO_BEAM_BUFFER_BYTES);
  if (bc.buffer < beam_trial_bytes(e->cfg))
    return fail(MIMO_EINVAL, "one trial's beam cells (" + std::to_string(beam_trial_bytes(e->cfg)) + " B at n_ant " +
                                 std::to_string(A) + ", n_fft " + std::to_string(F) +
                                 ") do not fit the beam buffer of " + std::to_string(bc.buffer) + " B");
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
                    per_trial, RowMode{MIMO_MODE_BEAM, beam_out, per_trial_beam, 0.0, &bc});
}

int32_t mimo_envelope_width(void) { return row_width(MIMO_MODE_ENV, 0, 0, 0); }

// The lower edge of bin b >= 1 in units of u = |.|^2 / ref_pow: the smallest v = 1.0625 u whose
// bits >> 49 are 8088 + b is 2^(-12 + b / 8) (1 + (b % 8) / 8), exactly.
int32_t mimo_envelope_edges(double* edges_out) {
  if (!edges_out) return fail(MIMO_EINVAL, "null edges_out");
  for (int b = 1; b < MIMO_ENV_BINS; ++b)
    edges_out[b - 1] = std::ldexp(1.0 + (b % 8) / 8.0, -12 + b / 8) * 16.0 / 17.0;
  return MIMO_OK;
}

int32_t mimo_engine_envelope_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                    const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                    int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                    uint32_t* per_trial, double ref_pow, double* env_out, double* per_trial_env) {
  if (int rc = row_call(e, "envelope", env_out, "env_out")) return rc;
  double scale;
  if (int rc = scale_of("ref_pow", ref_pow, 1.0625, "bin scale 1.0625 / ref_pow", &scale)) return rc;
  return run_points(e, n_points, points, seeds, first_trial, n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial, RowMode{MIMO_MODE_ENV, env_out, per_trial_env, scale});
}

int32_t mimo_soft_width(int32_t n_iters, int32_t incl_clean) {
  const int n_idx = width_n_idx(n_iters, incl_clean);
  return n_idx < 0 ? n_idx : row_width(MIMO_MODE_SOFT, 0, n_idx, 0);
}

int32_t mimo_engine_soft_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                uint32_t* per_trial, double rho_max, double* soft_out, double* per_trial_soft) {
  if (int rc = row_call(e, "soft", soft_out, "soft_out")) return rc;
  double scale;
  if (int rc = scale_of("rho_max", rho_max, 128.0, "bin scale 128 / rho_max", &scale)) return rc;
  return run_points(e, n_points, points, seeds, first_trial, n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial, RowMode{MIMO_MODE_SOFT, soft_out, per_trial_soft, scale});
}

int32_t mimo_coded_width(int32_t n_iters, int32_t incl_clean) {
  const int n_idx = width_n_idx(n_iters, incl_clean);
  return n_idx < 0 ? n_idx : row_width(MIMO_MODE_CODED, 0, n_idx, 0);
}

int32_t mimo_coded_codewords(int32_t n_sub_carr, int32_t constel_size, const mimo_ldpc_code* code) {
  mimo::LdpcHost h;
  std::string err;
  if (!mimo::ldpc_prepare(code, &h, &err)) return fail(MIMO_EINVAL, err);
  const int L = (int)std::lround(std::sqrt((double)constel_size));
  if (L * L != constel_size || !is_pow2(constel_size) || constel_size < 4 || constel_size > 4096)
    return fail(MIMO_EINVAL, "Constellation size must be a power of some number, only square QAM supported.");
  if (n_sub_carr < 1) return fail(MIMO_EINVAL, "n_sub_carr must be >= 1");
  const int64_t stream = (int64_t)n_sub_carr * (int64_t)std::lround(std::log2((double)constel_size));
  if ((int64_t)h.n_bits() > stream)
    return fail(MIMO_EINVAL, "code: N = n_cols z = " + std::to_string(h.n_bits()) + " code bits exceed the " +
                                 std::to_string(stream) + " bits (n_sub_carr log2 constel_size) of one trial");
  return (int32_t)(stream / h.n_bits());
}

int32_t mimo_engine_coded_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                 const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                 int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                 uint32_t* per_trial, const mimo_ldpc_code* code, double rho_max, double* coded_out,
                                 double* per_trial_coded, int8_t* per_trial_chan) {
  if (int rc = row_call(e, "coded", coded_out, "coded_out")) return rc;
  const int n_cw = mimo_coded_codewords(e->cfg.n_sub_carr, e->cfg.constel_size, code);
  if (n_cw < 0) return MIMO_EINVAL;
  double scale;
  if (int rc = scale_of("rho_max", rho_max, 32.0, "scale 32 / rho_max", &scale)) return rc;
  CodedCall cc;
  std::string err;
  if (!mimo::ldpc_prepare(code, &cc.code, &err)) return fail(MIMO_EINVAL, err);
  cc.n_cw = n_cw;
  cc.stream = (size_t)e->cfg.n_sub_carr * (size_t)std::lround(std::log2((double)e->cfg.constel_size));
  cc.per_trial_chan = per_trial_chan;
  return run_points(e, n_points, points, seeds, first_trial, n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial, RowMode{MIMO_MODE_CODED, coded_out, per_trial_coded, scale, nullptr, &cc});
}

int32_t mimo_turbo_width(int32_t n_passes) {
  if (n_passes < 1 || n_passes > MIMO_TURBO_MAX_PASSES)
    return fail(MIMO_EINVAL, "n_passes must be in [1, " + std::to_string(MIMO_TURBO_MAX_PASSES) + "]");
  return MIMO_CODED_FIXED * n_passes;
}

int32_t mimo_engine_turbo_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                 const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                 int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                 uint32_t* per_trial, const mimo_ldpc_code* code, double rho_max, int32_t n_passes,
                                 double* turbo_out, double* per_trial_turbo, int8_t* per_trial_chan,
                                 double* per_trial_z) {
  if (int rc = row_call(e, "turbo", turbo_out, "turbo_out")) return rc;
  if (e->cfg.receiver_kind != MIMO_RX_CNC)
    return fail(MIMO_EINVAL, "receiver_kind: turbo needs a MIMO_RX_CNC engine (MCNC with decoder feedback is not built)");
  if (mimo_turbo_width(n_passes) < 0) return MIMO_EINVAL;
  const int n_cw = mimo_coded_codewords(e->cfg.n_sub_carr, e->cfg.constel_size, code);
  if (n_cw < 0) return MIMO_EINVAL;
  double scale;
  if (int rc = scale_of("rho_max", rho_max, 32.0, "scale 32 / rho_max", &scale)) return rc;
  TurboCall tc;
  std::string err;
  if (!mimo::ldpc_prepare(code, &tc.cc.code, &err)) return fail(MIMO_EINVAL, err);
  tc.cc.n_cw = n_cw;
  tc.cc.stream = (size_t)e->cfg.n_sub_carr * (size_t)std::lround(std::log2((double)e->cfg.constel_size));
  tc.cc.per_trial_chan = per_trial_chan;
  tc.n_passes = n_passes;
  tc.per_trial_z = per_trial_z;
  RowMode rm{MIMO_MODE_TURBO, turbo_out, per_trial_turbo, scale};
  rm.turbo = &tc;
  return run_points(e, n_points, points, seeds, first_trial, n_trials, iters, n_iters, incl_clean, err_out, bits_out,
                    per_trial, rm);
}

int32_t mimo_engine_cnc_step(mimo_engine* e, const mimo_point* point, const double* z_iq, const int32_t* labels,
                             int64_t n, double* v_out) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  if (e->cfg.precision != MIMO_PREC_F64)
    return fail(MIMO_EINVAL, "cnc_step needs a float64 engine (no float32 step instances are built)");
  if (e->cfg.receiver_kind != MIMO_RX_CNC) return fail(MIMO_EINVAL, "receiver_kind: cnc_step needs a MIMO_RX_CNC engine");
  if (!point) return fail(MIMO_EINVAL, "null point");
  if (int rc = validate_point(e, point)) return rc;
  if (n < 0 || n > (1ll << 20)) return fail(MIMO_EINVAL, "n must be in [0, 1048576]");
  if (n == 0) return MIMO_OK;
  if (!z_iq || !labels || !v_out) return fail(MIMO_EINVAL, "null z_iq, labels or v_out");
  const size_t S = (size_t)e->cfg.n_sub_carr, cells = (size_t)n * S;
  for (size_t i = 0; i < cells; ++i)
    if (labels[i] < 0 || labels[i] >= e->cfg.constel_size)
      return fail(MIMO_EINVAL, "labels[" + std::to_string(i) + "] must be in [0, constel_size)");
  const mimo::InstanceKey key = select_instance(e, false);
  if (int rc = ensure_device(e)) return rc;
  using TP = mimo::TrialParams<double>;
  TP tp = base_params<double>(e, key, Iters{}, 0, 1);
  fill_point(e, *point, 0, 0, tp);
  // a one-point table behind the parameters, as a trial launch has it: TP | block offsets {0, n}
  mimo::DBuf tab, dz, dl, dv;
  const size_t off = (sizeof(TP) + 15) & ~size_t(15);
  MIMO_HIP_TRY(tab.alloc(off + 2 * sizeof(uint32_t)));
  MIMO_HIP_TRY(dz.alloc(cells * 16));
  MIMO_HIP_TRY(dl.alloc(cells * sizeof(int32_t)));
  MIMO_HIP_TRY(dv.alloc(cells * 16));
  const uint32_t start[2] = {0u, (uint32_t)n};
  MIMO_HIP_TRY(hipMemcpy(tab.p, &tp, sizeof(TP), hipMemcpyHostToDevice));
  MIMO_HIP_TRY(hipMemcpy(tab.as<char>() + off, start, sizeof start, hipMemcpyHostToDevice));
  MIMO_HIP_TRY(hipMemcpy(dz.p, z_iq, cells * 16, hipMemcpyHostToDevice));
  MIMO_HIP_TRY(hipMemcpy(dl.p, labels, cells * sizeof(int32_t), hipMemcpyHostToDevice));
  tp.points = tab.as<TP>();
  tp.point_start = reinterpret_cast<const uint32_t*>(tab.as<char>() + off);
  tp.n_points = 1;
  mimo::StepArgs a{};
  a.z = dz.as<double2>();
  a.labels = dl.as<int32_t>();
  a.v_out = dv.as<double2>();
  bool found = false;
  const hipError_t se = mimo::launch_turbo_step(key, false, (unsigned)n, e->stream, tp, a, &found);
  if (!found) return fail(MIMO_ENOKERNEL, "no step kernel instance for " + describe(key));
  if (se != hipSuccess) return fail(MIMO_EHIP, std::string("step kernel launch: ") + hipGetErrorString(se));
  MIMO_HIP_TRY(hipStreamSynchronize(e->stream));
  MIMO_HIP_TRY(hipMemcpy(v_out, dv.p, cells * 16, hipMemcpyDeviceToHost));
  return MIMO_OK;
}

int64_t mimo_bank_capacity(int32_t n_ant, int32_t n_sub_carr, int32_t precision) {
  if (n_ant < 1) return fail(MIMO_EINVAL, "n_ant must be >= 1");
  if (n_sub_carr < 1) return fail(MIMO_EINVAL, "n_sub_carr must be >= 1");
  if (precision != MIMO_PREC_F64 && precision != MIMO_PREC_F32)
    return fail(MIMO_EINVAL, "precision must be MIMO_PREC_F64 or MIMO_PREC_F32");
  const uint64_t cell = precision == MIMO_PREC_F32 ? sizeof(float2) : sizeof(double2);
  return (int64_t)(MIMO_BANK_BUFFER_BYTES / ((uint64_t)n_ant * (uint64_t)n_sub_carr * cell));
}

int32_t mimo_engine_set_channel_bank(mimo_engine* e, int32_t n_bank, const double* tables) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  const mimo_config& c = e->cfg;
  if (c.channel_kind != MIMO_CH_TABLE)
    return fail(MIMO_EINVAL, "channel_kind: a channel bank needs a MIMO_CH_TABLE engine");
  const int64_t cap = mimo_bank_capacity(c.n_ant, c.n_sub_carr, c.precision);
  if (n_bank < 0 || n_bank > cap)
    return fail(MIMO_EINVAL, "n_bank must be in [0, " + std::to_string(cap) + "] (mimo_bank_capacity)");
  if (n_bank > 0 && !tables) return fail(MIMO_EINVAL, "tables is required for n_bank > 0");
  const size_t A = (size_t)c.n_ant, S = (size_t)c.n_sub_carr, F = (size_t)c.n_fft;
  for (size_t j = 0; j < (size_t)n_bank; ++j)
    for (size_t i = 0; i < A * F * 2; ++i)
      if (!std::isfinite(tables[j * A * F * 2 + i]))
        return fail(MIMO_EINVAL, "tables must be finite (entry " + std::to_string(j) + ", antenna " +
                                     std::to_string(i / 2 / F) + ")");
  // keep the in-band columns, bins b(k), in the engine's precision (float32: rounded to nearest)
  const bool f32 = c.precision == MIMO_PREC_F32;
  std::vector<double2> b64(f32 ? 0 : (size_t)n_bank * A * S);
  std::vector<float2> b32(f32 ? (size_t)n_bank * A * S : 0);
  for (size_t j = 0; j < (size_t)n_bank; ++j)
    for (size_t a = 0; a < A; ++a)
      for (size_t k = 0; k < S; ++k) {
        const double* v = tables + ((j * A + a) * F + (size_t)band_bin((int)k, (int)S, (int)F)) * 2;
        if (f32) b32[(j * A + a) * S + k] = make_float2((float)v[0], (float)v[1]);
        else b64[(j * A + a) * S + k] = make_double2(v[0], v[1]);
      }
  e->bank64.swap(b64);
  e->bank32.swap(b32);
  e->n_bank = n_bank;
  e->tab_stale = true;
  return MIMO_OK;
}

int32_t mimo_engine_set_tdl(mimo_engine* e, const mimo_tdl* prof) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  if (e->cfg.channel_kind != MIMO_CH_TDL)
    return fail(MIMO_EINVAL, "channel_kind: a TDL profile needs a MIMO_CH_TDL engine");
  mimo::TdlHost host;
  std::string err;
  if (!mimo::tdl_prepare(prof, e->cfg.n_ant, e->cfg.n_fft, &host, &err)) return fail(MIMO_EINVAL, err);
  e->tdl = std::move(host);
  e->tdl_is_rays = false;
  e->have_tdl = true;
  e->tdl_stale = true;
  return MIMO_OK;
}

int32_t mimo_engine_set_rays(mimo_engine* e, const mimo_rays* prof) {
  if (!e) return fail(MIMO_EINVAL, "null engine");
  if (e->cfg.channel_kind != MIMO_CH_TDL)
    return fail(MIMO_EINVAL, "channel_kind: a ray-cluster profile needs a MIMO_CH_TDL engine");
  mimo::RaysHost host;
  std::string err;
  if (!mimo::rays_prepare(prof, e->cfg.n_ant, e->cfg.n_fft, &host, &err)) return fail(MIMO_EINVAL, err);
  e->rays = std::move(host);
  e->tdl_is_rays = true;
  e->have_tdl = true;
  e->tdl_stale = true;
  return MIMO_OK;
}

double mimo_engine_last_chan_ms(const mimo_engine* e) { return e ? e->last_chan_ms : 0.0; }
double mimo_engine_last_kernel_ms(const mimo_engine* e) { return e ? e->last_ms : 0.0; }
double mimo_engine_last_decode_ms(const mimo_engine* e) { return e ? e->last_decode_ms : 0.0; }
double mimo_engine_last_beam_ms(const mimo_engine* e) { return e ? e->last_beam_ms : 0.0; }

const char* mimo_engine_describe(const mimo_engine* e) {
  if (!e) return "";
  if (e->desc.empty())
    const_cast<mimo_engine*>(e)->desc = describe(select_instance(e, e->have_point && e->pt.csi_eps >= 0));
  return e->desc.c_str();
}

// Whatever device state exists goes with the engine (~mimo_engine), ready or not.
void mimo_engine_destroy(mimo_engine* e) { delete e; }

}  // extern "C"
