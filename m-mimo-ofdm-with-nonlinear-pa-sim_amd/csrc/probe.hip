// libmimo_probe: the trial kernel's building blocks behind plain C entry points (probe.h).
//
// Every kernel here is a thin shell around production code: the instance's FFT type
// (trial_kernel.h trial_fft_t), pa_block, fill_lut64 / fill_tw1 and the real.h primitives, on
// the tables host_tables.h builds for the engine.  Nothing is restated, so a rounded table, a
// dropped Newton step or a truncated series shows in the values these return
// (tests/test_gpu_probe_*.py compare them with a long-double reference).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "host_util.h"
#include "trial_kernel.h"
#include "trial_launch.h"
#include "host_tables.h"
#include "probe.h"

namespace {
thread_local std::string g_perr;  // this library's message, behind mimo_probe_last_error()
}
namespace mimo {
void set_error(const std::string& m) { g_perr = m; }
}  // namespace mimo
static_assert(MIMO_PROBE_EHIP == MIMO_EHIP, "MIMO_HIP_TRY returns the probe's code for a HIP error");

namespace {

using namespace mimo;

// The production zero mask of (F, T) with the band S = F / 2: S / T = P / 2 slots per thread,
// which the engine runs on the aligned slot map for P = 16 and 8 (engine.hip select_instance:
// S / T in {8, 4}) and on the generic one (no zero registers) else.
template <int F, int T>
constexpr uint32_t probe_zero_mask() {
  constexpr int P = F / T;
  if constexpr (P == 16) return Slots<F, T, 8, true>::zero_mask();
  else if constexpr (P == 8) return Slots<F, T, 4, true>::zero_mask();
  else return 0u;
}

template <typename R, int F, int T, int NBUF>
__global__ __launch_bounds__(T) void probe_fft_kernel(const cx<R>* __restrict__ in, cx<R>* __restrict__ out,
                                                      const cx<R>* tw, int masked, int pa_kind, R sat, R sqrt_sat,
                                                      R inv_sat, R rapp_p, R toi) {
  using C = cx<R>;
  using FFT = trial_fft_t<R, F, T, NBUF>;
  constexpr int P = FFT::P;
  constexpr bool WAVEFFT = wave_fft_used(F, T, sizeof(R) == 8);
  constexpr uint32_t ZM = probe_zero_mask<F, T>();
  constexpr bool COLD_OUT = sizeof(R) == 8 && (F != 4096 || MIMO_COLD_OUT_4096 != 0);  // as the trial kernel
  __shared__ C lds[FFT::LDS_TOTAL];
  constexpr int TW1_N = [] {
    if constexpr (WAVEFFT) return FFT::TWL_N; else return 1;
  }();
  __shared__ C tw1_s[TW1_N];
  const C* tw1 = WAVEFFT ? tw1_s : nullptr;
  const int t = threadIdx.x;
  if constexpr (WAVEFFT) {
    fill_tw1<FFT, T>(tw1_s, tw);
    __syncthreads();
  }
  const int tf = FFT::freq_thread(t);
  const C* row = in + (size_t)blockIdx.x * F;
  C d[P];
#pragma unroll
  for (int m = 0; m < P; ++m) d[m] = row[tf + T * m];
  if (masked) {
#pragma unroll
    for (int m = 0; m < P; ++m)
      if ((ZM >> m) & 1u) d[m] = czero<R>();
    FFT::template run<+1, 0, ZM>(d, lds, tw, t, false, typename FFT::NoFill{}, tw1);
  } else {
    FFT::template run<+1, 0, 0u>(d, lds, tw, t, false, typename FFT::NoFill{}, tw1);
  }
  pa_block<COLD_OUT>(pa_kind, d, sat, sqrt_sat, inv_sat, rapp_p, toi);
  FFT::template run_second<-1>(d, lds, tw, t, false, typename FFT::NoFill{}, tw1);
  C* orow = out + (size_t)blockIdx.x * F;
#pragma unroll
  for (int m = 0; m < P; ++m) orow[tf + T * m] = d[m];
}

// The table an instance's transform reads, as the engine uploads it (engine.hip ensure_device).
template <typename R>
std::vector<cx<R>> instance_table(int F, int T) {
  constexpr bool F64 = sizeof(R) == 8;
  using Cvt = std::conditional_t<F64, TwToF64, TwToF32>;
  if (wave_fft_used(F, T, F64)) return wave_twiddles(F, T, Cvt{});
  if constexpr (F64) {
    if (split_fft_used(F, T, true)) return split_twiddles(F, T);
  }
  return team_twiddles(F, T, Cvt{});
}

template <typename R, int F, int T, int NBUF>
int run_fft(int masked, int pa_kind, double sat, double p, double toi, int n_rows, const void* in, void* out) {
  using C = cx<R>;
  const std::vector<C> tw = instance_table<R>(F, T);
  DBuf dtw, din, dout;
  const size_t bytes = sizeof(C) * (size_t)F * n_rows;
  MIMO_HIP_TRY(dtw.alloc(sizeof(C) * tw.size()));
  MIMO_HIP_TRY(din.alloc(bytes));
  MIMO_HIP_TRY(dout.alloc(bytes));
  MIMO_HIP_TRY(hipMemcpy(dtw.p, tw.data(), sizeof(C) * tw.size(), hipMemcpyHostToDevice));
  MIMO_HIP_TRY(hipMemcpy(din.p, in, bytes, hipMemcpyHostToDevice));
  // the PA parameters as engine.hip fill_point forms them
  const R sat_r = (R)sat, sqrt_sat = (R)std::sqrt(std::max(sat, 0.0)), inv_sat = sat > 0 ? (R)(1.0 / sat) : R(0);
  if (n_rows > 0)
    hipLaunchKernelGGL((probe_fft_kernel<R, F, T, NBUF>), dim3((unsigned)n_rows), dim3(T), 0, 0, din.as<C>(),
                       dout.as<C>(), dtw.as<C>(), masked, pa_kind, sat_r, sqrt_sat, inv_sat, (R)p, (R)toi);
  MIMO_HIP_TRY(hipGetLastError());
  MIMO_HIP_TRY(hipDeviceSynchronize());
  MIMO_HIP_TRY(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
  return MIMO_PROBE_OK;
}

struct FftArgs {
  int masked, pa_kind;
  double sat, p, toi;
  int n_rows;
  const void* in;
  void* out;
  // info query (no launch) when non-null
  int32_t* team;
  uint32_t* zero_mask;
  int32_t* fft_kind;
};

template <typename R, int F, int T, int NBUF>
int fft_or_info(const FftArgs& a) {
  if (a.team) {
    constexpr bool F64 = sizeof(R) == 8;
    *a.team = T;
    *a.zero_mask = probe_zero_mask<F, T>();
    *a.fft_kind = wave_fft_used(F, T, F64) ? 1 : split_fft_used(F, T, F64) ? 2 : 0;
    return MIMO_PROBE_OK;
  }
  return run_fft<R, F, T, NBUF>(a.masked, a.pa_kind, a.sat, a.p, a.toi, a.n_rows, a.in, a.out);
}

template <int F>
int by_variant(int prec, int variant, const FftArgs& a) {
  if (prec == 0) {
    if (variant == 0) return fft_or_info<double, F, team_size64(F), 1>(a);
  } else {
    if (variant == 0) return fft_or_info<float, F, team_size(F), 1>(a);
    if (variant == 1) return fft_or_info<float, F, team_size(F), 2>(a);
    if constexpr (alt_team_size(F) != team_size(F)) {
      if (variant == 2) return fft_or_info<float, F, alt_team_size(F), 1>(a);
      if (variant == 3) return fft_or_info<float, F, alt_team_size(F), 2>(a);
    }
  }
  return fail(MIMO_PROBE_ENOINST, "no such FFT instance");
}

int by_size(int prec, int F, int variant, const FftArgs& a) {
  if (prec != 0 && prec != 1) return fail(MIMO_PROBE_EINVAL, "prec must be 0 (float64) or 1 (float32)");
  switch (F) {
    case 128: return by_variant<128>(prec, variant, a);
    case 256: return by_variant<256>(prec, variant, a);
    case 512: return by_variant<512>(prec, variant, a);
    case 1024: return by_variant<1024>(prec, variant, a);
    case 2048: return by_variant<2048>(prec, variant, a);
    case 4096: return by_variant<4096>(prec, variant, a);
    case 8192: return by_variant<8192>(prec, variant, a);
    default: return fail(MIMO_PROBE_EINVAL, "F must be a power of two in [128, 8192]");
  }
}

// ---------------------------------------------------------------- float64 primitives
constexpr int kMathT = 256;
struct LutSrc {
  const double2* lut;
};
__global__ __launch_bounds__(kMathT) void probe_math_kernel(int fn, LutSrc src, const void* in, int64_t n,
                                                            double* __restrict__ o0, double* __restrict__ o1) {
  fill_lut64<kMathT>(&src, (int)threadIdx.x);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kMathT + threadIdx.x;
  if (i >= n) return;
  const uint32_t* wi = static_cast<const uint32_t*>(in);
  const double* di = static_cast<const double*>(in);
  double a = 0.0, b = 0.0;
  switch (fn) {
    case 0: a = ln_unit<-32>((double)wi[i] + 0.5); break;  // as philox.h bm_log calls it
    case 1: sincos_lut(wi[i], a, b); break;
    case 2: sincos_rev_lut(di[i], a, b); break;
    case 3: a = sqrt_n1(di[i]); break;
    case 4: a = rsq_n1(di[i]); break;
    case 5: a = rsq_r(di[i]); break;
    case 6: a = rpow_neg_inv<4>(di[i]); break;
    case 7: a = rpow_neg_inv<6>(di[i]); break;
    default: break;
  }
  o0[i] = a;
  if (o1) o1[i] = b;
}

// ---------------------------------------------------------------- PA block
constexpr int kPaT = 256, kPaP = 8;
template <typename R, bool COLD_OUT>
__global__ __launch_bounds__(kPaT) void probe_pa_kernel(const cx<R>* __restrict__ in, cx<R>* __restrict__ out,
                                                        int64_t n_tiles, int pa_kind, R sat, R sqrt_sat, R inv_sat,
                                                        R rapp_p, R toi) {
  const int64_t tile = (int64_t)blockIdx.x * kPaT + threadIdx.x;
  if (tile >= n_tiles) return;
  cx<R> d[kPaP];
#pragma unroll
  for (int m = 0; m < kPaP; ++m) d[m] = in[tile * kPaP + m];
  pa_block<COLD_OUT>(pa_kind, d, sat, sqrt_sat, inv_sat, rapp_p, toi);
#pragma unroll
  for (int m = 0; m < kPaP; ++m) out[tile * kPaP + m] = d[m];
}

template <typename R>
int run_pa(int cold_out, int pa_kind, double sat, double p, double toi, int64_t n, const void* in, void* out) {
  using C = cx<R>;
  const int64_t n_tiles = (n + kPaP - 1) / kPaP;
  const size_t padded = sizeof(C) * (size_t)n_tiles * kPaP, bytes = sizeof(C) * (size_t)n;
  DBuf din, dout;
  MIMO_HIP_TRY(din.alloc(padded));
  MIMO_HIP_TRY(dout.alloc(padded));
  MIMO_HIP_TRY(hipMemset(din.p, 0, padded ? padded : 1));  // the last tile's tail: zeros (in bounds, defined)
  MIMO_HIP_TRY(hipMemcpy(din.p, in, bytes, hipMemcpyHostToDevice));
  const R sat_r = (R)sat, sqrt_sat = (R)std::sqrt(std::max(sat, 0.0)), inv_sat = sat > 0 ? (R)(1.0 / sat) : R(0);
  const unsigned blocks = (unsigned)((n_tiles + kPaT - 1) / kPaT);
  if (blocks > 0) {
    if (cold_out)
      hipLaunchKernelGGL((probe_pa_kernel<R, true>), dim3(blocks), dim3(kPaT), 0, 0, din.as<C>(), dout.as<C>(), n_tiles,
                         pa_kind, sat_r, sqrt_sat, inv_sat, (R)p, (R)toi);
    else
      hipLaunchKernelGGL((probe_pa_kernel<R, false>), dim3(blocks), dim3(kPaT), 0, 0, din.as<C>(), dout.as<C>(), n_tiles,
                         pa_kind, sat_r, sqrt_sat, inv_sat, (R)p, (R)toi);
  }
  MIMO_HIP_TRY(hipGetLastError());
  MIMO_HIP_TRY(hipDeviceSynchronize());
  MIMO_HIP_TRY(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
  return MIMO_PROBE_OK;
}

bool known_size(int F) { return F >= 128 && F <= 8192 && (F & (F - 1)) == 0; }

template <class V>
int give_table(const std::vector<V>& t, void* buf, int64_t* n) {
  const int64_t cap = *n;
  *n = (int64_t)t.size();
  if (buf && cap >= (int64_t)t.size()) std::memcpy(buf, t.data(), sizeof(V) * t.size());
  return MIMO_PROBE_OK;
}

// The held transform addresses of the float64 wave-split instance at F (wave_fft.h XAddr): every
// thread's packed words from the formulas the kernel packs them with, or the caller's, and what
// the kernel's accessors unpack from them at each use site.
template <int F>
int32_t xaddr_of(const uint32_t* words_in, uint32_t* words, uint32_t* sites, int32_t* info) {
  constexpr int T = team_size64(F);
  using W = WaveFft<F, T, double, true, true>;
  using S = typename W::Sub;
  using XA = typename W::XAddr;
  static_assert(W::XA_PLAN, "the plan the held addresses are written for");
  constexpr int NS1 = 1 << S::bits_before(1), NS2 = 1 << S::bits_before(2);
  const int32_t inf[MIMO_PROBE_XADDR_INFO] = {T, W::WV, W::P, W::NB, W::FW, W::ROW, W::LDS_TOTAL, S::R0, S::XS0, NS1, NS2,
                                              S::CT ? S::ct_off(1) : 0, S::CT ? S::ct_off(2) : fft_tw_off(W::FW, W::P, 2),
                                              W::TWL_N, W::TW_INTER, W::CB,
                                              S::CT ? ct_rows(1 << S::bits(1)) : 1 << S::bits(1),
                                              S::CT ? ct_rows(1 << S::bits(2)) : 1 << S::bits(2), S::psh(1),
                                              wave_fft_tw_total(F, T) + wave_fft_ct_n(F, T), S::CT ? 1 : 0};
  for (int i = 0; i < MIMO_PROBE_XADDR_INFO; ++i) info[i] = inf[i];
  for (int t = 0; t < T; ++t) {
    XA xa{};
    if (words_in) {
      xa.w_cr = words_in[3 * t], xa.w_x = words_in[3 * t + 1], xa.w_t = words_in[3 * t + 2];
    } else {
      xa.w_cr = XA::word_cr(t), xa.w_x = XA::word_x(t), xa.w_t = XA::word_t(t);
    }
    xa.w = t >> 6;
    words[3 * t] = xa.w_cr, words[3 * t + 1] = xa.w_x, words[3 * t + 2] = xa.w_t;
    uint32_t* o = sites + (size_t)MIMO_PROBE_XADDR_SITES * t;
    o[0] = xa.cross(), o[1] = xa.row(), o[2] = xa.x0r(), o[3] = xa.x1w(), o[4] = xa.x1r();
    o[5] = xa.template tws<NS1>(), o[6] = xa.template tws<NS2>();
    o[7] = xa.tw_inv(1), o[8] = xa.tw_inv(2), o[9] = xa.tw_fwd(xa.w);
  }
  return MIMO_PROBE_OK;
}

}  // namespace

extern "C" {

const char* mimo_probe_last_error(void) { return g_perr.c_str(); }

int32_t mimo_probe_fft_info(int32_t prec, int32_t F, int32_t variant, int32_t* team, uint32_t* zero_mask,
                            int32_t* fft_kind) {
  if (!team || !zero_mask || !fft_kind) return fail(MIMO_PROBE_EINVAL, "null output");
  FftArgs a{};
  a.team = team;
  a.zero_mask = zero_mask;
  a.fft_kind = fft_kind;
  return by_size(prec, F, variant, a);
}

int32_t mimo_probe_fft(int32_t prec, int32_t F, int32_t variant, int32_t masked, int32_t pa_kind, double sat, double p,
                       double toi, int32_t n_rows, const void* in_freq, void* out_freq) {
  if (n_rows < 0 || n_rows > 65535) return fail(MIMO_PROBE_EINVAL, "n_rows must be in [0, 65535]");
  if (!in_freq || !out_freq) return fail(MIMO_PROBE_EINVAL, "null array");
  if (pa_kind < PA_NONE || pa_kind > PA_TOI) return fail(MIMO_PROBE_EINVAL, "unknown PA kind");
  if ((pa_kind == PA_SOFTLIM || pa_kind == PA_RAPP) && !(sat > 0)) return fail(MIMO_PROBE_EINVAL, "sat must be > 0");
  if (pa_kind == PA_RAPP && !(p > 0)) return fail(MIMO_PROBE_EINVAL, "p must be > 0");
  FftArgs a{};
  a.masked = masked ? 1 : 0;
  a.pa_kind = pa_kind;
  a.sat = sat;
  a.p = p;
  a.toi = toi;
  a.n_rows = n_rows;
  a.in = in_freq;
  a.out = out_freq;
  return by_size(prec, F, variant, a);
}

int32_t mimo_probe_math(int32_t fn, int64_t n, const void* in, double* out0, double* out1) {
  if (fn < 0 || fn > 7) return fail(MIMO_PROBE_EINVAL, "fn must be in [0, 7]");
  if (n < 0 || n > (int64_t)1 << 28) return fail(MIMO_PROBE_EINVAL, "n must be in [0, 2^28]");
  if (!in || !out0) return fail(MIMO_PROBE_EINVAL, "null array");
  const size_t in_bytes = (size_t)n * (fn <= 1 ? sizeof(uint32_t) : sizeof(double)), out_bytes = (size_t)n * sizeof(double);
  const std::vector<double2> lut = lut64_table();
  DBuf dlut, din, d0, d1;
  MIMO_HIP_TRY(dlut.alloc(sizeof(double2) * lut.size()));
  MIMO_HIP_TRY(din.alloc(in_bytes));
  MIMO_HIP_TRY(d0.alloc(out_bytes));
  if (out1) MIMO_HIP_TRY(d1.alloc(out_bytes));
  MIMO_HIP_TRY(hipMemcpy(dlut.p, lut.data(), sizeof(double2) * lut.size(), hipMemcpyHostToDevice));
  MIMO_HIP_TRY(hipMemcpy(din.p, in, in_bytes, hipMemcpyHostToDevice));
  const unsigned blocks = (unsigned)((n + kMathT - 1) / kMathT);
  if (blocks > 0)
    hipLaunchKernelGGL(probe_math_kernel, dim3(blocks), dim3(kMathT), 0, 0, fn, LutSrc{dlut.as<double2>()}, din.p, n,
                       d0.as<double>(), out1 ? d1.as<double>() : nullptr);
  MIMO_HIP_TRY(hipGetLastError());
  MIMO_HIP_TRY(hipDeviceSynchronize());
  MIMO_HIP_TRY(hipMemcpy(out0, d0.p, out_bytes, hipMemcpyDeviceToHost));
  if (out1) MIMO_HIP_TRY(hipMemcpy(out1, d1.p, out_bytes, hipMemcpyDeviceToHost));
  return MIMO_PROBE_OK;
}

int32_t mimo_probe_pa(int32_t prec, int32_t cold_out, int32_t pa_kind, double sat, double p, double toi, int64_t n,
                      const void* in_iq, void* out_iq) {
  if (prec != 0 && prec != 1) return fail(MIMO_PROBE_EINVAL, "prec must be 0 (float64) or 1 (float32)");
  if (n < 0 || n > (int64_t)1 << 28) return fail(MIMO_PROBE_EINVAL, "n must be in [0, 2^28]");
  if (!in_iq || !out_iq) return fail(MIMO_PROBE_EINVAL, "null array");
  if (pa_kind < PA_NONE || pa_kind > PA_TOI) return fail(MIMO_PROBE_EINVAL, "unknown PA kind");
  if ((pa_kind == PA_SOFTLIM || pa_kind == PA_RAPP) && !(sat > 0)) return fail(MIMO_PROBE_EINVAL, "sat must be > 0");
  if (pa_kind == PA_RAPP && !(p > 0)) return fail(MIMO_PROBE_EINVAL, "p must be > 0");
  return prec == 0 ? run_pa<double>(cold_out, pa_kind, sat, p, toi, n, in_iq, out_iq)
                   : run_pa<float>(cold_out, pa_kind, sat, p, toi, n, in_iq, out_iq);
}

int32_t mimo_probe_alpha_fit(double g0sq, double* amono19, double* apoly9, double* xlim) {
  if (!(g0sq > 0) || !std::isfinite(g0sq)) return fail(MIMO_PROBE_EINVAL, "g0sq must be finite and > 0");
  if (!amono19 || !apoly9 || !xlim) return fail(MIMO_PROBE_EINVAL, "null output");
  const AlphaFit f = fit_alpha(g0sq);
  for (int i = 0; i < 19; ++i) amono19[i] = f.amono[i];
  for (int i = 0; i < 9; ++i) apoly9[i] = f.apoly[i];
  *xlim = f.xlim;
  return MIMO_PROBE_OK;
}

int32_t mimo_probe_table(int32_t kind, int32_t prec, int32_t F, void* buf, int64_t* n) {
  if (!n) return fail(MIMO_PROBE_EINVAL, "null length");
  if (prec != 0 && prec != 1) return fail(MIMO_PROBE_EINVAL, "prec must be 0 (float64) or 1 (float32)");
  if (kind == 4) {
    if (prec != 0) return fail(MIMO_PROBE_ENOINST, "lut64 is a float64 table");
    return give_table(lut64_table(), buf, n);
  }
  if (!known_size(F)) return fail(MIMO_PROBE_EINVAL, "F must be a power of two in [128, 8192]");
  const bool f64 = prec == 0;
  switch (kind) {
    case 0:
      if (f64) {
        const int T = team_size64(F);
        return give_table(split_fft_used(F, T, true) ? split_twiddles(F, T) : team_twiddles(F, T, TwToF64{}), buf, n);
      }
      return give_table(team_twiddles(F, team_size(F), TwToF32{}), buf, n);
    case 1:
      if (f64) return fail(MIMO_PROBE_ENOINST, "the alternative team is float32 only");
      return give_table(team_twiddles(F, alt_team_size(F), TwToF32{}), buf, n);
    case 2:
      if (!f64) return fail(MIMO_PROBE_ENOINST, "the wave-split FFT's table is float64 only");
      if (!wave_fft_used(F, team_size64(F), true))
        return fail(MIMO_PROBE_ENOINST, "no wave-split FFT at this size and precision");
      return give_table(wave_twiddles(F, team_size64(F), TwToF64{}), buf, n);
    case 3:
      if (!f64 || !split_fft_used(F, team_size64(F), true))
        return fail(MIMO_PROBE_ENOINST, "no split FFT at this size and precision");
      return give_table(split_twiddles(F, team_size64(F)), buf, n);
    default:
      return fail(MIMO_PROBE_EINVAL, "kind must be in [0, 4]");
  }
}

int32_t mimo_probe_xaddr(int32_t F, const uint32_t* words_in, uint32_t* words, uint32_t* sites, int32_t* info) {
  if (!words || !sites || !info) return fail(MIMO_PROBE_EINVAL, "null output");
  if (!known_size(F) || !wave_fft_used(F, team_size64(F), true))
    return fail(MIMO_PROBE_ENOINST, "no wave-split FFT at this size");
  return F == 1024 ? xaddr_of<1024>(words_in, words, sites, info) : xaddr_of<2048>(words_in, words, sites, info);
}

}  // extern "C"
