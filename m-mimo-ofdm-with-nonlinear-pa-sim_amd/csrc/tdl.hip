// The tapped-delay-line channel's generator kernel and its fine seam (tdl.h; include/mimo_engine.h
// mimo_engine_set_tdl, mimo_tdl_channels).  One workgroup per (block, antenna): its first wave draws
// the L taps into LDS, and after one barrier every thread accumulates the response of its columns
// over the taps in ascending order and stores it, the threads of a wave at adjacent columns.  The
// engine (in-band columns, the engine's precision) and the seam (every bin, complex128, the taps as
// well) run the same kernel template, so the same device functions: equal inputs, equal bits.
// The ray-cluster profile (mimo_engine_set_rays, mimo_rays_channels) is a kernel of its own,
// rays_fill, with another first stage and the same response; tdl_fill does not change with it.
#include "tdl.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "host_util.h"
#include "philox.h"

namespace mimo {
namespace {

constexpr int kTdlThreads = 256;
// Where the kernel reads the twiddle table W from: up to this n_fft a copy that every workgroup
// stages in dynamic LDS first (16 n_fft bytes: 64 KiB at 4096), beyond it global memory.  The
// generator is bound by these look-ups, not by its stores: against global memory the staged copy
// measured -26 % (8 taps) and -24 % (32) at n_fft 2048 and -46 % / -51 % at 4096
// (profiles/r20/tdl/; -DMIMO_TDL_W_LDS_MAX_F=0 builds the other side).  n_fft 8192 would take
// 128 KiB, one workgroup per CU, and was not measured: it reads global memory.  The values are the
// same either way, and so are the bits.
#ifndef MIMO_TDL_W_LDS_MAX_F
#define MIMO_TDL_W_LDS_MAX_F 4096
#endif
constexpr uint32_t kStreamTdl = 7;  // Philox stream of the taps (philox.h Stream; 6 is mimo_awgn's)

// Tap l of antenna a in trial `trial`: scale sqrt(-ln u1) exp(j 2 pi u2), mimo_awgn's formula.
__device__ __forceinline__ double2 tdl_tap(Key key, uint32_t l, uint32_t trial, uint32_t a, double scale) {
  const uint4 w = philox4x32_10(make_uint4(l, trial, kStreamTdl, a), key);
  const double u1 = ((double)w.x + 0.5) * 2.3283064365386963e-10, u2 = (double)w.y * 2.3283064365386963e-10;
  const double r = scale * sqrt(-log(u1));
  double s, c;
  sincospi(2.0 * u2, &s, &c);
  return make_double2(r * c, r * s);
}

// H at FFT bin `bin`: sum_l g[l] W[(bin d[l]) mod F] in ascending l from 0, each complex product as
// four fused multiply-adds written out (no contraction left to the compiler).  bin d < 2^26.
__device__ __forceinline__ double2 tdl_response(const double2* g, const int* d, int L, const double2* W,
                                                uint32_t bin, uint32_t fmask) {
  double re = 0.0, im = 0.0;
  for (int l = 0; l < L; ++l) {
    const double2 w = W[(bin * (uint32_t)d[l]) & fmask];
    const double2 t = g[l];
    re = fma(t.x, w.x, re);
    re = fma(-t.y, w.y, re);
    im = fma(t.x, w.y, im);
    im = fma(t.y, w.x, im);
  }
  return make_double2(re, im);
}

__device__ __forceinline__ void tdl_store(double2* p, double2 v) { *p = v; }
__device__ __forceinline__ void tdl_store(float2* p, double2 v) { *p = make_float2((float)v.x, (float)v.y); }

// grid (blocks, antennas).  n_sc > 0: the in-band columns of the trial kernel's table [block][A][S];
// n_sc = 0: all F bins.  WLDS: W staged in F double2 of dynamic LDS (the same values: the same bits).
template <typename OUT, bool WLDS>
__global__ __launch_bounds__(kTdlThreads) void tdl_fill(const double2* W, const double* __restrict__ sqrt_pow,
                                                        const double* __restrict__ ant_amp,
                                                        const int32_t* __restrict__ delays, int L, int F, int A, int n_sc,
                                                        const TdlSeg* __restrict__ segs,
                                                        const uint32_t* __restrict__ seg_start, int n_seg,
                                                        OUT* __restrict__ out, double2* __restrict__ taps) {
  __shared__ double2 g_s[kTdlMaxTaps];
  __shared__ int d_s[kTdlMaxTaps];
  const uint32_t b = blockIdx.x;
  const uint32_t a = blockIdx.y;
  uint32_t lo = 0, hi = (uint32_t)n_seg;  // uniform binary search, as the trial kernel's over point_start
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (seg_start[mid] <= b) lo = mid; else hi = mid;
  }
  const TdlSeg sg = segs[lo];
  const uint32_t trial = (uint32_t)(sg.first_trial + (b - seg_start[lo]));
  const Key key{(uint32_t)sg.seed, (uint32_t)(sg.seed >> 32)};
  const int t = threadIdx.x;
  if (t < L) {  // L <= 64: the first wave
    const double2 g = tdl_tap(key, (uint32_t)t, trial, a, ant_amp[a] * sqrt_pow[t]);
    g_s[t] = g;
    d_s[t] = delays[t];
    if (taps) taps[((size_t)b * A + a) * L + t] = g;
  }
  if constexpr (WLDS) {
    extern __shared__ double2 w_s[];
    for (int m = t; m < F; m += kTdlThreads) w_s[m] = W[m];
    W = w_s;
  }
  __syncthreads();
  const int n_cols = n_sc ? n_sc : F;
  const int half = n_sc >> 1;
  OUT* row = out + ((size_t)b * A + a) * n_cols;
  for (int c = t; c < n_cols; c += kTdlThreads) {
    const int bin = n_sc ? (c < half ? F - half + c : c - half + 1) : c;
    tdl_store(row + c, tdl_response(g_s, d_s, L, W, (uint32_t)bin, (uint32_t)F - 1u));
  }
}

// ---- the ray-cluster profile (tdl.h RaysHost) ----
constexpr uint32_t kStreamRays = 8;  // Philox stream of the ray gains
constexpr int kRayLanes = 16;                                  // adjacent lanes that share a tap's sum
constexpr int kRayGroups = kTdlThreads / kRayLanes;            // 16 such groups
constexpr int kRayTapsPerGroup = kTdlMaxTaps / kRayGroups;     // group g owns the taps g, g + 16, g + 32, g + 48

// Gain of ray r in trial `trial`: amp sqrt(-ln u1) exp(j 2 pi u2) (tdl_tap's formula, the amplitude
// folded into the radius), or amp exp(j 2 pi u2) for a specular ray.  The same for every antenna.
__device__ __forceinline__ double2 ray_gain(Key key, uint32_t r, uint32_t trial, double amp, bool specular) {
  const uint4 w = philox4x32_10(make_uint4(r, trial, kStreamRays, 0u), key);
  const double u1 = ((double)w.x + 0.5) * 2.3283064365386963e-10, u2 = (double)w.y * 2.3283064365386963e-10;
  const double rad = specular ? amp : amp * sqrt(-log(u1));
  double s, c;
  sincospi(2.0 * u2, &s, &c);
  return make_double2(rad * c, rad * s);
}

// A ray's term of its tap, c steer: the four fused multiply-adds of tdl_response onto (0, 0).
__device__ __forceinline__ double2 ray_term(double2 c, double2 s) {
  double re = fma(c.x, s.x, 0.0), im = fma(c.x, s.y, 0.0);
  re = fma(-c.y, s.y, re);
  im = fma(c.y, s.x, im);
  return make_double2(re, im);
}

// Sum of the terms [r0, r1) for the calling group of 16 lanes, in tdl.h's order: lane j of the group
// adds r0 + j, r0 + j + 16, ... in ascending r, then the 16 partial sums meet in a butterfly (all
// lanes: the same bits).  Every lane of the wave calls it, whatever its range.
__device__ __forceinline__ double2 ray_tap_sum(const double2* p_s, int r0, int r1, int lane) {
  double re = 0.0, im = 0.0;
  for (int r = r0 + lane; r < r1; r += kRayLanes) {
    const double2 p = p_s[r];
    re += p.x;
    im += p.y;
  }
  for (int d = kRayLanes / 2; d; d >>= 1) {
    re += __shfl_xor(re, d, 64);
    im += __shfl_xor(im, d, 64);
  }
  return make_double2(re, im);
}

// Dynamic LDS of rays_fill in double2: a scratch block of max(R, kRaysScratch) -- first the R terms
// of the antenna, then, in their place, the L taps and (from entry kTdlMaxTaps) the L delays -- and
// behind it W (F) where it is staged.  No static LDS.
constexpr int kRaysScratch = kTdlMaxTaps + kTdlMaxTaps / 4;
__host__ __device__ constexpr int rays_scratch(int R) { return R > kRaysScratch ? R : kRaysScratch; }

// tdl_fill's grid, segment lookup and column loop; ahead of them the ray stage:
//  1. thread t draws the gains of the rays t, t + 256, ..., multiplies each by the antenna's steering
//     value and leaves the term in LDS (antenna 0's workgroup also stores the gain);
//  2. barrier; group g of 16 lanes sums the terms of the taps g, g + 16, ... (ray_tap_sum), its
//     lane k keeping the k-th of them;
//  3. barrier; the taps and the delays take the terms' place in LDS; barrier; tdl_response.
//
// The three choices of this stage, from the CU's 160 KiB of LDS, its residency rule (workgroups per
// CU <= floor(160 KiB / LDS per workgroup)) and the measurements in profiles/r26/rays/ (generator
// time over the TDL generator's at the same delays, config 2 and the paper geometry, 8 / 32 taps):
//  * steer's row a is read straight from global memory, by the thread that draws the ray's gain
//    and ahead of the draw.  A workgroup uses each of its R values once, the threads of a wave read
//    adjacent 16-byte values, and the load's latency passes behind the draw's few hundred
//    instructions.  A copy of the row in LDS beside the gains, read inside the tap sums, measured
//    slower than the global reads there (+9 % at 640 rays, +29 % at 1,024, config 2) and was dropped.
//  * The tap sums go one tap per group of 16 lanes, the lanes interleaved over the tap's terms and
//    a four-step butterfly at the end; they read LDS only, and the groups' ranges are loaded ahead
//    of the draws.  One tap of 1,024 rays is 64 additions deep per lane, not 1,024 deep on one
//    thread, and 64 taps of one ray are four short butterflies per group.  One tap per wave (six
//    steps, up to 16 taps in turn) measured +27 to +31 % over the TDL generator at 1 to 20 rays per
//    tap, config 2; this split +7 to +15 %: the steps' latency is the cost, not the additions.
//  * W stays staged in LDS up to MIMO_TDL_W_LDS_MAX_F.  At F 4096 that is 64 KiB, and the terms'
//    16 KiB at R 1,024 make 80 KiB: two workgroups per CU as for tdl_fill, but only because the
//    taps and delays reuse the terms' block.  With 1.25 KiB of static LDS on top (one workgroup per
//    CU) R 1,024 measured 2.65 ms at 8 taps against 2.04 ms with W in global memory; as built
//    1.48 ms against 2.02 ms, and 4.1 against 8.2 ms at 32 taps.
template <typename OUT, bool WLDS>
__global__ __launch_bounds__(kTdlThreads) void rays_fill(const double2* W, const double2* __restrict__ steer,
                                                         const double* __restrict__ ray_amp,
                                                         const uint8_t* __restrict__ ray_kind,
                                                         const int32_t* __restrict__ tap_first,
                                                         const int32_t* __restrict__ delays, int L, int R, int F, int A,
                                                         int n_sc, const TdlSeg* __restrict__ segs,
                                                         const uint32_t* __restrict__ seg_start, int n_seg,
                                                         OUT* __restrict__ out, double2* __restrict__ taps,
                                                         double2* __restrict__ gains) {
  extern __shared__ double2 rays_s[];
  const uint32_t b = blockIdx.x;
  const uint32_t a = blockIdx.y;
  uint32_t lo = 0, hi = (uint32_t)n_seg;  // tdl_fill's search
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (seg_start[mid] <= b) lo = mid; else hi = mid;
  }
  const TdlSeg sg = segs[lo];
  const uint32_t trial = (uint32_t)(sg.first_trial + (b - seg_start[lo]));
  const Key key{(uint32_t)sg.seed, (uint32_t)(sg.seed >> 32)};
  const int t = threadIdx.x;
  const int lane = t & (kRayLanes - 1), grp = t / kRayLanes;
  int r0[kRayTapsPerGroup], r1[kRayTapsPerGroup];  // the ranges of the group's taps, loaded ahead of the draws
#pragma unroll
  for (int k = 0; k < kRayTapsPerGroup; ++k) {
    const int l = grp + k * kRayGroups;
    r0[k] = l < L ? tap_first[l] : 0;
    r1[k] = l < L ? tap_first[l + 1] : 0;
  }
  const double2* srow = steer + (size_t)a * R;
  // the gains are redrawn by every antenna's workgroup: R draws against S L complex products
  for (int r = t; r < R; r += kTdlThreads) {
    const double2 s = srow[r];
    const double2 c = ray_gain(key, (uint32_t)r, trial, ray_amp[r], ray_kind[r] != 0);
    rays_s[r] = ray_term(c, s);
    if (gains && a == 0) gains[(size_t)b * R + r] = c;
  }
  if constexpr (WLDS) {
    double2* w_s = rays_s + rays_scratch(R);
    for (int m = t; m < F; m += kTdlThreads) w_s[m] = W[m];
    W = w_s;
  }
  __syncthreads();
  double2 mine = make_double2(0.0, 0.0);  // tap grp + 16 lane
#pragma unroll
  for (int k = 0; k < kRayTapsPerGroup; ++k) {
    if (k * kRayGroups >= L) break;  // uniform in the workgroup
    const double2 g = ray_tap_sum(rays_s, r0[k], r1[k], lane);
    if (lane == k) mine = g;
  }
  __syncthreads();  // every term is read
  double2* g_s = rays_s;
  int* d_s = reinterpret_cast<int*>(rays_s + kTdlMaxTaps);
  const int l_mine = grp + kRayGroups * lane;
  if (lane < kRayTapsPerGroup && l_mine < L) {
    g_s[l_mine] = mine;
    d_s[l_mine] = delays[l_mine];
    if (taps) taps[((size_t)b * A + a) * L + l_mine] = mine;
  }
  __syncthreads();
  const int n_cols = n_sc ? n_sc : F;
  const int half = n_sc >> 1;
  OUT* row = out + ((size_t)b * A + a) * n_cols;
  for (int c = t; c < n_cols; c += kTdlThreads) {
    const int bin = n_sc ? (c < half ? F - half + c : c - half + 1) : c;
    tdl_store(row + c, tdl_response(g_s, d_s, L, W, (uint32_t)bin, (uint32_t)F - 1u));
  }
}

}  // namespace

std::vector<double> TdlHost::blob() const {
  const int L = n_taps, F = n_fft, A = n_ant;
  std::vector<double> v((size_t)2 * F + L + A + (L + 1) / 2, 0.0);
  // W[m] = exp(-j 2 pi m / F), formed in long double and rounded once; W[0] = (1, -0.0)
  const long double two_pi = 8.0L * atanl(1.0L);
  for (int m = 0; m < F; ++m) {
    const long double ang = two_pi * (long double)m / (long double)F;
    v[2 * (size_t)m] = (double)cosl(ang);
    v[2 * (size_t)m + 1] = (double)(-sinl(ang));
  }
  std::copy(sqrt_pow.begin(), sqrt_pow.end(), v.begin() + 2 * (size_t)F);
  std::copy(ant_amp.begin(), ant_amp.end(), v.begin() + 2 * (size_t)F + L);
  std::memcpy(v.data() + 2 * (size_t)F + L + A, delays.data(), sizeof(int32_t) * (size_t)L);
  return v;
}

bool tdl_prepare(const mimo_tdl* prof, int n_ant, int n_fft, TdlHost* out, std::string* err) {
  auto bad = [&](const std::string& m) {
    *err = m;
    return false;
  };
  if (!prof) return bad("null profile (mimo_tdl)");
  if (prof->n_taps < 1 || prof->n_taps > kTdlMaxTaps)
    return bad("n_taps must be in [1, " + std::to_string(kTdlMaxTaps) + "]");
  if (!prof->delays) return bad("delays is required");
  if (!prof->powers) return bad("powers is required");
  const int L = prof->n_taps;
  for (int l = 0; l < L; ++l) {
    if (prof->delays[l] < 0 || prof->delays[l] >= n_fft)
      return bad("delays must be in [0, n_fft) (tap " + std::to_string(l) + ")");
    if (l && prof->delays[l] <= prof->delays[l - 1])
      return bad("delays must be strictly ascending (tap " + std::to_string(l) + ")");
    if (!(prof->powers[l] > 0) || !std::isfinite(prof->powers[l]))
      return bad("powers must be finite and > 0 (tap " + std::to_string(l) + ")");
  }
  if (prof->ant_amp)
    for (int a = 0; a < n_ant; ++a)
      if (!(prof->ant_amp[a] > 0) || !std::isfinite(prof->ant_amp[a]))
        return bad("ant_amp must be finite and > 0 (antenna " + std::to_string(a) + ")");
  out->n_taps = L;
  out->n_ant = n_ant;
  out->n_fft = n_fft;
  out->delays.assign(prof->delays, prof->delays + L);
  out->sqrt_pow.resize(L);
  for (int l = 0; l < L; ++l) out->sqrt_pow[l] = std::sqrt(prof->powers[l]);
  if (prof->ant_amp) out->ant_amp.assign(prof->ant_amp, prof->ant_amp + n_ant);
  else out->ant_amp.assign(n_ant, 1.0);
  return true;
}

hipError_t launch_tdl(hipStream_t st, const TdlHost& prof, const double* blob, const TdlSeg* segs,
                      const uint32_t* seg_start, int n_seg, uint32_t n_blocks, int n_sc, double2* out64, float2* out32,
                      double2* taps) {
  if (n_blocks == 0) return hipSuccess;
  const int L = prof.n_taps, F = prof.n_fft, A = prof.n_ant;
  const double2* W = reinterpret_cast<const double2*>(blob);
  const double* sqrt_pow = blob + 2 * (size_t)F;
  const double* ant_amp = sqrt_pow + L;
  const int32_t* delays = reinterpret_cast<const int32_t*>(ant_amp + A);
  const dim3 grid(n_blocks, (unsigned)A);
  auto go = [&](auto kernel, auto* out) -> hipError_t {
    const size_t lds = F <= MIMO_TDL_W_LDS_MAX_F ? (size_t)F * sizeof(double2) : 0;
    if (lds > (48u << 10))  // beyond the default limit of a launch
      if (hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
        return e;
    hipLaunchKernelGGL(kernel, grid, dim3(kTdlThreads), lds, st, W, sqrt_pow, ant_amp, delays, L, F, A, n_sc, segs,
                       seg_start, n_seg, out, taps);
    return hipGetLastError();
  };
  const bool wlds = F <= MIMO_TDL_W_LDS_MAX_F;
  if (out64) return wlds ? go(tdl_fill<double2, true>, out64) : go(tdl_fill<double2, false>, out64);
  return wlds ? go(tdl_fill<float2, true>, out32) : go(tdl_fill<float2, false>, out32);
}

size_t RaysHost::off_steer() const {
  const size_t base = (size_t)2 * tdl.n_fft + tdl.n_taps + tdl.n_ant + (tdl.n_taps + 1) / 2;  // TdlHost::blob()
  return (base + 1) & ~size_t(1);  // double2: 16 bytes
}

std::vector<double> RaysHost::blob() const {
  const size_t R = (size_t)n_rays;
  std::vector<double> v = tdl.blob();
  v.resize(off_kind() + (R + 7) / 8, 0.0);
  std::copy(steer.begin(), steer.end(), v.begin() + off_steer());
  std::copy(ray_amp.begin(), ray_amp.end(), v.begin() + off_amp());
  std::memcpy(v.data() + off_first(), tap_first.data(), sizeof(int32_t) * tap_first.size());
  std::memcpy(v.data() + off_tap(), ray_tap.data(), sizeof(int32_t) * R);
  std::memcpy(v.data() + off_kind(), ray_kind.data(), R);
  return v;
}

bool rays_prepare(const mimo_rays* prof, int n_ant, int n_fft, RaysHost* out, std::string* err) {
  auto bad = [&](const std::string& m) {
    *err = m;
    return false;
  };
  if (!prof) return bad("null profile (mimo_rays)");
  if (prof->n_taps < 1 || prof->n_taps > kTdlMaxTaps)
    return bad("n_taps must be in [1, " + std::to_string(kTdlMaxTaps) + "]");
  if (prof->n_rays < prof->n_taps || prof->n_rays > kRaysMax)
    return bad("n_rays must be in [n_taps, " + std::to_string(kRaysMax) + "]");
  if (!prof->delays) return bad("delays is required");
  if (!prof->ray_tap) return bad("ray_tap is required");
  if (!prof->ray_amp) return bad("ray_amp is required");
  if (!prof->steer) return bad("steer is required");
  const int L = prof->n_taps, R = prof->n_rays;
  for (int l = 0; l < L; ++l) {
    if (prof->delays[l] < 0 || prof->delays[l] >= n_fft)
      return bad("delays must be in [0, n_fft) (tap " + std::to_string(l) + ")");
    if (l && prof->delays[l] <= prof->delays[l - 1])
      return bad("delays must be strictly ascending (tap " + std::to_string(l) + ")");
  }
  if (prof->ray_tap[0] != 0) return bad("ray_tap must start at tap 0 (ray 0)");
  for (int r = 1; r < R; ++r)
    if (prof->ray_tap[r] != prof->ray_tap[r - 1] && prof->ray_tap[r] != prof->ray_tap[r - 1] + 1)
      return bad("ray_tap must be non-decreasing in steps of 0 or 1 (ray " + std::to_string(r) + ")");
  if (prof->ray_tap[R - 1] != L - 1) return bad("ray_tap must end at tap n_taps - 1: every tap needs a ray");
  for (int r = 0; r < R; ++r) {
    if (!(prof->ray_amp[r] > 0) || !std::isfinite(prof->ray_amp[r]))
      return bad("ray_amp must be finite and > 0 (ray " + std::to_string(r) + ")");
    if (prof->ray_kind && prof->ray_kind[r] > 1)
      return bad("ray_kind must be 0 (diffuse) or 1 (specular) (ray " + std::to_string(r) + ")");
  }
  for (int a = 0; a < n_ant; ++a)
    for (int r = 0; r < R; ++r) {
      const double* z = prof->steer + 2 * ((size_t)a * R + r);
      if (!std::isfinite(z[0]) || !std::isfinite(z[1]))
        return bad("steer must be finite (antenna " + std::to_string(a) + ", ray " + std::to_string(r) + ")");
    }
  out->tdl.n_taps = L;
  out->tdl.n_ant = n_ant;
  out->tdl.n_fft = n_fft;
  out->tdl.delays.assign(prof->delays, prof->delays + L);
  out->tdl.sqrt_pow.assign(L, 1.0);
  out->tdl.ant_amp.assign(n_ant, 1.0);
  out->n_rays = R;
  out->ray_tap.assign(prof->ray_tap, prof->ray_tap + R);
  out->ray_amp.assign(prof->ray_amp, prof->ray_amp + R);
  if (prof->ray_kind) out->ray_kind.assign(prof->ray_kind, prof->ray_kind + R);
  else out->ray_kind.assign(R, 0);
  out->steer.assign(prof->steer, prof->steer + 2 * (size_t)n_ant * R);
  out->tap_first.assign(L + 1, R);
  for (int r = R - 1; r >= 0; --r) out->tap_first[prof->ray_tap[r]] = r;
  return true;
}

hipError_t launch_rays(hipStream_t st, const RaysHost& prof, const double* blob, const TdlSeg* segs,
                       const uint32_t* seg_start, int n_seg, uint32_t n_blocks, int n_sc, double2* out64,
                       float2* out32, double2* taps, double2* gains) {
  if (n_blocks == 0) return hipSuccess;
  const int L = prof.tdl.n_taps, F = prof.tdl.n_fft, A = prof.tdl.n_ant, R = prof.n_rays;
  const double2* W = reinterpret_cast<const double2*>(blob);
  const int32_t* delays = reinterpret_cast<const int32_t*>(blob + 2 * (size_t)F + L + A);
  const double2* steer = reinterpret_cast<const double2*>(blob + prof.off_steer());
  const double* ray_amp = blob + prof.off_amp();
  const int32_t* tap_first = reinterpret_cast<const int32_t*>(blob + prof.off_first());
  const uint8_t* ray_kind = reinterpret_cast<const uint8_t*>(blob + prof.off_kind());
  const dim3 grid(n_blocks, (unsigned)A);
  const bool wlds = F <= MIMO_TDL_W_LDS_MAX_F;
  auto go = [&](auto kernel, auto* out) -> hipError_t {
    const size_t lds = ((size_t)rays_scratch(R) + (wlds ? (size_t)F : 0)) * sizeof(double2);  // 80 KiB at most
    if (lds > (32u << 10))  // at or beyond the default limit of a launch (set from 32 KiB on: it costs nothing)
      if (hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
        return e;
    hipLaunchKernelGGL(kernel, grid, dim3(kTdlThreads), lds, st, W, steer, ray_amp, ray_kind, tap_first, delays, L, R, F,
                       A, n_sc, segs, seg_start, n_seg, out, taps, gains);
    return hipGetLastError();
  };
  if (out64) return wlds ? go(rays_fill<double2, true>, out64) : go(rays_fill<double2, false>, out64);
  return wlds ? go(rays_fill<float2, true>, out32) : go(rays_fill<float2, false>, out32);
}

}  // namespace mimo

using mimo::fail;

extern "C" int32_t mimo_tdl_channels(const mimo_tdl* prof, int32_t n_ant, int32_t n_fft, uint64_t seed,
                                     uint64_t first_trial, int64_t n, double* h_out, double* taps_out) {
  if (n_fft < 2 || n_fft > 8192 || (n_fft & (n_fft - 1)))
    return fail(MIMO_EINVAL, "n_fft must be a power of two in [2, 8192]");
  if (n_ant < 1 || n_ant > 4096) return fail(MIMO_EINVAL, "n_ant must be in [1, 4096]");
  if (n < 0) return fail(MIMO_EINVAL, "n must be >= 0");
  mimo::TdlHost host;
  std::string err;
  if (!mimo::tdl_prepare(prof, n_ant, n_fft, &host, &err)) return fail(MIMO_EINVAL, err);
  if (n == 0) return MIMO_OK;
  if (!h_out) return fail(MIMO_EINVAL, "null h_out");
  const std::vector<double> blob = host.blob();
  const size_t per_trial = (size_t)n_ant * (size_t)n_fft, L = (size_t)host.n_taps;
  // trials of one launch: at most 256 MiB of responses
  const int64_t chunk = std::max<int64_t>(1, (int64_t)((256u << 20) / (per_trial * sizeof(double2))));
  const int64_t nb_max = std::min(n, chunk);
  mimo::DBuf d_blob, d_seg, d_h, d_taps;  // the seam's device allocations, released with the call
  MIMO_HIP_TRY(hipMalloc(&d_blob.p, blob.size() * sizeof(double)));
  MIMO_HIP_TRY(hipMalloc(&d_seg.p, sizeof(mimo::TdlSeg) + 2 * sizeof(uint32_t)));
  MIMO_HIP_TRY(hipMalloc(&d_h.p, (size_t)nb_max * per_trial * sizeof(double2)));
  if (taps_out) MIMO_HIP_TRY(hipMalloc(&d_taps.p, (size_t)nb_max * n_ant * L * sizeof(double2)));
  MIMO_HIP_TRY(hipMemcpy(d_blob.p, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice));
  for (int64_t done = 0; done < n; done += chunk) {
    const int64_t nb = std::min(chunk, n - done);
    struct {
      mimo::TdlSeg seg;
      uint32_t start[2];
    } tab{{seed, first_trial + (uint64_t)done}, {0u, (uint32_t)nb}};
    MIMO_HIP_TRY(hipMemcpy(d_seg.p, &tab, sizeof tab, hipMemcpyHostToDevice));
    const char* seg_base = static_cast<const char*>(d_seg.p);
    MIMO_HIP_TRY(mimo::launch_tdl(nullptr, host, static_cast<const double*>(d_blob.p),
                                  reinterpret_cast<const mimo::TdlSeg*>(seg_base),
                                  reinterpret_cast<const uint32_t*>(seg_base + sizeof(mimo::TdlSeg)), 1, (uint32_t)nb,
                                  0, static_cast<double2*>(d_h.p), nullptr, static_cast<double2*>(d_taps.p)));
    MIMO_HIP_TRY(hipMemcpy(h_out + (size_t)done * per_trial * 2, d_h.p, (size_t)nb * per_trial * sizeof(double2),
                           hipMemcpyDeviceToHost));
    if (taps_out)
      MIMO_HIP_TRY(hipMemcpy(taps_out + (size_t)done * n_ant * L * 2, d_taps.p,
                             (size_t)nb * n_ant * L * sizeof(double2), hipMemcpyDeviceToHost));
  }
  return MIMO_OK;
}

extern "C" int32_t mimo_rays_channels(const mimo_rays* prof, int32_t n_ant, int32_t n_fft, uint64_t seed,
                                      uint64_t first_trial, int64_t n, double* h_out, double* taps_out,
                                      double* gains_out) {
  if (n_fft < 2 || n_fft > 8192 || (n_fft & (n_fft - 1)))
    return fail(MIMO_EINVAL, "n_fft must be a power of two in [2, 8192]");
  if (n_ant < 1 || n_ant > 4096) return fail(MIMO_EINVAL, "n_ant must be in [1, 4096]");
  if (n < 0) return fail(MIMO_EINVAL, "n must be >= 0");
  mimo::RaysHost host;
  std::string err;
  if (!mimo::rays_prepare(prof, n_ant, n_fft, &host, &err)) return fail(MIMO_EINVAL, err);
  if (n == 0) return MIMO_OK;
  if (!h_out) return fail(MIMO_EINVAL, "null h_out");
  const std::vector<double> blob = host.blob();
  const size_t per_trial = (size_t)n_ant * (size_t)n_fft, L = (size_t)host.tdl.n_taps, R = (size_t)host.n_rays;
  // trials of one launch: at most 256 MiB of responses
  const int64_t chunk = std::max<int64_t>(1, (int64_t)((256u << 20) / (per_trial * sizeof(double2))));
  const int64_t nb_max = std::min(n, chunk);
  mimo::DBuf d_blob, d_seg, d_h, d_taps, d_gains;  // the seam's device allocations, released with the call
  MIMO_HIP_TRY(hipMalloc(&d_blob.p, blob.size() * sizeof(double)));
  MIMO_HIP_TRY(hipMalloc(&d_seg.p, sizeof(mimo::TdlSeg) + 2 * sizeof(uint32_t)));
  MIMO_HIP_TRY(hipMalloc(&d_h.p, (size_t)nb_max * per_trial * sizeof(double2)));
  if (taps_out) MIMO_HIP_TRY(hipMalloc(&d_taps.p, (size_t)nb_max * n_ant * L * sizeof(double2)));
  if (gains_out) MIMO_HIP_TRY(hipMalloc(&d_gains.p, (size_t)nb_max * R * sizeof(double2)));
  MIMO_HIP_TRY(hipMemcpy(d_blob.p, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice));
  for (int64_t done = 0; done < n; done += chunk) {
    const int64_t nb = std::min(chunk, n - done);
    struct {
      mimo::TdlSeg seg;
      uint32_t start[2];
    } tab{{seed, first_trial + (uint64_t)done}, {0u, (uint32_t)nb}};
    MIMO_HIP_TRY(hipMemcpy(d_seg.p, &tab, sizeof tab, hipMemcpyHostToDevice));
    const char* seg_base = static_cast<const char*>(d_seg.p);
    MIMO_HIP_TRY(mimo::launch_rays(nullptr, host, static_cast<const double*>(d_blob.p),
                                   reinterpret_cast<const mimo::TdlSeg*>(seg_base),
                                   reinterpret_cast<const uint32_t*>(seg_base + sizeof(mimo::TdlSeg)), 1, (uint32_t)nb,
                                   0, static_cast<double2*>(d_h.p), nullptr, static_cast<double2*>(d_taps.p),
                                   static_cast<double2*>(d_gains.p)));
    MIMO_HIP_TRY(hipMemcpy(h_out + (size_t)done * per_trial * 2, d_h.p, (size_t)nb * per_trial * sizeof(double2),
                           hipMemcpyDeviceToHost));
    if (taps_out)
      MIMO_HIP_TRY(hipMemcpy(taps_out + (size_t)done * n_ant * L * 2, d_taps.p,
                             (size_t)nb * n_ant * L * sizeof(double2), hipMemcpyDeviceToHost));
    if (gains_out)
      MIMO_HIP_TRY(hipMemcpy(gains_out + (size_t)done * R * 2, d_gains.p, (size_t)nb * R * sizeof(double2),
                             hipMemcpyDeviceToHost));
  }
  return MIMO_OK;
}
