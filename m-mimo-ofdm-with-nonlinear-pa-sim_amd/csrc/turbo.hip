// The step kernel of the turbo mode (turbo.h): per trial, the decisions of the pass before -- the
// decoder's where it decoded, the demapper's on the undecoded tail -- are re-modulated, sent through
// the receiver's PA model and subtracted from the received vector, v = z - dist, and v is demapped
// to the next pass's channel values.  The CNC part is the fused kernel's own (trial_kernel.h, the
// RX_CNC loop): the instance's FFT type, slot map, pa_block, qam.h and softbits.h on the engine's
// twiddle tables, with the decided labels in place of the slice.  No Box-Muller tables and no alpha
// table: the kernel holds the FFT's exchange buffer and the wave-split twiddle copy alone.
#include "turbo.h"

#include "trial_kernel.h"

namespace mimo {
namespace {

template <int F, int NSLOT, bool ALIGNED, bool FIRST>
__global__ __launch_bounds__(team_size64(F)) void turbo_step(TrialParams<double> p0, StepArgs a) {
  using R = double;
  using C = cx<R>;
  constexpr int T = team_size64(F);
  using FFT = trial_fft_t<R, F, T, 1>;
  using SL = Slots<F, T, NSLOT, ALIGNED>;
  constexpr int P = FFT::P;
  constexpr bool WAVEFFT = wave_fft_used(F, T, true);
  constexpr bool COLD_OUT = F != 4096 || MIMO_COLD_OUT_4096 != 0;  // as the trial kernel
  // ---- which point and trial this block runs (the trial kernel's search over point_start)
  uint32_t pi = 0;
  if (p0.n_points > 1) {
    uint32_t lo = 0, hi = (uint32_t)p0.n_points;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (p0.point_start[mid] <= blockIdx.x) lo = mid; else hi = mid;
    }
    pi = lo;
  }
  using CParams = const __attribute__((address_space(4))) TrialParams<R>;
  CParams& p = *(CParams*)(p0.points + pi);
  __shared__ C lds[FIRST ? 1 : FFT::LDS_TOTAL];
  constexpr int TW1_N = [] {
    if constexpr (WAVEFFT && !FIRST) return FFT::TWL_N; else return 1;
  }();
  __shared__ C tw1_s[TW1_N];
  const C* tw1 = WAVEFFT && !FIRST ? tw1_s : nullptr;
  const int t = threadIdx.x;
  const bool t0 = (t == 0);
  const int tf = FFT::freq_thread(t);
  if constexpr (WAVEFFT && !FIRST) {
    fill_tw1<FFT, T>(tw1_s, p.tw_wave);
    __syncthreads();
  }
  const uint32_t trial = (uint32_t)(p.first_trial + (blockIdx.x - p0.point_start[pi]));
  const Key key{(uint32_t)p.seed, (uint32_t)(p.seed >> 32)};
  const int S = p.n_sc, L = p.qam_l, hb = p.half_bits;
  const size_t stream = (size_t)S * (size_t)(2 * hb);
  const size_t zrow = (size_t)blockIdx.x * (size_t)S, srow = (size_t)blockIdx.x * stream;

  // the thread's sub-carriers: the transmitted labels (the trial kernel's draw) and z
  int ks[NSLOT];
  uint32_t valid_mask = 0, lab[NSLOT];
  C v[NSLOT];
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    bool ok;
    ks[s] = SL::k_of(s, tf, S, ok);
    valid_mask |= (ok ? 1u : 0u) << s;
    lab[s] = ok && !a.labels ? qam_label(key, ks[s], trial, p.label_mask) : 0u;
    v[s] = ok ? a.z[zrow + (size_t)ks[s]] : czero<R>();
  }

  if constexpr (!FIRST) {
    // the decided labels: bit j of the stream is bit 2 hb - 1 - j of the label
    uint32_t lh[NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      lh[s] = 0u;
      if (!((valid_mask >> s) & 1u)) continue;
      if (a.labels) {
        lh[s] = (uint32_t)a.labels[zrow + (size_t)ks[s]];
        continue;
      }
      uint32_t e = 0u;
      for (int j = 0; j < 2 * hb; ++j) {
        const size_t pos = (size_t)j * (size_t)S + (size_t)ks[s];
        const bool wrong = pos < (size_t)a.n_dec ? a.hard[srow + pos] != 0 : a.chan_in[srow + pos] < 0;
        e |= (wrong ? 1u : 0u) << (2 * hb - 1 - j);
      }
      lh[s] = lab[s] ^ e;
    }
    // corrector.py:84-110 with the decided symbols (trial_kernel.h, the RX_CNC loop's body)
    const R inv_sqrt_f = p.inv_sqrt_f;
    C d[P], x[NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s)
      x[s] = ((valid_mask >> s) & 1u) ? cscale(qam_point<R>(lh[s], L, hb), inv_sqrt_f) : czero<R>();
    SL::scatter(d, x, t0);
    FFT::template run<+1, 0, SL::zero_mask()>(d, lds, WAVEFFT ? p.tw_wave : p.tw, t, false, typename FFT::NoFill{}, tw1);
    pa_block<COLD_OUT>(p.cnc_pa_kind, d, p.sat_cnc, p.sqrt_sat_cnc, p.inv_sat_cnc, p.rapp_p, p.toi_cnc);
    FFT::template run_second<-1>(d, lds, WAVEFFT ? p.tw_wave : p.tw, t, false, typename FFT::NoFill{}, tw1);
    const R sc = inv_sqrt_f * p.inv_alpha_cnc;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const C y = SL::gather(d, s, t0);
      const C dist = ((valid_mask >> s) & 1u) ? csub(cscale(y, sc), qam_point<R>(lh[s], L, hb)) : czero<R>();
      v[s] = csub(v[s], dist);
    }
  }

#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    if (!((valid_mask >> s) & 1u)) continue;
    if (a.v_out) a.v_out[zrow + (size_t)ks[s]] = v[s];
    if (a.chan_out) {
      // the coded instances' coded_put: one int8 per bit, signed by the transmitted bit
      const uint32_t li = lab[s] >> hb, lq = lab[s] & ((1u << hb) - 1u);
      int8_t* o = a.chan_out + srow + (size_t)ks[s];
      soft_axis((double)v[s].x, L, hb, [&](int j, double lam) {
        o[(size_t)(hb - 1 - j) * (size_t)S] = (int8_t)coded_value(lam, (li >> j) & 1u, a.scale);
      });
      soft_axis((double)v[s].y, L, hb, [&](int j, double lam) {
        o[(size_t)(2 * hb - 1 - j) * (size_t)S] = (int8_t)coded_value(lam, (lq >> j) & 1u, a.scale);
      });
    }
  }
}

struct Go {
  bool first;
  unsigned blocks;
  hipStream_t st;
  const TrialParams<double>* p;
  const StepArgs* a;
};

template <int F, int NSLOT, bool AL>
hipError_t go(const Go& g, bool* found) {
  *found = true;
  if (g.first) hipLaunchKernelGGL((turbo_step<F, NSLOT, AL, true>), dim3(g.blocks), dim3(team_size64(F)), 0, g.st, *g.p, *g.a);
  else hipLaunchKernelGGL((turbo_step<F, NSLOT, AL, false>), dim3(g.blocks), dim3(team_size64(F)), 0, g.st, *g.p, *g.a);
  return hipGetLastError();
}

// the slot maps of a size: trial_inst.hip by_team's
template <int F>
hipError_t by_slots(const InstanceKey& k, const Go& g, bool* found) {
  constexpr int T = team_size64(F), P = F / T;
  if (k.T != T) return hipSuccess;
  if (k.aligned) {
    if constexpr (8 < P) {
      if (k.nslot == 8) return go<F, 8, true>(g, found);
    }
    if constexpr (4 < P) {
      if (k.nslot == 4) return go<F, 4, true>(g, found);
    }
    return hipSuccess;
  }
  if (k.nslot != P) return hipSuccess;
  return go<F, P, false>(g, found);
}

hipError_t by_size(const InstanceKey& k, const Go& g, bool* found) {
  *found = false;
  if (!k.f64) return hipSuccess;
  switch (k.F) {
    case 128: return by_slots<128>(k, g, found);
    case 256: return by_slots<256>(k, g, found);
    case 512: return by_slots<512>(k, g, found);
    case 1024: return by_slots<1024>(k, g, found);
    case 2048: return by_slots<2048>(k, g, found);
    case 4096: return by_slots<4096>(k, g, found);
    case 8192: return by_slots<8192>(k, g, found);
    default: return hipSuccess;
  }
}

}  // namespace

hipError_t launch_turbo_step(const InstanceKey& key, bool first, unsigned blocks, hipStream_t st,
                             const TrialParams<double>& p, const StepArgs& a, bool* found) {
  if (blocks == 0) {
    *found = true;
    return hipSuccess;
  }
  return by_size(key, Go{first, blocks, st, &p, &a}, found);
}

}  // namespace mimo
