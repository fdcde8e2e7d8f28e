// Beamforming kernel of the beam mode: the field of the array at a list of probe positions.
//
// For probe q, antenna a and FFT bin k the LoS channel is (oracle/refmath.py los_channel)
//   G_q[a,k] = exp(+j 2 pi d_qa f_k / c) c / (4 pi d_qa f_k),
// and per trial the kernel forms R_q[k] = sum_a G_q[a,k] Y_a[k], U_q[k] = sum_a G_q[a,k] X_a[k]
// (in band) and the five sums of include/mimo_engine.h from them.  N_q A F phasors and
// 8 N_q A (F + S) flops per trial with no reuse across bins: VALU work, one lane per bin.
//
// Mapping: a 256-thread block takes kBeamQT probes per wave (4 waves: 4 kBeamQT probes) and
// kBeamTT trials, and walks the F bins in chunks of 64 (lane = bin: the 16-byte loads of a wave
// are 1 KiB contiguous).  Per chunk and antenna a wave computes kBeamQT phasors and reuses each
// over the kBeamTT trials; the four waves read the same cells, so three of four reads hit the
// CU's L1.  The amplitude is separable, c / (4 pi d f) = (1 / d_qa) (1 / (4 pi f_k / c)): 1 / d_qa
// scales the phasor inside the antenna loop, the bin's factor the sums after it.  The phase is
// formed in cycles, u = d_qa (f_k / c), and reduced exactly (r = u - rint(u), |r| <= 1/2): two
// roundings before the reduction, none in it.  sin / cos of 2 pi r by unit_phasor below, which
// needs no argument handling beyond the quadrant (against the library's sincospi: 217 instead of
// 233 instructions per in-band antenna step; the time at config 2 with 181 probes is the same
// within the spread between runs, 22.7 to 23.3 against 23.3 to 23.7 ms).
// The lane's sums run over its bins in bin order, then a fixed shuffle tree sums the 64 lanes:
// the order depends on the sizes alone, so equal calls give equal bits.
#include "beam.h"

namespace mimo {
namespace {

constexpr int kBeamQT = 2;  // probes per wave
constexpr int kBeamTT = 4;  // trials per block
constexpr int kBeamThreads = 256;
constexpr double kInv4Pi = 0.07957747154594767;  // 1 / (4 pi)

// (sin, cos)(pi t) for |t| <= 1: t = n / 2 + z with n = rint(2 t) and |z| <= 1/4 (exact), the
// Taylor series of sin(pi z) to z^15 and of cos(pi z) to z^16 (the next terms are below 2^-54 at
// pi / 4; coefficients pi^k / k! rounded to nearest), then the quadrant's swap and signs.  Against a
// 120-bit evaluation the absolute error stays below 2 x 2^-53 (200,000 random arguments and the
// quadrant edges).
__device__ __forceinline__ void unit_phasor(double t, double& sn, double& cs) {
  const double n = rint(2.0 * t);
  const double z = fma(-0.5, n, t), z2 = z * z;
  double ps = -2.1915353447830217e-05;
  ps = fma(ps, z2, 0.00046630280576761255);
  ps = fma(ps, z2, -0.0073704309457143504);
  ps = fma(ps, z2, 0.08214588661112823);
  ps = fma(ps, z2, -0.5992645293207921);
  ps = fma(ps, z2, 2.5501640398773455);
  ps = fma(ps, z2, -5.16771278004997);
  ps = fma(ps, z2, 3.141592653589793) * z;
  double pc = 4.303069587032947e-06;
  pc = fma(pc, z2, -0.0001046381049248457);
  pc = fma(pc, z2, 0.0019295743094039231);
  pc = fma(pc, z2, -0.02580689139001406);
  pc = fma(pc, z2, 0.2353306303588932);
  pc = fma(pc, z2, -1.3352627688545895);
  pc = fma(pc, z2, 4.0587121264167685);
  pc = fma(pc, z2, -4.934802200544679);
  pc = fma(pc, z2, 1.0);
  const int q = (int)n;  // -2 ... 2; quadrant q mod 4: (s, c), (c, -s), (-s, -c), (-c, s)
  const double s = (q & 1) ? pc : ps, c = (q & 1) ? ps : pc;
  sn = (q & 2) ? -s : s;
  cs = ((q + 1) & 2) ? -c : c;
}

template <int QT, int TT>
__global__ __launch_bounds__(kBeamThreads) void beam_kernel(const double2* __restrict__ cells,
                                                            const double* __restrict__ dist,
                                                            const double* __restrict__ inv_dist,
                                                            const double* __restrict__ f_over_c, int n_trials, int A,
                                                            int F, int S, int n_probes, int n_ptiles,
                                                            double* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int pt = (int)(blockIdx.x % (unsigned)n_ptiles), tt = (int)(blockIdx.x / (unsigned)n_ptiles);
  // probes and trials past the end repeat the last one (loads stay in bounds) and store nothing
  int q[QT], t[TT];
#pragma unroll
  for (int i = 0; i < QT; ++i) q[i] = min((pt * (kBeamThreads / 64) + w) * QT + i, n_probes - 1);
#pragma unroll
  for (int j = 0; j < TT; ++j) t[j] = min(tt * TT + j, n_trials - 1);
  const size_t AF = (size_t)A * (size_t)F;
  const double2* __restrict__ Y = cells;
  const double2* __restrict__ X = cells + (size_t)n_trials * AF;
  const int half = S >> 1;
  const double inv_f = 1.0 / (double)F, f_d = (double)F;
  double sums[QT][TT][kBeamFixed];
#pragma unroll
  for (int i = 0; i < QT; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j)
#pragma unroll
      for (int c = 0; c < kBeamFixed; ++c) sums[i][j][c] = 0.0;

  for (int k0 = 0; k0 < F; k0 += 64) {
    const int k = k0 + lane;
    const bool inb = (k >= 1 && k <= half) || k >= F - half;
    const bool any_inb = k0 <= half || k0 + 63 >= F - half;  // the same for the whole wave
    const double foc = f_over_c[k];
    double2 R[QT][TT], U[QT][TT];
#pragma unroll
    for (int i = 0; i < QT; ++i)
#pragma unroll
      for (int j = 0; j < TT; ++j) R[i][j] = U[i][j] = make_double2(0.0, 0.0);
    for (int a = 0; a < A; ++a) {
      double2 y[TT], x[TT];
#pragma unroll
      // (a base that is the same for the whole wave plus the lane: scalar address arithmetic)
      for (int j = 0; j < TT; ++j) y[j] = (Y + (((size_t)t[j] * A + a) * (size_t)F + k0))[lane];
      if (any_inb) {
#pragma unroll
        for (int j = 0; j < TT; ++j)
          x[j] = inb ? (X + (((size_t)t[j] * A + a) * (size_t)F + k0))[lane] : make_double2(0.0, 0.0);
      }
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        const double u = dist[(size_t)q[i] * A + a] * foc;
        const double r = u - rint(u);
        double sn, cs;
        unit_phasor(2.0 * r, sn, cs);
        const double id = inv_dist[(size_t)q[i] * A + a];
        const double gr = cs * id, gi = sn * id;
#pragma unroll
        for (int j = 0; j < TT; ++j) {
          R[i][j].x = fma(gr, y[j].x, fma(-gi, y[j].y, R[i][j].x));
          R[i][j].y = fma(gr, y[j].y, fma(gi, y[j].x, R[i][j].y));
        }
        if (any_inb) {
#pragma unroll
          for (int j = 0; j < TT; ++j) {
            U[i][j].x = fma(gr, x[j].x, fma(-gi, x[j].y, U[i][j].x));
            U[i][j].y = fma(gr, x[j].y, fma(gi, x[j].x, U[i][j].y));
          }
        }
      }
    }
    // the bin's amplitude factor, squared; Y = cell / sqrt(F), X = cell sqrt(F) (powers of two)
    const double wk = kInv4Pi / foc, w2 = wk * wk;
#pragma unroll
    for (int i = 0; i < QT; ++i)
#pragma unroll
      for (int j = 0; j < TT; ++j) {
        const double2 rr = R[i][j];
        const double py = fma(rr.x, rr.x, rr.y * rr.y) * w2 * inv_f;
        sums[i][j][0] += inb ? py : 0.0;
        sums[i][j][1] += inb ? 0.0 : py;
        if (any_inb) {  // (U = 0 in the lanes off band)
          const double2 uu = U[i][j];
          sums[i][j][2] += fma(uu.x, uu.x, uu.y * uu.y) * w2 * f_d;
          sums[i][j][3] += fma(rr.x, uu.x, rr.y * uu.y) * w2;
          sums[i][j][4] += fma(rr.y, uu.x, -(rr.x * uu.y)) * w2;
        }
      }
  }
#pragma unroll
  for (int i = 0; i < QT; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j) {
      const int qi = (pt * (kBeamThreads / 64) + w) * QT + i, tj = tt * TT + j;
#pragma unroll
      for (int c = 0; c < kBeamFixed; ++c) {
        double v = sums[i][j][c];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0 && qi < n_probes && tj < n_trials)
          rows[((size_t)tj * (size_t)n_probes + (size_t)qi) * kBeamFixed + c] = v;
      }
    }
}

}  // namespace

hipError_t launch_beam(hipStream_t st, const double* cells, const double* dist, const double* inv_dist,
                       const double* f_over_c, int n_trials, int n_ant, int n_fft, int n_sub_carr, int n_probes,
                       double* rows) {
  if (n_trials < 1 || n_probes < 1) return hipSuccess;
  const int per_block = (kBeamThreads / 64) * kBeamQT;
  const int n_ptiles = (n_probes + per_block - 1) / per_block;
  const unsigned n_ttiles = (unsigned)((n_trials + kBeamTT - 1) / kBeamTT);
  hipLaunchKernelGGL((beam_kernel<kBeamQT, kBeamTT>), dim3(n_ttiles * (unsigned)n_ptiles), dim3(kBeamThreads), 0, st,
                     reinterpret_cast<const double2*>(cells), dist, inv_dist, f_over_c, n_trials, n_ant, n_fft,
                     n_sub_carr, n_probes, n_ptiles, rows);
  return hipGetLastError();
}

}  // namespace mimo
