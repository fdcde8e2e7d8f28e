// Layered normalised min-sum decoding of QC-LDPC codewords (ldpc.h; the rules stand next to
// mimo_ldpc_code in include/mimo_engine.h).  One workgroup per block of codewords; the lanes are
// the z checks of a layer (base row), so a workgroup has z threads rounded up to whole waves.  The
// a-posteriori values L (int16 per code bit) and the compressed check state (8 B per check: the
// sign mask of its edges, the two smallest scaled magnitudes and which edge holds the smallest)
// live in LDS; global memory is read once per channel value and written once per row cell.
#include "ldpc.h"

#include <algorithm>
#include <tuple>
#include <type_traits>

#include "host_util.h"

namespace mimo {
namespace {

constexpr int kMaxThreads = 512;  // z <= 512

// R of edge e of a check from its compressed state: every edge gets the smallest magnitude of the
// others (r2 for the edge that holds the smallest itself, r1 otherwise), signed by the parity of
// the others' signs.
__device__ __forceinline__ int edge_msg(uint32_t mask, uint32_t mm, int e) {
  const int r1 = (int)(mm & 0xffu), r2 = (int)((mm >> 8) & 0xffu), arg = (int)((mm >> 16) & 0xffu);
  const int mag = e == arg ? r2 : r1;
  const bool neg = ((__popc(mask) ^ (int)(mask >> e)) & 1) != 0;
  return neg ? -mag : mag;
}

// HARD (the turbo mode's instance alone) takes two more arguments, ta = (int8_t* hard, int64_t
// row_stride): the sign of every final L (1 iff L < 0) also goes to hard, where given, at chan's own
// addressing, the block's row is row_stride doubles from the one before, and app is not written.
// Without it the kernel takes no further argument and is the one it was (as the trial kernel's modes:
// an unused argument would move the implicit ones).
template <bool HARD, typename... TA>
__global__ __launch_bounds__(kMaxThreads) void k_ldpc_decode(int z, int n_rows, int n_cols, int n_dec_iters,
                                                            const int32_t* __restrict__ tables,
                                                            const int8_t* __restrict__ chan, int64_t block_stride,
                                                            int n_stride, int n_cw, double* __restrict__ rows,
                                                            int16_t* __restrict__ app, TA... ta) {
  static_assert(std::is_same_v<std::tuple<TA...>, std::conditional_t<HARD, std::tuple<int8_t*, int64_t>, std::tuple<>>>);
  const std::tuple<TA...> turbo(ta...);
  extern __shared__ __attribute__((aligned(8))) unsigned char ldpc_lds[];
  __shared__ int red[kMaxThreads / 64][3];
  const int N = n_cols * z, n_chk = n_rows * z;
  int16_t* L = reinterpret_cast<int16_t*>(ldpc_lds);
  uint2* state = reinterpret_cast<uint2*>(ldpc_lds + (((size_t)N * 2 + 7) & ~size_t(7)));
  const int32_t* row_start = tables;
  const int32_t* edge = tables + n_rows + 1;
  const int t = threadIdx.x, T = blockDim.x;
  const int8_t* cb = chan + (int64_t)blockIdx.x * block_stride;
  int cell_raw = 0, cell_bit = 0, cell_frame = 0, cell_synd = 0;  // thread 0's
  for (int w = 0; w < n_cw; ++w) {
    int raw = 0;
    for (int n = t; n < N; n += T) {
      const int c = cb[(int64_t)n * n_stride + w];
      L[n] = (int16_t)c;
      raw += c < 0;
    }
    for (int k = t; k < n_chk; k += T) state[k] = make_uint2(0u, 0u);
    __syncthreads();
    for (int it = 0; it < n_dec_iters; ++it) {
      for (int r = 0; r < n_rows; ++r) {
        if (t < z) {
          // the checks of a layer touch disjoint bits: a block of a row is a permutation
          const int e0 = row_start[r], ne = row_start[r + 1] - e0;
          const uint2 old = state[r * z + t];
          int m1 = 0x7fffffff, m2 = 0x7fffffff, arg = 0;
          uint32_t mask = 0u;
          for (int e = 0; e < ne; ++e) {
            const int cs = edge[e0 + e];
            int i = t + (cs & 0xffff);
            i = i >= z ? i - z : i;
            const int v = (int)L[(cs >> 16) * z + i] - edge_msg(old.x, old.y, e);
            const int a = v < 0 ? -v : v;
            mask |= (v < 0 ? 1u : 0u) << e;
            if (a < m1) {
              m2 = m1;
              m1 = a;
              arg = e;
            } else if (a < m2) {
              m2 = a;
            }
          }
          const uint32_t r1 = (uint32_t)min(127, (3 * m1) >> 2), r2 = (uint32_t)min(127, (3 * m2) >> 2);
          const uint32_t mm = r1 | (r2 << 8) | ((uint32_t)arg << 16);
          for (int e = 0; e < ne; ++e) {
            const int cs = edge[e0 + e];
            int i = t + (cs & 0xffff);
            i = i >= z ? i - z : i;
            const int n = (cs >> 16) * z + i;
            L[n] = (int16_t)((int)L[n] - edge_msg(old.x, old.y, e) + edge_msg(mask, mm, e));
          }
          state[r * z + t] = make_uint2(mask, mm);
        }
        __syncthreads();  // the next layer reads what this one wrote
      }
    }
    // hard decisions: wrong bits (against the all-zero codeword) and the syndrome
    int nbit = 0, synd = 0;
    for (int n = t; n < N; n += T) {
      const int v = L[n];
      nbit += v < 0;
      if constexpr (!HARD)
        if (app) app[((int64_t)blockIdx.x * n_cw + w) * N + n] = (int16_t)v;
      if constexpr (HARD)
        if (int8_t* hard = std::get<0>(turbo)) hard[(int64_t)blockIdx.x * block_stride + (int64_t)n * n_stride + w] = (int8_t)(v < 0);
    }
    if (t < z)
      for (int r = 0; r < n_rows; ++r) {
        const int e0 = row_start[r], ne = row_start[r + 1] - e0;
        int par = 0;
        for (int e = 0; e < ne; ++e) {
          const int cs = edge[e0 + e];
          int i = t + (cs & 0xffff);
          i = i >= z ? i - z : i;
          par ^= L[(cs >> 16) * z + i] < 0;
        }
        synd += par;
      }
    // fixed order: a shuffle tree per wave, the waves in wave order (integers in any case)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      raw += __shfl_xor(raw, off, 64);
      nbit += __shfl_xor(nbit, off, 64);
      synd += __shfl_xor(synd, off, 64);
    }
    if ((t & 63) == 0) {
      red[t >> 6][0] = raw;
      red[t >> 6][1] = nbit;
      red[t >> 6][2] = synd;
    }
    __syncthreads();
    if (t == 0) {
      int a = 0, b = 0, c = 0;
      for (int v = 0; v < (T >> 6); ++v) {
        a += red[v][0];
        b += red[v][1];
        c += red[v][2];
      }
      cell_raw += a;
      cell_bit += b;
      cell_frame += b > 0;
      cell_synd += c > 0;
    }
    __syncthreads();  // red and L are rewritten by the next codeword
  }
  if (t == 0 && rows) {
    int64_t row_stride = kCodedFixed;
    if constexpr (HARD) row_stride = std::get<1>(turbo);
    double* o = rows + (int64_t)blockIdx.x * row_stride;
    o[0] = (double)cell_raw;
    o[1] = (double)cell_bit;
    o[2] = (double)cell_frame;
    o[3] = (double)cell_synd;
  }
}

}  // namespace

bool ldpc_prepare(const mimo_ldpc_code* code, LdpcHost* out, std::string* err) {
  auto bad = [&](const std::string& m) {
    *err = m;
    return false;
  };
  if (!code) return bad("null code");
  if (code->z < 1 || code->z > 512) return bad("code.z must be in [1, 512]");
  if (code->n_rows < 1 || code->n_rows > 64) return bad("code.n_rows must be in [1, 64]");
  if (code->n_cols < 2 || code->n_cols > 128) return bad("code.n_cols must be in [2, 128]");
  if (code->n_dec_iters < 1 || code->n_dec_iters > 64) return bad("code.n_dec_iters must be in [1, 64]");
  if (!code->shifts) return bad("null code.shifts");
  const int z = code->z, nr = code->n_rows, nc = code->n_cols;
  std::vector<int> col_w(nc, 0);
  out->tables.assign(nr + 1, 0);
  for (int r = 0; r < nr; ++r) {
    int w = 0;
    for (int c = 0; c < nc; ++c) {
      const int s = code->shifts[(size_t)r * nc + c];
      if (s < -1 || s >= z)
        return bad("code.shifts[" + std::to_string(r) + "][" + std::to_string(c) + "] must be -1 or in [0, z)");
      if (s < 0) continue;
      ++w;
      ++col_w[c];
      out->tables.push_back((c << 16) | s);
    }
    if (w < 2 || w > 32) return bad("code.shifts: base row " + std::to_string(r) + " must have weight 2 ... 32");
    out->tables[r + 1] = out->tables[r] + w;
  }
  for (int c = 0; c < nc; ++c)
    if (col_w[c] < 1) return bad("code.shifts: base column " + std::to_string(c) + " must have weight >= 1");
  out->z = z;
  out->n_rows = nr;
  out->n_cols = nc;
  out->n_dec_iters = code->n_dec_iters;
  out->lds_bytes = (((size_t)nc * z * 2 + 7) & ~size_t(7)) + (size_t)nr * z * 8;
  // (the kernel's static LDS, the wave sums of its reduction, on top)
  const size_t need = out->lds_bytes + sizeof(int) * (kMaxThreads / 64) * 3;
  if (need > kLdpcLdsBytes)
    return bad("code: the decoder state (2 B per code bit + 8 B per check = " + std::to_string(need) +
               " B) does not fit the " + std::to_string(kLdpcLdsBytes) + " B of LDS of one workgroup");
  return true;
}

hipError_t launch_ldpc(hipStream_t st, const LdpcHost& code, const int32_t* tables, const int8_t* chan,
                       int64_t n_blocks, int64_t block_stride, int n_stride, int n_cw, double* rows, int16_t* app,
                       int8_t* hard, int64_t row_stride) {
  if (n_blocks <= 0 || n_cw <= 0) return hipSuccess;
  const int threads = std::min(kMaxThreads, (code.z + 63) & ~63);
  auto go = [&](auto* kern, auto... ta) {
    const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)code.lds_bytes);
    if (ae != hipSuccess) return ae;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_blocks), dim3(threads), code.lds_bytes, st, code.z, code.n_rows, code.n_cols,
                       code.n_dec_iters, tables, chan, block_stride, n_stride, n_cw, rows, app, ta...);
    return hipGetLastError();
  };
  if (hard || row_stride != kCodedFixed) return go(&k_ldpc_decode<true, int8_t*, int64_t>, hard, row_stride);
  return go(&k_ldpc_decode<false>);
}

}  // namespace mimo

using mimo::fail;

extern "C" int32_t mimo_ldpc_decode(const mimo_ldpc_code* code, const int8_t* chan, int64_t n_cw, int16_t* app_out) {
  mimo::LdpcHost h;
  std::string err;
  if (!mimo::ldpc_prepare(code, &h, &err)) return fail(MIMO_EINVAL, err);
  if (n_cw < 0) return fail(MIMO_EINVAL, "n_cw must be >= 0");
  if (n_cw == 0) return MIMO_OK;
  if (!chan || !app_out) return fail(MIMO_EINVAL, "null chan or app_out");
  const int64_t N = h.n_bits();
  if (n_cw > (int64_t)0x7fffffff) return fail(MIMO_EINVAL, "n_cw must be below 2^31");
  for (int64_t i = 0; i < n_cw * N; ++i)
    if (chan[i] < -63 || chan[i] > 63)
      return fail(MIMO_EINVAL, "chan[" + std::to_string(i) + "] must be in [-63, 63]");
  mimo::DBuf dt, dc, da;
  MIMO_HIP_TRY(dt.alloc(h.tables.size() * sizeof(int32_t)));
  MIMO_HIP_TRY(dc.alloc((size_t)(n_cw * N)));
  MIMO_HIP_TRY(da.alloc((size_t)(n_cw * N) * sizeof(int16_t)));
  MIMO_HIP_TRY(hipMemcpy(dt.p, h.tables.data(), h.tables.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  MIMO_HIP_TRY(hipMemcpy(dc.p, chan, (size_t)(n_cw * N), hipMemcpyHostToDevice));
  MIMO_HIP_TRY(mimo::launch_ldpc(nullptr, h, static_cast<const int32_t*>(dt.p), static_cast<const int8_t*>(dc.p),
                                 n_cw, N, 1, 1, nullptr, static_cast<int16_t*>(da.p)));
  MIMO_HIP_TRY(hipMemcpy(app_out, da.p, (size_t)(n_cw * N) * sizeof(int16_t), hipMemcpyDeviceToHost));
  return MIMO_OK;
}
