// The LDPC decoder of the coded mode (ldpc.hip; include/mimo_engine.h mimo_engine_coded_points,
// mimo_ldpc_decode): layered normalised min-sum on a QC-LDPC code given by its base matrix.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mimo_engine.h"

namespace mimo {

constexpr int kCodedFixed = 4;                 // MIMO_CODED_FIXED
constexpr size_t kLdpcLdsBytes = 160u << 10;   // the LDS one workgroup may hold on gfx950

// A checked code and its host tables: the per-row edge lists (the shift table without its zero
// blocks), as the kernel reads them.
struct LdpcHost {
  int z = 0, n_rows = 0, n_cols = 0, n_dec_iters = 0;
  // tables = row_start [n_rows + 1] | edge [row_start[n_rows]]: edge = (base column << 16) | shift,
  // the edges of a row in ascending column order
  std::vector<int32_t> tables;
  size_t lds_bytes = 0;  // of one workgroup: L (int16 per code bit) + 8 B of check state per check
  int n_bits() const { return n_cols * z; }
};

// Checks every rule of include/mimo_engine.h's mimo_ldpc_code (host only) and fills the tables.
// -> true, or false with the message that names the field.
bool ldpc_prepare(const mimo_ldpc_code* code, LdpcHost* out, std::string* err);

// Decodes n_blocks * n_cw codewords, one workgroup per block, its n_cw codewords one after the other:
// bit n of codeword w of block b is chan[b * block_stride + n * n_stride + w] (the coded mode:
// block = (trial, counter index), block_stride = S log2 M, n_stride = n_cw; the seam: one codeword
// per block, n_stride = 1).
//  rows  null, or [n_blocks][kCodedFixed]: over the block's codewords the number of chan < 0, of
//        L < 0 after decoding, of codewords with any L < 0 and of codewords whose hard decision
//        has a non-zero syndrome.  Every cell written once, by plain stores; integer sums.
//  app   null, or [n_blocks][n_cw][N] int16: the final L.
//  tables the device copy of LdpcHost::tables.
//  hard  null, or the decisions at chan's own addressing (the turbo mode): 1 where the final L < 0,
//        else 0 (L = 0 counts as non-negative), one int8 per decoded bit; the stores coalesce like
//        chan's loads.
//  row_stride  doubles between the rows of two blocks (the turbo mode: a trial's passes side by side).
//        With hard or a row_stride of its own a second kernel of the same decoder runs, which writes
//        no app; without either, the kernel of the coded mode.
hipError_t launch_ldpc(hipStream_t st, const LdpcHost& code, const int32_t* tables, const int8_t* chan,
                       int64_t n_blocks, int64_t block_stride, int n_stride, int n_cw, double* rows, int16_t* app,
                       int8_t* hard = nullptr, int64_t row_stride = kCodedFixed);

}  // namespace mimo
