// The verdict of the sparse (2:4) MFMA datapath check: what the host decides
// from the records and tiles mi355x_mfma_datapath_sparse wrote (shared by
// hsa_chip.cpp and native/tests/datapath_sparse_contract_cli.cpp). Host only, no
// HSA: the caller owns the dispatch and hands over plain memory.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "datapath_sparse_kernel.h"
#include "datapath_verdict_common.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

// The tile a wave with nonce `nw` computes in `stage`, as words (1024, or 256
// for stages 4, 6 and 8): what dpsp_expected gives per element, with the
// operands generated once per tile instead of once per output. A's compressed
// elements keep their order and carry the k their index field names; B is laid
// out by k. Every product and every partial sum is exact for these operands
// (datapath_sparse_kernel.h), so neither the order nor a fused multiply-add
// changes a bit.
inline void datapath_sparse_expected_tile(uint32_t stage, uint32_t nw, uint32_t* want) {
  const uint32_t dim = dpsp_dim(stage), groups = dpsp_groups(stage), per = dpsp_per(stage), kb = dpsp_kb(stage);
  const uint32_t terms = groups * 4 * per;  // compressed elements of a row
  const bool i8 = dpsp_kind(stage) == MI355X_DPSP_I8;
  static thread_local uint32_t a[32][64], ak[32][64], b[32][128];  // element values (f32 words or int8) and A's k
  for (uint32_t rc = 0; rc < dim; ++rc)
    for (uint32_t h = 0; h < groups; ++h) {
      const uint32_t idx = dpsp_index_bits(stage, rc, h, nw);
      for (uint32_t d = 0; d < 8; ++d) {
        const uint32_t aw = d < 4 ? dpsp_a_word(stage, rc, h, d, nw) : 0u, bw = dpsp_b_word(stage, rc, h, d, nw);
        for (uint32_t x = 0; x < per; ++x) {
          const uint32_t e = d * per + x;
          b[rc][kb * h + e] = i8 ? static_cast<uint32_t>(static_cast<int8_t>(bw >> (8 * x))) : dpsp_widen(stage, 1, bw, x);
          if (d >= 4) continue;
          a[rc][h * 4 * per + e] = i8 ? static_cast<uint32_t>(static_cast<int8_t>(aw >> (8 * x))) : dpsp_widen(stage, 0, aw, x);
          ak[rc][h * 4 * per + e] = dpsp_k_of(stage, h, 4 * (e >> 1) + ((idx >> (2 * e)) & 3));
        }
      }
    }
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t j = 0; j < dim; ++j) {
      uint32_t c = dpsp_c_word(stage, i, j, nw);
      if (i8) {
        for (uint32_t n = 0; n < terms; ++n) c += static_cast<uint32_t>(static_cast<int32_t>(a[i][n]) * static_cast<int32_t>(b[j][ak[i][n]]));
      } else {
        float s, x, y;
        std::memcpy(&s, &c, sizeof(s));
        for (uint32_t n = 0; n < terms; ++n) {
          std::memcpy(&x, &a[i][n], sizeof(x));
          std::memcpy(&y, &b[j][ak[i][n]], sizeof(y));
          s = s + x * y;
        }
        std::memcpy(&c, &s, sizeof(c));
      }
      want[i * dim + j] = c;
    }
}

MI355X_DP_SQUARE_TRAITS(DatapathSparseTraits, datapath_sparse, DPSP, dpsp, "datapath sparse check");

// `records`: grid * MI355X_DPSP_REC_WORDS words, `tiles`: grid * MI355X_DPSP_WG_WORDS words, as
// mi355x_mfma_datapath_sparse left them (datapath_verdict_common.h).
inline void datapath_sparse_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid,
                                    mi355x_datapath_sparse_result* out) {
  datapath_register_verdict<DatapathSparseTraits>(records, tiles, grid, out);
}

}  // namespace mi355x
