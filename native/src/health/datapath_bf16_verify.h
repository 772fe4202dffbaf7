// The verdict of the bf16 MFMA datapath check: what the host decides from the
// records and tiles mi355x_mfma_datapath_bf16 wrote (shared by hsa_chip.cpp and
// native/tests/datapath_bf16_contract_cli.cpp). Host only, no HSA: the caller
// owns the dispatch and hands over plain memory.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "datapath_bf16_kernel.h"
#include "datapath_verdict_common.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

inline float dpbf_as_float(uint32_t w) {
  float f;
  std::memcpy(&f, &w, sizeof(f));
  return f;
}

inline uint32_t dpbf_as_word(float f) {
  uint32_t w;
  std::memcpy(&w, &f, sizeof(w));
  return w;
}

// The tile a wave with nonce `nw` computes in `stage`, as words (1024 for
// stages 0..3, 256 for stage 4). Plain float arithmetic in k order: every
// product and every partial sum is exact for these operands
// (datapath_bf16_kernel.h), so neither the order nor a fused multiply-add
// changes a bit.
inline void datapath_bf16_expected_tile(uint32_t stage, uint32_t nw, uint32_t* want) {
  const uint32_t dim = dpbf_dim(stage), words = dpbf_blocks(stage) * 4;
  float a[32][32], b[32][32];
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t w = 0; w < words; ++w) {
      const uint32_t aw = dpbf_a_word(stage, i, w >> 2, w & 3, nw);
      const uint32_t bw = dpbf_b_word(stage, i, w >> 2, w & 3, nw);
      for (uint32_t e = 0; e < 2; ++e) {
        a[i][2 * w + e] = dpbf_as_float(dpbf_widen(aw, e));
        b[i][2 * w + e] = dpbf_as_float(dpbf_widen(bw, e));
      }
    }
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t j = 0; j < dim; ++j) {
      float d = dpbf_as_float(dpbf_c_word(stage, i, j, nw));
      for (uint32_t k = 0; k < 2 * words; ++k) d = d + a[i][k] * b[j][k];
      want[i * dim + j] = dpbf_as_word(d);
    }
}

MI355X_DP_SQUARE_TRAITS(DatapathBf16Traits, datapath_bf16, DPBF, dpbf, "datapath bf16 check");

// `records`: grid * MI355X_DPBF_REC_WORDS words, `tiles`: grid * MI355X_DPBF_WG_WORDS words, as
// mi355x_mfma_datapath_bf16 left them (datapath_verdict_common.h).
inline void datapath_bf16_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid,
                                  mi355x_datapath_bf16_result* out) {
  datapath_register_verdict<DatapathBf16Traits>(records, tiles, grid, out);
}

}  // namespace mi355x
