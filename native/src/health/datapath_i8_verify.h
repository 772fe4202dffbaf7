// The verdict of the int8 MFMA datapath check: what the host decides from the
// records and tiles mi355x_mfma_datapath_i8 wrote (shared by hsa_chip.cpp and
// native/tests/datapath_i8_contract_cli.cpp). Host only, no HSA: the caller
// owns the dispatch and hands over plain memory.
#pragma once

#include <cstdint>

#include "datapath_i8_kernel.h"
#include "datapath_verdict_common.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

// The tile a wave with nonce `nw` computes in `stage`, as words (1024 for
// stages 0..3, 256 for stage 4). Plain int32 arithmetic: no stage can overflow
// (datapath_i8_kernel.h), so the order of the sum does not matter.
inline void datapath_i8_expected_tile(uint32_t stage, uint32_t nw, uint32_t* want) {
  const uint32_t dim = dpi8_dim(stage), words = dpi8_blocks(stage) * 4;
  uint32_t a[32][16], b[32][16];
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t w = 0; w < words; ++w) {
      a[i][w] = dpi8_a_word(stage, i, w >> 2, w & 3, nw);
      b[i][w] = dpi8_b_word(stage, i, w >> 2, w & 3, nw);
    }
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t j = 0; j < dim; ++j) {
      int32_t d = static_cast<int32_t>(dpi8_c_word(stage, i, j, nw));
      for (uint32_t w = 0; w < words; ++w) d = dpi8_dot4(a[i][w], b[j][w], d);
      want[i * dim + j] = static_cast<uint32_t>(d);
    }
}

MI355X_DP_SQUARE_TRAITS(DatapathI8Traits, datapath_i8, DPI8, dpi8, "datapath i8 check");

// `records`: grid * MI355X_DPI8_REC_WORDS words, `tiles`: grid * MI355X_DPI8_WG_WORDS words, as
// mi355x_mfma_datapath_i8 left them (datapath_verdict_common.h).
inline void datapath_i8_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid,
                                mi355x_datapath_i8_result* out) {
  datapath_register_verdict<DatapathI8Traits>(records, tiles, grid, out);
}

}  // namespace mi355x
