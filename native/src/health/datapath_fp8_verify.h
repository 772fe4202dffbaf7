// The verdict of the fp8 / MX-scaled MFMA datapath check: what the host decides
// from the records and tiles mi355x_mfma_datapath_fp8 wrote (shared by
// hsa_chip.cpp and native/tests/datapath_fp8_contract_cli.cpp). Host only, no
// HSA: the caller owns the dispatch and hands over plain memory.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "datapath_fp8_kernel.h"
#include "datapath_verdict_common.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

inline float dpf8_as_float(uint32_t w) {
  float f;
  std::memcpy(&f, &w, sizeof(f));
  return f;
}

inline uint32_t dpf8_as_word(float f) {
  uint32_t w;
  std::memcpy(&w, &f, sizeof(w));
  return w;
}

// The tile a wave with nonce `nw` computes in `stage`, as words (1024, or 256
// for stages 3 and 7). Plain float arithmetic in k order on operands decoded
// by integer arithmetic (dpf8_decode) and scaled by exact powers of two: every
// product and every partial sum is exact for these operands
// (datapath_fp8_kernel.h), so neither the order nor a fused multiply-add
// changes a bit.
inline void datapath_fp8_expected_tile(uint32_t stage, uint32_t nw, uint32_t* want) {
  const uint32_t dim = dpf8_dim(stage), blocks = dpf8_blocks(stage), dwords = dpf8_dwords(stage);
  const uint32_t depth = blocks * dwords * 4;
  const uint32_t fa = dpf8_fmt_a(stage), fb = dpf8_fmt_b(stage);
  static thread_local float a[32][128], b[32][128];
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t h = 0; h < blocks; ++h) {
      for (uint32_t d = 0; d < dwords; ++d) {
        float sa = 1.0f, sb = 1.0f;
        if (dpf8_scaled(stage)) {  // the scale of the bytes' scale block, which is not the lane group's own
          const uint32_t g = dpf8_scale_block(stage, h, d);
          sa = dpf8_as_float(dpf8_scale_f32(dpf8_scale_byte(nw, stage, 0, i, g)));
          sb = dpf8_as_float(dpf8_scale_f32(dpf8_scale_byte(nw, stage, 1, i, g)));
        }
        const uint32_t aw = dpf8_a_word(stage, i, h, d, nw);
        const uint32_t bw = dpf8_b_word(stage, i, h, d, nw);
        for (uint32_t e = 0; e < 4; ++e) {
          const uint32_t k = (h * dwords + d) * 4 + e;
          a[i][k] = dpf8_as_float(dpf8_decode((aw >> (8 * e)) & 0xFFu, fa)) * sa;
          b[i][k] = dpf8_as_float(dpf8_decode((bw >> (8 * e)) & 0xFFu, fb)) * sb;
        }
      }
    }
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t j = 0; j < dim; ++j) {
      float d = dpf8_as_float(dpf8_c_word(stage, i, j, nw));
      for (uint32_t k = 0; k < depth; ++k) d = d + a[i][k] * b[j][k];
      want[i * dim + j] = dpf8_as_word(d);
    }
}

MI355X_DP_SQUARE_TRAITS(DatapathFp8Traits, datapath_fp8, DPF8, dpf8, "datapath fp8 check");

// `records`: grid * MI355X_DPF8_REC_WORDS words, `tiles`: grid * MI355X_DPF8_WG_WORDS words, as
// mi355x_mfma_datapath_fp8 left them (datapath_verdict_common.h).
inline void datapath_fp8_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid,
                                 mi355x_datapath_fp8_result* out) {
  datapath_register_verdict<DatapathFp8Traits>(records, tiles, grid, out);
}

}  // namespace mi355x
