// The verdict of the fp6 / fp4 MX-scaled MFMA datapath check: what the host decides
// from the records and tiles mi355x_mfma_datapath_f6f4 wrote (shared by
// hsa_chip.cpp and native/tests/datapath_f6f4_contract_cli.cpp). Host only, no
// HSA: the caller owns the dispatch and hands over plain memory.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "datapath_f6f4_kernel.h"
#include "datapath_verdict_common.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

inline float dpf6_as_float(uint32_t w) {
  float f;
  std::memcpy(&f, &w, sizeof(f));
  return f;
}

inline uint32_t dpf6_as_word(float f) {
  uint32_t w;
  std::memcpy(&w, &f, sizeof(w));
  return w;
}

// The tile a wave with nonce `nw` computes in `stage`, as words (1024, or 256
// for stages 3 and 7). Plain float arithmetic in k order on the recipe's codes
// (dpf6_elem, placed by dpf6_k: the packing into dwords plays no part here),
// decoded by integer arithmetic (dpf6_decode) and scaled by exact powers of
// two: every product and every partial sum is exact for these operands
// (datapath_f6f4_kernel.h), so neither the order nor a fused multiply-add
// changes a bit.
inline void datapath_f6f4_expected_tile(uint32_t stage, uint32_t nw, uint32_t* want) {
  const uint32_t dim = dpf6_dim(stage), groups = dpf6_groups(stage), depth = groups * 32;
  const uint32_t fa = dpf6_fmt(stage, 0), fb = dpf6_fmt(stage, 1);
  static thread_local float a[32][128], b[32][128];
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t h = 0; h < groups; ++h)
      for (uint32_t e = 0; e < 32; ++e) {
        const uint32_t ka = dpf6_k(stage, fa, h, e), kb = dpf6_k(stage, fb, h, e);
        a[i][ka] = dpf6_as_float(dpf6_decode(dpf6_elem(stage, 0, i, h, e, nw), fa)) *
                   dpf6_as_float(dpf6_scale_f32(dpf6_scale_byte(nw, stage, 0, i, ka >> 5)));
        b[i][kb] = dpf6_as_float(dpf6_decode(dpf6_elem(stage, 1, i, h, e, nw), fb)) *
                   dpf6_as_float(dpf6_scale_f32(dpf6_scale_byte(nw, stage, 1, i, kb >> 5)));
      }
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t j = 0; j < dim; ++j) {
      float d = dpf6_as_float(dpf6_c_word(stage, i, j, nw));
      for (uint32_t k = 0; k < depth; ++k) d = d + a[i][k] * b[j][k];
      want[i * dim + j] = dpf6_as_word(d);
    }
}

MI355X_DP_SQUARE_TRAITS(DatapathF6f4Traits, datapath_f6f4, DPF6, dpf6, "datapath f6f4 check");

// `records`: grid * MI355X_DPF6_REC_WORDS words, `tiles`: grid * MI355X_DPF6_WG_WORDS words, as
// mi355x_mfma_datapath_f6f4 left them (datapath_verdict_common.h).
inline void datapath_f6f4_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid,
                                 mi355x_datapath_f6f4_result* out) {
  datapath_register_verdict<DatapathF6f4Traits>(records, tiles, grid, out);
}

}  // namespace mi355x
