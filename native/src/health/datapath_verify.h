// The verdict of the MFMA datapath check: what the host decides from the
// records and tiles mi355x_mfma_datapath wrote (shared by hsa_chip.cpp and
// native/tests/datapath_contract_cli.cpp). Host only, no HSA: the caller owns
// the dispatch and hands over plain memory.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "datapath_kernel.h"
#include "datapath_verdict_common.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

// The tile a wave with nonce `nw` computes in `stage`, as words. Plain float
// arithmetic in k order: every product and partial sum is exact by
// construction (datapath_kernel.h), so no fma is needed.
inline void datapath_expected_tile(uint32_t stage, uint32_t nw, uint32_t* want) {
  float a[MI355X_DP_M][MI355X_DP_K], b[MI355X_DP_K][MI355X_DP_N];
  for (uint32_t i = 0; i < MI355X_DP_M; ++i)
    for (uint32_t k = 0; k < MI355X_DP_K; ++k) a[i][k] = dp_as_float(dp_a_word(stage, i, k, nw));
  for (uint32_t k = 0; k < MI355X_DP_K; ++k)
    for (uint32_t j = 0; j < MI355X_DP_N; ++j) b[k][j] = dp_as_float(dp_b_word(stage, k, j, nw));
  for (uint32_t i = 0; i < MI355X_DP_M; ++i)
    for (uint32_t j = 0; j < MI355X_DP_N; ++j) {
      float d = dp_as_float(dp_c_word(stage, i, j, nw));
      for (uint32_t k = 0; k < MI355X_DP_K; ++k) d += a[i][k] * b[k][j];
      want[i * MI355X_DP_N + j] = dp_as_word(d);
    }
}

MI355X_DP_ASSERT_RECORD(MI355X_DPREC);
// four stages of one 32x32 tile each
struct DatapathF32Traits {
  using Result = mi355x_datapath_result;
  using Args = mi355x_datapath_args;
  static constexpr const char* kKind = "datapath";
  static constexpr const char* kSymbol = "mi355x_mfma_datapath.kd";
  static constexpr const char* kDispatch = "datapath check";
  static constexpr uint32_t kMagic = MI355X_DP_MAGIC, kRecWords = MI355X_DP_REC_WORDS, kWgWords = MI355X_DP_WG_WORDS,
                            kThreads = MI355X_DP_THREADS, kStages = MI355X_DP_STAGES, kTileWords = MI355X_DP_TILE;
  static uint32_t wave_nonce(uint32_t nonce, uint32_t wg) { return dp_wave_nonce(nonce, wg, 0); }
  static uint32_t tile_offset(uint32_t stage) { return stage * MI355X_DP_TILE; }
  static uint32_t tiles(uint32_t) { return 1; }
  static uint32_t tile_words(uint32_t) { return MI355X_DP_TILE; }
  static void expected_tile(uint32_t stage, uint32_t, uint32_t nw, uint32_t* want) {
    datapath_expected_tile(stage, nw, want);
  }
};

// `records`: grid * MI355X_DP_REC_WORDS words, `tiles`: grid * MI355X_DP_WG_WORDS words, as
// mi355x_mfma_datapath left them (datapath_verdict_common.h).
inline void datapath_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid,
                             mi355x_datapath_result* out) {
  datapath_register_verdict<DatapathF32Traits>(records, tiles, grid, out);
}

}  // namespace mi355x
