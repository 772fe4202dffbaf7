// The verdict of the f64 MFMA datapath check: what the host decides from the
// records and tiles mi355x_mfma_datapath_f64 wrote (shared by hsa_chip.cpp and
// native/tests/datapath_f64_contract_cli.cpp). Host only, no HSA and no
// floating point: the caller owns the dispatch and hands over plain memory.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "datapath_f64_kernel.h"
#include "datapath_verdict_common.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

// a double's bit pattern as v * 2^e with v odd (or v = 0): the recipe holds
// only normals and +0
inline void dpd_decode(uint64_t bits, int64_t* v, int32_t* e) {
  *v = 0;
  *e = 0;
  if ((bits << 1) == 0) return;
  uint64_t sig = (1ull << 52) | (bits & 0xFFFFFFFFFFFFFull);
  const int tz = __builtin_ctzll(sig);
  sig >>= tz;
  *v = (bits >> 63) ? -static_cast<int64_t>(sig) : static_cast<int64_t>(sig);
  *e = static_cast<int32_t>((bits >> 52) & 0x7FFu) - 1075 + tz;
}

// The tile `t` a wave with nonce `nw` computes in `stage`, as words (low word
// of a double first): 512 for the 16x16 stages, 128 for stages 5 and 6. Integer
// arithmetic only: each product is a 64-bit product of two odd significands
// (at most 53 bits for these operands), the terms of an output are brought to
// their smallest exponent (they share one by construction) and summed in an
// int64_t, and the sum is normalised into a double's bit pattern.
inline void datapath_f64_expected_tile(uint32_t stage, uint32_t t, uint32_t nw, uint32_t* want) {
  for (uint32_t d = 0; d < dpd_tile_doubles(stage); ++d) {
    const uint32_t row = dpd_row_of(stage, d), col = dpd_col_of(stage, d);
    int64_t v[5];
    int32_t e[5];
    dpd_decode(dpd_c_bits(stage, row, col, nw) ^ dpd_neg_c(stage, t), &v[4], &e[4]);
    for (uint32_t k = 0; k < 4; ++k) {
      int64_t va, vb;
      int32_t ea, eb;
      dpd_decode(dpd_a_bits(stage, t, row, k, nw) ^ dpd_neg_ab(stage, t), &va, &ea);
      dpd_decode(dpd_b_bits(stage, t, col, k, nw), &vb, &eb);
      v[k] = va * vb;
      e[k] = ea + eb;
    }
    int32_t emin = INT32_MAX;
    for (int i = 0; i < 5; ++i)
      if (v[i] != 0) emin = std::min(emin, e[i]);
    int64_t sum = 0;
    for (int i = 0; i < 5; ++i)
      if (v[i] != 0) sum += v[i] * (int64_t{1} << (e[i] - emin));
    const uint64_t bits = dpd_scaled_int(sum, emin);  // never zero (datapath_f64_kernel.h)
    want[2 * d] = static_cast<uint32_t>(bits);
    want[2 * d + 1] = static_cast<uint32_t>(bits >> 32);
  }
}

MI355X_DP_ASSERT_RECORD(MI355X_DPDREC);
// twelve tiles in seven stages: a stage holds dpd_tiles(stage) tiles, 16x16 or 4x4 doubles each; a word of a
// stage is numbered over all its tiles
struct DatapathF64Traits {
  using Result = mi355x_datapath_f64_result;
  using Args = mi355x_datapath_f64_args;
  static constexpr const char* kKind = "datapath_f64";
  static constexpr const char* kSymbol = "mi355x_mfma_datapath_f64.kd";
  static constexpr const char* kDispatch = "datapath f64 check";
  static constexpr uint32_t kMagic = MI355X_DPD_MAGIC, kRecWords = MI355X_DPD_REC_WORDS,
                            kWgWords = MI355X_DPD_WG_WORDS, kThreads = MI355X_DPD_THREADS,
                            kStages = MI355X_DPD_STAGES, kTileWords = MI355X_DPD_TILE;
  static uint32_t wave_nonce(uint32_t nonce, uint32_t wg) { return dpd_wave_nonce(nonce, wg, 0); }
  static uint32_t tile_offset(uint32_t stage) { return dpd_tile_offset(stage); }
  static uint32_t tiles(uint32_t stage) { return dpd_tiles(stage); }
  static uint32_t tile_words(uint32_t stage) { return dpd_tile_doubles(stage) * 2; }
  static void expected_tile(uint32_t stage, uint32_t t, uint32_t nw, uint32_t* want) {
    datapath_f64_expected_tile(stage, t, nw, want);
  }
};

// `records`: grid * MI355X_DPD_REC_WORDS words, `tiles`: grid * MI355X_DPD_WG_WORDS words, as
// mi355x_mfma_datapath_f64 left them (datapath_verdict_common.h).
inline void datapath_f64_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid,
                                 mi355x_datapath_f64_result* out) {
  datapath_register_verdict<DatapathF64Traits>(records, tiles, grid, out);
}

}  // namespace mi355x
