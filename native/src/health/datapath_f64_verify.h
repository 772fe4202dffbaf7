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

// `records`: grid * MI355X_DPD_REC_WORDS words, `tiles`: grid *
// MI355X_DPD_WG_WORDS words, as mi355x_mfma_datapath_f64 left them. The
// caller has set out->nonce; every verdict field must be zero.
inline void datapath_f64_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid,
                                 mi355x_datapath_f64_result* out) {
  const uint32_t nonce = out->nonce;
  std::vector<uint32_t> cu_keys, simd_keys;
  cu_keys.reserve(grid);
  simd_keys.reserve(static_cast<size_t>(grid) * 4);
  uint32_t xmask = 0;
  out->first_bad_wg = out->first_bad_stage = out->first_bad_word = -1;
  for (uint32_t w = 0; w < grid; ++w) {
    const uint32_t* r = records + static_cast<size_t>(w) * MI355X_DPD_REC_WORDS;
    const bool present = r[MI355X_DPDREC_MAGIC] == MI355X_DPD_MAGIC && r[MI355X_DPDREC_WG] == w &&
                         r[MI355X_DPDREC_NONCE] == (nonce ^ w);
    if (!present) continue;
    uint32_t dev_bad = 0;
    for (int s = 0; s < MI355X_DPD_STAGES; ++s) {
      out->stage_bad[s] += r[MI355X_DPDREC_BAD + s];
      dev_bad += r[MI355X_DPDREC_BAD + s];
    }
    out->mfma_bad += dev_bad;
    const uint32_t x = r[MI355X_DPDREC_XCC] & 0xF;
    xmask |= 1u << x;
    cu_keys.push_back((x << 16) | ((r[MI355X_DPDREC_HWID] >> 8) & 0xFF));
    for (int v = 0; v < MI355X_DPD_THREADS / 64; ++v) {
      const uint32_t h = r[MI355X_DPDREC_HWID + v];
      simd_keys.push_back((x << 16) | (((h >> 8) & 0xFF) << 2) | ((h >> 4) & 0x3));
    }
    // wave 0's twelve tiles against the host reference
    const uint32_t nw = dpd_wave_nonce(nonce, w, 0);
    const uint32_t* tile = tiles + static_cast<size_t>(w) * MI355X_DPD_WG_WORDS;
    uint32_t tb = 0;
    uint32_t expect[MI355X_DPD_TILE];
    for (uint32_t s = 0; s < MI355X_DPD_STAGES; ++s) {
      const uint32_t words = dpd_tile_doubles(s) * 2;
      for (uint32_t t = 0; t < dpd_tiles(s); ++t) {
        datapath_f64_expected_tile(s, t, nw, expect);
        for (uint32_t k = 0; k < words; ++k) {
          const uint32_t got = tile[dpd_tile_offset(s) + t * words + k];
          const uint32_t want = expect[k];
          if (got == want) continue;
          ++tb;
          if (out->first_bad_wg < 0) {
            out->first_bad_wg = static_cast<int>(w);
            out->first_bad_stage = static_cast<int>(s);
            out->first_bad_word = static_cast<int>(t * words + k);
            out->first_bad_got = got;
            out->first_bad_want = want;
            out->first_bad_xor = got ^ want;
          }
        }
      }
    }
    out->tile_bad += tb;
    if (dev_bad == 0 && tb == 0) ++out->records_ok;
  }
  std::sort(cu_keys.begin(), cu_keys.end());
  out->cus_covered = static_cast<int>(std::unique(cu_keys.begin(), cu_keys.end()) - cu_keys.begin());
  std::sort(simd_keys.begin(), simd_keys.end());
  out->simds_covered = static_cast<int>(std::unique(simd_keys.begin(), simd_keys.end()) - simd_keys.begin());
  out->xccs_covered = __builtin_popcount(xmask);
  out->ok = out->records_ok == static_cast<int>(grid);
  if (out->ok) return;
  int n = std::snprintf(out->error, sizeof(out->error), "%d/%u workgroups exact (device_bad=%u tile_bad=%u)",
                        out->records_ok, grid, out->mfma_bad, out->tile_bad);
  if (out->first_bad_wg >= 0 && n > 0 && n < static_cast<int>(sizeof(out->error))) {
    const uint32_t x = out->first_bad_xor;
    n += std::snprintf(out->error + n, sizeof(out->error) - n, "; first bad: wg %d stage %d word %d xor 0x%08x",
                       out->first_bad_wg, out->first_bad_stage, out->first_bad_word, x);
    if ((x & (x - 1)) == 0 && n < static_cast<int>(sizeof(out->error)))
      std::snprintf(out->error + n, sizeof(out->error) - n, " (bit %d)", __builtin_ctz(x));
  }
}

}  // namespace mi355x
