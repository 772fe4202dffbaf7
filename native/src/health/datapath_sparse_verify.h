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

// `records`: grid * MI355X_DPSP_REC_WORDS words, `tiles`: grid *
// MI355X_DPSP_WG_WORDS words, as mi355x_mfma_datapath_sparse left them. The
// caller has set out->nonce; every verdict field must be zero.
inline void datapath_sparse_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid,
                                    mi355x_datapath_sparse_result* out) {
  const uint32_t nonce = out->nonce;
  std::vector<uint32_t> cu_keys, simd_keys;
  cu_keys.reserve(grid);
  simd_keys.reserve(static_cast<size_t>(grid) * 4);
  uint32_t xmask = 0;
  out->first_bad_wg = out->first_bad_stage = out->first_bad_word = -1;
  for (uint32_t w = 0; w < grid; ++w) {
    const uint32_t* r = records + static_cast<size_t>(w) * MI355X_DPSP_REC_WORDS;
    const bool present = r[MI355X_DPSPREC_MAGIC] == MI355X_DPSP_MAGIC && r[MI355X_DPSPREC_WG] == w &&
                         r[MI355X_DPSPREC_NONCE] == (nonce ^ w);
    if (!present) continue;
    uint32_t dev_bad = 0;
    for (int s = 0; s < MI355X_DPSP_STAGES; ++s) {
      out->stage_bad[s] += r[MI355X_DPSPREC_BAD + s];
      dev_bad += r[MI355X_DPSPREC_BAD + s];
    }
    out->mfma_bad += dev_bad;
    const uint32_t x = r[MI355X_DPSPREC_XCC] & 0xF;
    xmask |= 1u << x;
    cu_keys.push_back((x << 16) | ((r[MI355X_DPSPREC_HWID] >> 8) & 0xFF));
    for (int v = 0; v < MI355X_DPSP_THREADS / 64; ++v) {
      const uint32_t h = r[MI355X_DPSPREC_HWID + v];
      simd_keys.push_back((x << 16) | (((h >> 8) & 0xFF) << 2) | ((h >> 4) & 0x3));
    }
    // wave 0's ten tiles against the host reference
    const uint32_t nw = dpsp_wave_nonce(nonce, w, 0);
    const uint32_t* tile = tiles + static_cast<size_t>(w) * MI355X_DPSP_WG_WORDS;
    uint32_t tb = 0;
    uint32_t expect[MI355X_DPSP_TILE];
    for (uint32_t s = 0; s < MI355X_DPSP_STAGES; ++s) {
      datapath_sparse_expected_tile(s, nw, expect);
      const uint32_t words = dpsp_dim(s) * dpsp_dim(s);
      for (uint32_t k = 0; k < words; ++k) {
        const uint32_t got = tile[dpsp_tile_offset(s) + k];
        const uint32_t want = expect[k];
        if (got == want) continue;
        ++tb;
        if (out->first_bad_wg < 0) {
          out->first_bad_wg = static_cast<int>(w);
          out->first_bad_stage = static_cast<int>(s);
          out->first_bad_word = static_cast<int>(k);
          out->first_bad_got = got;
          out->first_bad_want = want;
          out->first_bad_xor = got ^ want;
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
