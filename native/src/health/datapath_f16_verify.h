// The verdict of the f16 MFMA datapath check: what the host decides from the
// records and tiles mi355x_mfma_datapath_f16 wrote (shared by hsa_chip.cpp and
// native/tests/datapath_f16_contract_cli.cpp). Host only, no HSA: the caller
// owns the dispatch and hands over plain memory.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "datapath_f16_kernel.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

inline float dphf_as_float(uint32_t w) {
  float f;
  std::memcpy(&f, &w, sizeof(f));
  return f;
}

inline uint32_t dphf_as_word(float f) {
  uint32_t w;
  std::memcpy(&w, &f, sizeof(w));
  return w;
}

// The tile a wave with nonce `nw` computes in `stage`, as words (1024 for the
// 32x32 stages, 256 for stages 4 and 6). Plain float arithmetic in k order over
// the halves widened by integer arithmetic: every product and every partial
// sum is exact for these operands (datapath_f16_kernel.h), so neither the
// order nor a fused multiply-add changes a bit.
inline void datapath_f16_expected_tile(uint32_t stage, uint32_t nw, uint32_t* want) {
  const uint32_t dim = dphf_dim(stage), dwords = dphf_dwords(stage), words = dphf_blocks(stage) * dwords;
  float a[32][32], b[32][32];
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t w = 0; w < words; ++w) {
      const uint32_t aw = dphf_a_word(stage, i, w / dwords, w % dwords, nw);
      const uint32_t bw = dphf_b_word(stage, i, w / dwords, w % dwords, nw);
      for (uint32_t e = 0; e < 2; ++e) {
        a[i][2 * w + e] = dphf_as_float(dphf_widen(aw, e));
        b[i][2 * w + e] = dphf_as_float(dphf_widen(bw, e));
      }
    }
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t j = 0; j < dim; ++j) {
      float d = dphf_as_float(dphf_c_word(stage, i, j, nw));
      for (uint32_t k = 0; k < 2 * words; ++k) d = d + a[i][k] * b[j][k];
      want[i * dim + j] = dphf_as_word(d);
    }
}

// `records`: grid * MI355X_DPHF_REC_WORDS words, `tiles`: grid *
// MI355X_DPHF_WG_WORDS words, as mi355x_mfma_datapath_f16 left them. The
// caller has set out->nonce; every verdict field must be zero.
inline void datapath_f16_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid,
                                  mi355x_datapath_f16_result* out) {
  const uint32_t nonce = out->nonce;
  std::vector<uint32_t> cu_keys, simd_keys;
  cu_keys.reserve(grid);
  simd_keys.reserve(static_cast<size_t>(grid) * 4);
  uint32_t xmask = 0;
  out->first_bad_wg = out->first_bad_stage = out->first_bad_word = -1;
  for (uint32_t w = 0; w < grid; ++w) {
    const uint32_t* r = records + static_cast<size_t>(w) * MI355X_DPHF_REC_WORDS;
    const bool present = r[MI355X_DPHFREC_MAGIC] == MI355X_DPHF_MAGIC && r[MI355X_DPHFREC_WG] == w &&
                         r[MI355X_DPHFREC_NONCE] == (nonce ^ w);
    if (!present) continue;
    uint32_t dev_bad = 0;
    for (int s = 0; s < MI355X_DPHF_STAGES; ++s) {
      out->stage_bad[s] += r[MI355X_DPHFREC_BAD + s];
      dev_bad += r[MI355X_DPHFREC_BAD + s];
    }
    out->mfma_bad += dev_bad;
    const uint32_t x = r[MI355X_DPHFREC_XCC] & 0xF;
    xmask |= 1u << x;
    cu_keys.push_back((x << 16) | ((r[MI355X_DPHFREC_HWID] >> 8) & 0xFF));
    for (int v = 0; v < MI355X_DPHF_THREADS / 64; ++v) {
      const uint32_t h = r[MI355X_DPHFREC_HWID + v];
      simd_keys.push_back((x << 16) | (((h >> 8) & 0xFF) << 2) | ((h >> 4) & 0x3));
    }
    // wave 0's seven tiles against the host reference
    const uint32_t nw = dphf_wave_nonce(nonce, w, 0);
    const uint32_t* tile = tiles + static_cast<size_t>(w) * MI355X_DPHF_WG_WORDS;
    uint32_t tb = 0;
    uint32_t expect[MI355X_DPHF_TILE];
    for (uint32_t s = 0; s < MI355X_DPHF_STAGES; ++s) {
      datapath_f16_expected_tile(s, nw, expect);
      const uint32_t words = dphf_dim(s) * dphf_dim(s);
      for (uint32_t k = 0; k < words; ++k) {
        const uint32_t got = tile[dphf_tile_offset(s) + k];
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
