// The verdict of the split-K GEMM check: what the host decides from the records
// mi355x_mfma_datapath_splitk wrote and the D tiles and ledgers
// mi355x_splitk_drain copied out (shared by hsa_chip.cpp and
// native/tests/datapath_splitk_contract_cli.cpp). Host only, no HSA: the caller
// owns the dispatches and hands over plain memory.
//
// A tile's final D is the GEMM pipeline check's D for the same panel at
// ksteps_total = splits * ksteps, whatever order the partials arrived in, so the
// method is datapath_gemm_verify.h's, tile by tile:
//   1. every D word must be n * q with n an integer, |n| < 2^24;
//   2. the integers of a row are checked exactly by projection on two integer
//      vectors, in int64_t;
//   3. only a failing row is recomputed in full, to name and count its wrong words;
//   4. each workgroup's folds are compared with the folds of the elements of its
//      k-range;
//   5. each ledger: arrivals = splits, the xor of nonce ^ wg over the tile's
//      workgroups, and the sums / xors of the contributors' folds.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "datapath_gemm_verify.h"
#include "datapath_splitk_kernel.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

// the folds of B per split and column half (the same for every tile)
inline std::vector<GemmFold> datapath_splitk_b_folds(const GemmB& b, uint32_t splits, uint32_t ksteps) {
  std::vector<GemmFold> f(static_cast<size_t>(splits) * 2);
  for (uint32_t k = 0; k < b.K; ++k)
    for (uint32_t j = 0; j < MI355X_DPGM_TILE; ++j)
      f[(k / (ksteps * MI355X_DPGM_KSTEP)) * 2 + (j >> 6)].add(b.elem[static_cast<size_t>(k) * MI355X_DPGM_TILE + j]);
  return f;
}

// the 16 fold words of the record of the workgroup with split `s`, from the folds of A (per split and row half) and B
inline void datapath_splitk_folds(const GemmFold* fa, const GemmFold* fb, uint32_t s, uint32_t* folds) {
  for (uint32_t v = 0; v < 4; ++v) {
    folds[v * 4 + 0] = fa[s * 2 + (v >> 1)].x;
    folds[v * 4 + 1] = fa[s * 2 + (v >> 1)].s;
    folds[v * 4 + 2] = fb[s * 2 + (v & 1)].x;
    folds[v * 4 + 3] = fb[s * 2 + (v & 1)].s;
  }
}

// the ledger a tile's workgroups leave, from their fold words
inline void datapath_splitk_ledger(const GemmFold* fa, const GemmFold* fb, uint32_t nonce, uint32_t tile, uint32_t splits,
                                   uint32_t* led) {
  std::memset(led, 0, MI355X_DPSK_LEDGER_WORDS * sizeof(uint32_t));
  for (uint32_t s = 0; s < splits; ++s) {
    led[MI355X_DPSKLED_ARRIVALS] += 1;
    led[MI355X_DPSKLED_WHO] ^= nonce ^ (tile * splits + s);
    led[MI355X_DPSKLED_A_SUM] += fa[s * 2].s + fa[s * 2 + 1].s;
    led[MI355X_DPSKLED_A_XOR] ^= fa[s * 2].x ^ fa[s * 2 + 1].x;
    led[MI355X_DPSKLED_B_SUM] += fb[s * 2].s + fb[s * 2 + 1].s;
    led[MI355X_DPSKLED_B_XOR] ^= fb[s * 2].x ^ fb[s * 2 + 1].x;
  }
}

// the folds of A_t per split and row half
inline std::vector<GemmFold> datapath_splitk_a_folds(uint32_t nonce, uint32_t tile, uint32_t splits, uint32_t ksteps) {
  const uint32_t kt = splits * ksteps, K = kt * MI355X_DPGM_KSTEP;
  std::vector<GemmFold> f(static_cast<size_t>(splits) * 2);
  std::vector<uint16_t> ae(K);
  std::vector<int16_t> au(K);
  for (uint32_t i = 0; i < MI355X_DPGM_TILE; ++i) {
    datapath_gemm_a_row(dpgm_wg_seed(nonce, tile), kt, i, ae.data(), au.data());
    for (uint32_t k = 0; k < K; ++k) f[(k / (ksteps * MI355X_DPGM_KSTEP)) * 2 + (i >> 6)].add(ae[k]);
  }
  return f;
}

// `records`: tiles * splits * MI355X_DPSK_REC_WORDS words as the kernel left them; `d`: tiles * 16384 words and
// `ledger`: tiles * 8 words as the drain copied them. The caller has set out->nonce; every verdict field must be zero.
// stage_bad: wrong fold words of the A feed, of the B feed, wrong D words, wrong ledger words; mfma_bad is the feeds'
// sum. records_ok counts exact tiles: all of a tile's records present, and nothing of it wrong.
inline void datapath_splitk_verdict(const uint32_t* records, const uint32_t* d, const uint32_t* ledger, uint32_t tiles,
                                    uint32_t splits, uint32_t ksteps, mi355x_datapath_splitk_result* out) {
  const uint32_t nonce = out->nonce, kt = splits * ksteps;
  const GemmB b(nonce, kt);
  const std::vector<GemmFold> fb = datapath_splitk_b_folds(b, splits, ksteps);
  std::vector<uint32_t> cu_keys, simd_keys;
  std::vector<uint16_t> ae(b.K);
  std::vector<int16_t> au(b.K);
  uint32_t xmask = 0;
  int xccs_min = -1;
  out->first_bad_wg = out->first_bad_stage = out->first_bad_word = -1;
  const auto note = [out](uint32_t tile, int stage, uint32_t word, uint32_t got, uint32_t want) {
    ++out->stage_bad[stage];
    if (out->first_bad_wg >= 0 && (out->first_bad_wg != static_cast<int>(tile) || out->first_bad_stage <= stage)) return;
    out->first_bad_wg = static_cast<int>(tile);
    out->first_bad_stage = stage;
    out->first_bad_word = static_cast<int>(word);
    out->first_bad_got = got;
    out->first_bad_want = want;
    out->first_bad_xor = got ^ want;
  };
  const auto bad_total = [out] { return out->stage_bad[0] + out->stage_bad[1] + out->stage_bad[2] + out->stage_bad[3]; };
  for (uint32_t t = 0; t < tiles; ++t) {
    const uint32_t before = bad_total();
    const uint32_t seed = dpgm_wg_seed(nonce, t);
    const uint32_t* tile = d + static_cast<size_t>(t) * MI355X_DPSK_TILE_WORDS;
    std::vector<GemmFold> fa(static_cast<size_t>(splits) * 2);
    for (uint32_t i = 0; i < MI355X_DPGM_TILE; ++i) {
      datapath_gemm_a_row(seed, kt, i, ae.data(), au.data());
      int64_t want[2] = {0, 0}, got[2] = {0, 0};
      for (uint32_t k = 0; k < b.K; ++k) {
        fa[(k / (ksteps * MI355X_DPGM_KSTEP)) * 2 + (i >> 6)].add(ae[k]);
        want[0] += au[k] * b.bx[0][k];
        want[1] += au[k] * b.bx[1][k];
      }
      bool row_ok = true;
      for (uint32_t j = 0; j < MI355X_DPGM_TILE; ++j) {
        const int64_t ga = dpgm_ga(seed, i, j);
        int64_t n = 0;
        row_ok = datapath_gemm_quanta(tile[i * MI355X_DPGM_TILE + j], dpgm_qx(seed, nonce, i, j), &n) && row_ok;
        for (int v = 0; v < 2; ++v) {
          want[v] += ga * b.x[v][j];
          got[v] += n * b.x[v][j];
        }
      }
      if (row_ok && got[0] == want[0] && got[1] == want[1]) continue;
      for (uint32_t j = 0; j < MI355X_DPGM_TILE; ++j) {  // the whole row, to name and count its wrong words
        int64_t n = dpgm_ga(seed, i, j);
        for (uint32_t k = 0; k < b.K; ++k) n += au[k] * b.units[static_cast<size_t>(k) * MI355X_DPGM_TILE + j];
        const uint32_t word = datapath_gemm_word(n, dpgm_qx(seed, nonce, i, j)), at = i * MI355X_DPGM_TILE + j;
        if (tile[at] != word) note(t, 2, t * MI355X_DPSK_TILE_WORDS + at, tile[at], word);
      }
    }
    bool all_here = true;
    uint32_t tile_xmask = 0;
    for (uint32_t s = 0; s < splits; ++s) {
      const uint32_t w = t * splits + s;
      const uint32_t* r = records + static_cast<size_t>(w) * MI355X_DPSK_REC_WORDS;
      if (r[MI355X_DPSKREC_MAGIC] != MI355X_DPSK_MAGIC || r[MI355X_DPSKREC_WG] != w || r[MI355X_DPSKREC_NONCE] != (nonce ^ w) ||
          r[MI355X_DPSKREC_TILES] != tiles || r[MI355X_DPSKREC_SPLITS] != splits || r[MI355X_DPSKREC_KSTEPS] != ksteps) {
        all_here = false;
        continue;
      }
      const uint32_t xcc = r[MI355X_DPSKREC_XCC] & 0xF;
      tile_xmask |= 1u << xcc;
      cu_keys.push_back((xcc << 16) | ((r[MI355X_DPSKREC_HWID] >> 8) & 0xFF));
      for (int v = 0; v < MI355X_DPSK_THREADS / 64; ++v) {
        const uint32_t h = r[MI355X_DPSKREC_HWID + v];
        simd_keys.push_back((xcc << 16) | (((h >> 8) & 0xFF) << 2) | ((h >> 4) & 0x3));
      }
      uint32_t folds[16];
      datapath_splitk_folds(fa.data(), fb.data(), s, folds);
      for (uint32_t word = 0; word < 8; ++word)
        for (uint32_t stage = 0; stage < 2; ++stage) {
          const uint32_t slot = dpsk_fold_slot(stage, word);
          if (r[slot] != folds[slot - MI355X_DPSKREC_FOLD]) note(t, static_cast<int>(stage), w * 8 + word, r[slot], folds[slot - MI355X_DPSKREC_FOLD]);
        }
    }
    uint32_t led[MI355X_DPSK_LEDGER_WORDS];
    datapath_splitk_ledger(fa.data(), fb.data(), nonce, t, splits, led);
    for (uint32_t word = 0; word < MI355X_DPSK_LEDGER_WORDS; ++word) {
      const uint32_t got = ledger[t * MI355X_DPSK_LEDGER_WORDS + word];
      if (got != led[word]) note(t, 3, t * MI355X_DPSK_LEDGER_WORDS + word, got, led[word]);
    }
    xmask |= tile_xmask;
    if (all_here && (xccs_min < 0 || __builtin_popcount(tile_xmask) < xccs_min)) xccs_min = __builtin_popcount(tile_xmask);
    if (all_here && bad_total() == before) ++out->records_ok;
  }
  out->mfma_bad = out->stage_bad[0] + out->stage_bad[1];
  out->tile_bad = out->stage_bad[2];
  out->ledger_bad = out->stage_bad[3];
  std::sort(cu_keys.begin(), cu_keys.end());
  out->cus_covered = static_cast<int>(std::unique(cu_keys.begin(), cu_keys.end()) - cu_keys.begin());
  std::sort(simd_keys.begin(), simd_keys.end());
  out->simds_covered = static_cast<int>(std::unique(simd_keys.begin(), simd_keys.end()) - simd_keys.begin());
  out->xccs_covered = __builtin_popcount(xmask);
  out->xccs_per_tile_min = xccs_min < 0 ? 0 : xccs_min;
  out->ok = out->records_ok == static_cast<int>(tiles);
  if (out->ok) return;
  int n = std::snprintf(out->error, sizeof(out->error), "%d/%u tiles exact (feed_bad=%u tile_bad=%u ledger_bad=%u)",
                        out->records_ok, tiles, out->mfma_bad, out->tile_bad, out->ledger_bad);
  if (out->first_bad_wg >= 0 && n > 0 && n < static_cast<int>(sizeof(out->error))) {
    const uint32_t x = out->first_bad_xor;
    n += std::snprintf(out->error + n, sizeof(out->error) - n, "; first bad: tile %d stage %d word %d xor 0x%08x",
                       out->first_bad_wg, out->first_bad_stage, out->first_bad_word, x);
    if ((x & (x - 1)) == 0 && n < static_cast<int>(sizeof(out->error)))
      std::snprintf(out->error + n, sizeof(out->error) - n, " (bit %d)", __builtin_ctz(x));
  }
}

}  // namespace mi355x
