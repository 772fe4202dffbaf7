// The verdict the eight register-only datapath checks share (f32, int8, bf16,
// fp8, f16, f64, fp6 / fp4, sparse): what the host decides from the records and
// tiles a check's kernel wrote. A check describes itself by a traits struct
// (DatapathTraits below, its own datapath_*_verify.h): the record and tile
// sizes of its kernel header, where a stage's tiles lie, and its expected_tile,
// the part that really differs per number format. hsa_chip.cpp runs the checks
// from the same traits. Host only, no HSA: the caller owns the dispatch and
// hands over plain memory.
//
// A traits struct T has
//   Result, Args             the check's result struct and its kernel's arguments (records, tiles, nonce, grid)
//   kKind                    the kind's wire name, a row of probe_kinds.h
//   kSymbol, kDispatch       the kernel's symbol; what a dispatch that misses its deadline is called
//   kMagic, kRecWords, kWgWords, kThreads, kStages, kTileWords (the largest tile)
//   wave_nonce(nonce, wg)    wave 0's nonce
//   tile_offset(stage), tiles(stage), tile_words(stage)
//                            a stage's tiles lie one after another from tile_offset, within a workgroup's kWgWords
//   expected_tile(stage, tile, nw, want)
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mi355x/liveness_probe.h"

namespace mi355x {

// a record's words, the same in all eight kernel headers (each verify header asserts its own)
enum : uint32_t { kDpRecMagic = 0, kDpRecWg = 1, kDpRecNonce = 2, kDpRecXcc = 3, kDpRecHwid = 4, kDpRecBad = 8 };

#define MI355X_DP_ASSERT_RECORD(REC)                                                                               \
  static_assert(REC##_MAGIC == kDpRecMagic && REC##_WG == kDpRecWg && REC##_NONCE == kDpRecNonce &&                \
                    REC##_XCC == kDpRecXcc && REC##_HWID == kDpRecHwid && REC##_BAD == kDpRecBad,                  \
                "the shared verdict reads this record layout")

// The traits of a check whose every stage is one square tile of dim(stage)^2
// words: P the kernel header's macro prefix (DPI8), p its functions' (dpi8),
// `what` the name of its dispatch ("datapath i8 check").
#define MI355X_DP_SQUARE_TRAITS(Traits, kind, P, p, what)                                                          \
  MI355X_DP_ASSERT_RECORD(MI355X_##P##REC);                                                                        \
  struct Traits {                                                                                                  \
    using Result = mi355x_##kind##_result;                                                                         \
    using Args = mi355x_##kind##_args;                                                                             \
    static constexpr const char* kKind = #kind;                                                                    \
    static constexpr const char* kSymbol = "mi355x_mfma_" #kind ".kd";                                             \
    static constexpr const char* kDispatch = what;                                                                 \
    static constexpr uint32_t kMagic = MI355X_##P##_MAGIC, kRecWords = MI355X_##P##_REC_WORDS,                     \
                              kWgWords = MI355X_##P##_WG_WORDS, kThreads = MI355X_##P##_THREADS,                   \
                              kStages = MI355X_##P##_STAGES, kTileWords = MI355X_##P##_TILE;                       \
    static uint32_t wave_nonce(uint32_t nonce, uint32_t wg) { return p##_wave_nonce(nonce, wg, 0); }               \
    static uint32_t tile_offset(uint32_t stage) { return p##_tile_offset(stage); }                                 \
    static uint32_t tiles(uint32_t) { return 1; }                                                                  \
    static uint32_t tile_words(uint32_t stage) { return p##_dim(stage) * p##_dim(stage); }                         \
    static void expected_tile(uint32_t stage, uint32_t, uint32_t nw, uint32_t* want) {                             \
      kind##_expected_tile(stage, nw, want);                                                                       \
    }                                                                                                              \
  }

// `records`: grid * T::kRecWords words, `tiles`: grid * T::kWgWords words, as
// the kernel left them. The caller has set out->nonce; every verdict field
// must be zero.
template <typename T>
void datapath_register_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid,
                               typename T::Result* out) {
  const uint32_t nonce = out->nonce;
  std::vector<uint32_t> cu_keys, simd_keys;
  cu_keys.reserve(grid);
  simd_keys.reserve(static_cast<size_t>(grid) * 4);
  uint32_t xmask = 0;
  out->first_bad_wg = out->first_bad_stage = out->first_bad_word = -1;
  for (uint32_t w = 0; w < grid; ++w) {
    const uint32_t* r = records + static_cast<size_t>(w) * T::kRecWords;
    const bool present = r[kDpRecMagic] == T::kMagic && r[kDpRecWg] == w && r[kDpRecNonce] == (nonce ^ w);
    if (!present) continue;
    uint32_t dev_bad = 0;
    for (uint32_t s = 0; s < T::kStages; ++s) {
      out->stage_bad[s] += r[kDpRecBad + s];
      dev_bad += r[kDpRecBad + s];
    }
    out->mfma_bad += dev_bad;
    const uint32_t x = r[kDpRecXcc] & 0xF;
    xmask |= 1u << x;
    cu_keys.push_back((x << 16) | ((r[kDpRecHwid] >> 8) & 0xFF));
    for (uint32_t v = 0; v < T::kThreads / 64; ++v) {
      const uint32_t h = r[kDpRecHwid + v];
      simd_keys.push_back((x << 16) | (((h >> 8) & 0xFF) << 2) | ((h >> 4) & 0x3));
    }
    // wave 0's tiles against the host reference
    const uint32_t nw = T::wave_nonce(nonce, w);
    const uint32_t* tile = tiles + static_cast<size_t>(w) * T::kWgWords;
    uint32_t tb = 0;
    uint32_t expect[T::kTileWords];
    for (uint32_t s = 0; s < T::kStages; ++s) {
      const uint32_t words = T::tile_words(s);
      for (uint32_t t = 0; t < T::tiles(s); ++t) {
        T::expected_tile(s, t, nw, expect);
        for (uint32_t k = 0; k < words; ++k) {
          const uint32_t got = tile[T::tile_offset(s) + t * words + k];
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
