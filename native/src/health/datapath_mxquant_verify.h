// The verdict of the MX quantise check: what the host decides from the records,
// quantised images and Y tiles mi355x_mfma_datapath_mxquant wrote (shared by
// hsa_chip.cpp and native/tests/datapath_mxquant_contract_cli.cpp). Host only,
// no HSA: the caller owns the dispatches and hands over plain memory.
//
//   1. H is never formed: S_in of an element comes from its column's two live
//      terms (datapath_mxquant_kernel.h), the block's lg = floor(log2 max|S|),
//      its scale byte 125 + lg + g_i + f_b and each code from S * 2^(2-lg) by the
//      e2m1 rounding rule in integers (quarters against the grid's midpoints,
//      ties to the even code, the last code absorbing everything above);
//      every dword of the image is compared with that;
//   2. every Y word must be n * q with n an integer, |n| < 2^24;
//        n_ij = ga_ij + 2 * sum_n uq_in 2^(lg + f_b) * uw_jn 2^d'_j[b]
//      with uq from the expected codes, never from the device's image, and the
//      integers of a row are checked exactly by projection on two integer
//      vectors x with no zero entry (all ones, and odd hash values), in int64_t,
//      against (W2 x)_n computed once; only a failing row is recomputed in full;
//   3. the folds of the W1 and W2 fragments and of the scale VGPRs each wave fed
//      to its MFMAs are compared with the folds of what should have arrived.
// Word numbers (first_bad_word, --corrupt-datapath-mxquant): stage 0 (W1 feed)
// wg * 16 + wave * 2 + {0 xor, 1 sum}; stage 1 (W2 and scale feed) wg * 16 +
// wave * 4 + {W2 xor, W2 sum, scale xor, scale sum}; stage 2 (image)
// wg * 2176 hsteps + dword; stage 3 wg * 16384 + row * 128 + column.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "datapath_mxgemm_verify.h"
#include "datapath_mxquant_kernel.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

// the e2m1 code of magnitude v4 / 4: the grid's midpoints in quarters; a tie goes to the even code
inline uint32_t datapath_mxquant_code(int32_t v4) {
  static const int32_t mid[7] = {1, 3, 5, 7, 10, 14, 20};
  uint32_t code = 0;
  for (uint32_t c = 0; c < 7; ++c) code += v4 > mid[c] || (v4 == mid[c] && (c & 1u));
  return code;
}

// what is shared by all workgroups: the hidden columns' live terms, W1's fold, W2 scaled, W2 x, its folds
struct MqShared {
  uint32_t hsteps, N;                    // N = 128 hsteps hidden columns
  std::vector<uint8_t> p0, p1;           // the live pairs
  std::vector<int8_t> t0, t1;
  std::vector<uint32_t> f;               // f_b, N / 32
  std::vector<uint32_t> w2;              // [col][N / 8]
  std::vector<uint8_t> sb;               // [col][N / 32]
  std::vector<int16_t> units;            // [n][col]: uw 2^d'
  std::vector<int64_t> wx[2];            // (W2 x)_n
  int64_t x[2][MI355X_DPMQ_TILE];
  int32_t sbase[MI355X_DPMQ_TILE];
  MxFold w1fold, w2fold[2], sbfold[2];   // W1 whole (every wave reads it all); W2 and its gathered scales per column half

  MqShared(uint32_t nonce, uint32_t hsteps_) : hsteps(hsteps_), N(hsteps_ * MI355X_DPMQ_TILE) {
    p0.resize(N), p1.resize(N), t0.resize(N), t1.resize(N), f.resize(N / 32u);
    for (uint32_t n = 0; n < N; ++n) {
      uint32_t pair[2];
      int32_t t[2];
      dpmq_live(nonce, n, pair, t);
      p0[n] = static_cast<uint8_t>(pair[0]), p1[n] = static_cast<uint8_t>(pair[1]);
      t0[n] = static_cast<int8_t>(t[0]), t1[n] = static_cast<int8_t>(t[1]);
      f[n >> 5] = dpmq_f(nonce, n >> 5);
      for (uint32_t pair_i = 0; pair_i < 64; ++pair_i) w1fold.add(dpmq_w1_dword(nonce, n, pair_i));
    }
    w2.resize(static_cast<size_t>(MI355X_DPMQ_TILE) * (N / 8u));
    sb.resize(static_cast<size_t>(MI355X_DPMQ_TILE) * (N / 32u));
    units.resize(static_cast<size_t>(N) * MI355X_DPMQ_TILE);
    for (auto& v : wx) v.assign(N, 0);
    for (uint32_t j = 0; j < MI355X_DPMQ_TILE; ++j) {
      sbase[j] = static_cast<int32_t>(dpmq_sb_base(nonce, j));
      x[0][j] = 1;
      x[1][j] = static_cast<int64_t>((dpbf_hash(nonce, MI355X_DPMQ_SPACE_XV, j) & 0xFFu) | 1u);
      for (uint32_t n = 0; n < N; ++n) {
        if ((n & 7u) == 0u) w2fold[j >> 6].add(w2[j * (N / 8u) + n / 8u] = dpmq_w2_dword(nonce, hsteps, j, n / 8u));
        const uint32_t d = dpmq_sb_delta(nonce, j, n >> 5);
        if ((n & 31u) == 0u) sb[j * (N / 32u) + (n >> 5)] = static_cast<uint8_t>(sbase[j] + d);
        const int16_t u = static_cast<int16_t>(datapath_mxgemm_units((w2[j * (N / 8u) + n / 8u] >> (4u * (n & 7u))) & 0xFu) * (1 << d));
        units[static_cast<size_t>(n) * MI355X_DPMQ_TILE + j] = u;
        wx[0][n] += u * x[0][j];
        wx[1][n] += u * x[1][j];
      }
      for (uint32_t s = 0; s < hsteps; ++s) {
        uint32_t raw;
        std::memcpy(&raw, &sb[j * (N / 32u) + 4u * s], 4);
        sbfold[j >> 6].add(dpmq_gather(raw, 0));
        sbfold[j >> 6].add(dpmq_gather(raw, 1));
      }
    }
  }
};

// one token row of workgroup seed `seed`: its 16 hsteps code dwords, its hsteps scale dwords and its quantised
// elements as integers uq 2^(lg + f_b) (units of 2^(g_i - 4)); the gathered scale VGPRs fold into `sfold`
inline void datapath_mxquant_row(const MqShared& sh, uint32_t seed, uint32_t token, uint32_t* codes, uint32_t* scales,
                                 int16_t* uq, MxFold* sfold) {
  static const int16_t kUnits[8] = {0, 1, 2, 3, 4, 6, 8, 12};
  const uint32_t rh = dpmq_row(seed, token);
  const int32_t g = dpmq_g(rh);
  int32_t a[64];
  for (uint32_t p = 0; p < 64; ++p) a[p] = dpmq_a(seed, rh, token, p);
  std::fill(codes, codes + sh.N / 8u, 0u);
  std::fill(scales, scales + sh.hsteps, 0u);
  for (uint32_t b = 0; b < sh.N / 32u; ++b) {
    int32_t s[32], m = 0;
    for (uint32_t e = 0; e < 32; ++e) {
      const uint32_t n = 32u * b + e;
      s[e] = a[sh.p0[n]] * sh.t0[n] + a[sh.p1[n]] * sh.t1[n];
      m = std::max(m, s[e] < 0 ? -s[e] : s[e]);
    }
    const int32_t lg = m ? 31 - __builtin_clz(static_cast<uint32_t>(m)) : 0;
    const int32_t fb = static_cast<int32_t>(sh.f[b]);
    // the byte from the amax word, as the kernel takes it: its exponent field is 127 + lg + g + f_b
    const uint32_t e8 = dpmq_e8m0(m ? static_cast<uint32_t>(127 + lg + g + fb) << 23 : 0u);
    scales[b >> 2] |= e8 << (8u * (b & 3u));
    for (uint32_t e = 0; e < 32; ++e) {
      const int32_t mag = s[e] < 0 ? -s[e] : s[e];
      const uint32_t code = datapath_mxquant_code(mag << (4 - lg)) | (s[e] < 0 ? 8u : 0u);
      const uint32_t n = 32u * b + e;
      codes[n >> 3] |= code << (4u * (n & 7u));
      uq[n] = static_cast<int16_t>((s[e] < 0 ? -kUnits[code & 7u] : kUnits[code & 7u]) * (1 << (lg + fb)));
    }
  }
  for (uint32_t s = 0; s < sh.hsteps; ++s) {
    sfold->add(dpmq_gather(scales[s], 0));
    sfold->add(dpmq_gather(scales[s], 1));
  }
}

// the six fold words of wave v: W1 whole, W2 of its column half, the scale VGPRs of its row half and column half
inline void datapath_mxquant_wave_folds(const MqShared& sh, const MxFold* sfa, uint32_t v, uint32_t* out) {
  out[0] = sh.w1fold.x;
  out[1] = sh.w1fold.s;
  out[2] = sh.w2fold[v & 1].x;
  out[3] = sh.w2fold[v & 1].s;
  out[4] = sfa[v >> 1].x ^ sh.sbfold[v & 1].x;
  out[5] = sfa[v >> 1].s + sh.sbfold[v & 1].s;
}

// the image of a correct run of workgroup wg: the 24 fold words of its record, its quantised image, its Y words
inline void datapath_mxquant_expected(const MqShared& sh, uint32_t nonce, uint32_t wg, uint32_t* folds, uint32_t* image,
                                      uint32_t* tile) {
  const uint32_t seed = dpmq_wg_seed(nonce, wg);
  std::vector<int16_t> uq(sh.N);
  MxFold sfa[2];
  for (uint32_t i = 0; i < MI355X_DPMQ_TILE; ++i) {
    datapath_mxquant_row(sh, seed, i, image + i * (sh.N / 8u), image + 2048u * sh.hsteps + i * sh.hsteps, uq.data(), &sfa[i >> 6]);
    const int32_t g = dpmq_g(dpmq_row(seed, i));
    int64_t n[MI355X_DPMQ_TILE] = {};
    for (uint32_t k = 0; k < sh.N; ++k) {
      const int16_t* wu = &sh.units[static_cast<size_t>(k) * MI355X_DPMQ_TILE];
      for (uint32_t j = 0; j < MI355X_DPMQ_TILE; ++j) n[j] += uq[k] * wu[j];
    }
    for (uint32_t j = 0; j < MI355X_DPMQ_TILE; ++j)
      tile[i * MI355X_DPMQ_TILE + j] = dpbf_scaled_int(static_cast<int32_t>(dpmq_ga(seed, i, j) + 2 * n[j]), g + sh.sbase[j] - 132);
  }
  for (uint32_t v = 0; v < 4; ++v) datapath_mxquant_wave_folds(sh, sfa, v, folds + v * 6u);
}

// `records`: grid * MI355X_DPMQ_REC_WORDS words, `image`: grid * MI355X_DPMQ_IMG_WORDS(hsteps), `tiles`: grid *
// MI355X_DPMQ_WG_WORDS, as mi355x_mfma_datapath_mxquant left them. The caller has set out->nonce; every verdict
// field must be zero.
inline void datapath_mxquant_verdict(const uint32_t* records, const uint32_t* image, const uint32_t* tiles, uint32_t grid,
                                     uint32_t hsteps, mi355x_datapath_mxquant_result* out) {
  const uint32_t nonce = out->nonce, img_words = MI355X_DPMQ_IMG_WORDS(hsteps);
  const MqShared sh(nonce, hsteps);
  std::vector<uint32_t> cu_keys, simd_keys, want_img(sh.N / 8u + hsteps);
  std::vector<int16_t> uq(sh.N);
  uint32_t xmask = 0;
  out->first_bad_wg = out->first_bad_stage = out->first_bad_word = -1;
  const auto note = [out](uint32_t wg, int stage, uint32_t word, uint32_t got, uint32_t want) {
    ++out->stage_bad[stage];
    if (out->first_bad_wg >= 0 && (out->first_bad_wg != static_cast<int>(wg) || out->first_bad_stage <= stage)) return;
    out->first_bad_wg = static_cast<int>(wg);
    out->first_bad_stage = stage;
    out->first_bad_word = static_cast<int>(word);
    out->first_bad_got = got;
    out->first_bad_want = want;
    out->first_bad_xor = got ^ want;
  };
  const auto bad_words = [out] { return out->stage_bad[0] + out->stage_bad[1] + out->stage_bad[2] + out->stage_bad[3]; };
  for (uint32_t w = 0; w < grid; ++w) {
    const uint32_t* r = records + static_cast<size_t>(w) * MI355X_DPMQ_REC_WORDS;
    if (r[MI355X_DPMQREC_MAGIC] != MI355X_DPMQ_MAGIC || r[MI355X_DPMQREC_WG] != w ||
        r[MI355X_DPMQREC_NONCE] != (nonce ^ w) || (r[MI355X_DPMQREC_XCC] >> 8) != hsteps)
      continue;
    const uint32_t xcc = r[MI355X_DPMQREC_XCC] & 0xF;
    xmask |= 1u << xcc;
    cu_keys.push_back((xcc << 16) | ((r[MI355X_DPMQREC_HWID] >> 8) & 0xFF));
    for (int v = 0; v < MI355X_DPMQ_THREADS / 64; ++v) {
      const uint32_t h = r[MI355X_DPMQREC_HWID + v];
      simd_keys.push_back((xcc << 16) | (((h >> 8) & 0xFF) << 2) | ((h >> 4) & 0x3));
    }
    const uint32_t before = bad_words();
    const uint32_t seed = dpmq_wg_seed(nonce, w);
    const uint32_t* img = image + static_cast<size_t>(w) * img_words;
    const uint32_t* tile = tiles + static_cast<size_t>(w) * MI355X_DPMQ_WG_WORDS;
    MxFold sfa[2];
    for (uint32_t i = 0; i < MI355X_DPMQ_TILE; ++i) {
      uint32_t* want_codes = want_img.data();
      uint32_t* want_scales = want_img.data() + sh.N / 8u;
      datapath_mxquant_row(sh, seed, i, want_codes, want_scales, uq.data(), &sfa[i >> 6]);
      for (uint32_t d = 0; d < sh.N / 8u; ++d) {
        const uint32_t at = i * (sh.N / 8u) + d;
        if (img[at] != want_codes[d]) note(w, 2, w * img_words + at, img[at], want_codes[d]);
      }
      for (uint32_t s = 0; s < hsteps; ++s) {
        const uint32_t at = 2048u * hsteps + i * hsteps + s;
        if (img[at] != want_scales[s]) note(w, 2, w * img_words + at, img[at], want_scales[s]);
      }
      const int32_t g = dpmq_g(dpmq_row(seed, i));
      int64_t want[2] = {0, 0}, got[2] = {0, 0};
      for (uint32_t k = 0; k < sh.N; ++k) {
        want[0] += 2 * uq[k] * sh.wx[0][k];
        want[1] += 2 * uq[k] * sh.wx[1][k];
      }
      bool row_ok = true;
      for (uint32_t j = 0; j < MI355X_DPMQ_TILE; ++j) {
        const int64_t ga = dpmq_ga(seed, i, j);
        int64_t n = 0;
        row_ok = datapath_mxgemm_quanta(tile[i * MI355X_DPMQ_TILE + j], g + sh.sbase[j] - 132, &n) && row_ok;
        for (int v = 0; v < 2; ++v) {
          want[v] += ga * sh.x[v][j];
          got[v] += n * sh.x[v][j];
        }
      }
      if (row_ok && got[0] == want[0] && got[1] == want[1]) continue;
      for (uint32_t j = 0; j < MI355X_DPMQ_TILE; ++j) {  // the whole row, to name and count its wrong words
        int64_t n = 0;
        for (uint32_t k = 0; k < sh.N; ++k) n += uq[k] * sh.units[static_cast<size_t>(k) * MI355X_DPMQ_TILE + j];
        const uint32_t word = dpbf_scaled_int(static_cast<int32_t>(dpmq_ga(seed, i, j) + 2 * n), g + sh.sbase[j] - 132);
        const uint32_t at = i * MI355X_DPMQ_TILE + j;
        if (tile[at] != word) note(w, 3, w * MI355X_DPMQ_WG_WORDS + at, tile[at], word);
      }
    }
    for (uint32_t v = 0; v < 4; ++v) {
      uint32_t want[6];
      datapath_mxquant_wave_folds(sh, sfa, v, want);
      for (uint32_t k = 0; k < 6; ++k) {
        const uint32_t got = r[MI355X_DPMQREC_FOLD + v * 6u + k];
        if (got != want[k]) note(w, k < 2 ? 0 : 1, w * 16u + (k < 2 ? v * 2u + k : v * 4u + k - 2u), got, want[k]);
      }
    }
    if (bad_words() == before) ++out->records_ok;
  }
  out->mfma_bad = out->stage_bad[0] + out->stage_bad[1];
  out->tile_bad = out->stage_bad[3];
  std::sort(cu_keys.begin(), cu_keys.end());
  out->cus_covered = static_cast<int>(std::unique(cu_keys.begin(), cu_keys.end()) - cu_keys.begin());
  std::sort(simd_keys.begin(), simd_keys.end());
  out->simds_covered = static_cast<int>(std::unique(simd_keys.begin(), simd_keys.end()) - simd_keys.begin());
  out->xccs_covered = __builtin_popcount(xmask);
  out->ok = out->records_ok == static_cast<int>(grid);
  if (out->ok) return;
  int n = std::snprintf(out->error, sizeof(out->error), "%d/%u workgroups exact (feed_bad=%u quant_bad=%u y_bad=%u)",
                        out->records_ok, grid, out->mfma_bad, out->stage_bad[2], out->tile_bad);
  if (out->first_bad_wg >= 0 && n > 0 && n < static_cast<int>(sizeof(out->error))) {
    const uint32_t x = out->first_bad_xor;
    n += std::snprintf(out->error + n, sizeof(out->error) - n, "; first bad: wg %d stage %d word %d xor 0x%08x",
                       out->first_bad_wg, out->first_bad_stage, out->first_bad_word, x);
    if ((x & (x - 1)) == 0 && n < static_cast<int>(sizeof(out->error)))
      std::snprintf(out->error + n, sizeof(out->error) - n, " (bit %d)", __builtin_ctz(x));
  }
}

}  // namespace mi355x
