// The verdict of the MXFP4 GEMM pipeline check: what the host decides from the
// records and D tiles mi355x_mfma_datapath_mxgemm wrote (shared by hsa_chip.cpp
// and native/tests/datapath_mxgemm_contract_cli.cpp). Host only, no HSA: the
// caller owns the dispatches and hands over plain memory.
//
// The method of datapath_gemm_verify.h:
//   1. every D word must be n * q with n an integer, |n| < 2^24 (q is the
//      output's quantum, datapath_mxgemm_kernel.h); anything else is wrong at once;
//   2. with ua, ub the elements in units of 2^-1 (decoded by integer arithmetic,
//      dpf6_decode: no device or library convert) and d, d' the scale offsets,
//        n_ij = ga_ij + 2 * sum_k ua_ik 2^d_i[k>>5] * ub_jk 2^d'_j[k>>5]
//      and the integers of a row are checked exactly by projection on two integer
//      vectors x with no zero entry (all ones, and odd hash values), in int64_t:
//        sum_j n_ij x_j == ga_i . x + 2 * sum_g 2^d_i[g] sum_(k in g) ua_ik (B x)_k
//      with (B x)_k = sum_j ub_jk 2^d'_j[k>>5] x_j computed once;
//   3. only a failing row is recomputed in full, to name and count its wrong words;
//   4. the folds of the fragments and scale VGPRs each wave fed to its MFMAs are
//      compared with the folds of what should have arrived.
// Word numbers (first_bad_word, --corrupt-datapath-mxgemm): stages 0 (A feed),
// 1 (B feed) and 2 (scale feed) wg * 16 + wave * 2 + {0 xor, 1 sum}, the record
// word dpmx_fold_slot(stage, wave * 2 + ..); stage 3 wg * 16384 + row * 128 + column.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "datapath_f6f4_kernel.h"
#include "datapath_mxgemm_kernel.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

// xor and sum modulo 2^32 over dwords
struct MxFold {
  uint32_t x = 0, s = 0;
  void add(uint32_t w) {
    x ^= w;
    s += w;
  }
};

// an e2m1 code in units of 2^-1, from the f32 word of its value
inline int32_t datapath_mxgemm_units(uint32_t code) {
  const uint32_t w = dpf6_decode(code, MI355X_DPF6_E2M1);
  if ((w & 0x7FFFFFFFu) == 0u) return 0;  // +-0: in no operand, but a faulty feed may hold it
  const int32_t mag = static_cast<int32_t>(((w & 0x7FFFFFu) | 0x800000u) >> (149u - ((w >> 23) & 0xFFu)));
  return (w >> 31) ? -mag : mag;
}

// one row of A_wg (which = 0, seed = the workgroup's) or column of B (which = 1, seed = the nonce): its K/8 dwords,
// its K/32 scale bytes, its elements as integers ua * 2^d, and their folds into the half's feed and scale folds
inline void datapath_mxgemm_line(uint32_t seed, uint32_t which, uint32_t ksteps, uint32_t rc, uint32_t* dwords,
                                 uint8_t* scales, int16_t* units, MxFold* feed, MxFold* sfold) {
  const uint32_t blocks = ksteps * 8u;
  int16_t code_units[16];  // decoded once a line, not once an element
  for (uint32_t c = 0; c < 16; ++c) code_units[c] = static_cast<int16_t>(datapath_mxgemm_units(c));
  for (uint32_t g = 0; g < blocks; ++g) {
    scales[g] = static_cast<uint8_t>(dpmx_scale_byte(seed, which, rc, g));
    const uint32_t d = dpmx_delta(seed, which, rc, g);
    for (uint32_t kd = 4u * g; kd < 4u * g + 4u; ++kd) {
      const uint32_t w = which ? dpmx_b_dword(seed, ksteps, rc, kd) : dpmx_a_dword(seed, ksteps, rc, kd);
      dwords[kd] = w;
      feed->add(w);
      for (uint32_t e = 0; e < 8; ++e)
        units[kd * 8u + e] = static_cast<int16_t>(code_units[(w >> (4u * e)) & 0xFu] * (1 << d));
    }
  }
  for (uint32_t s = 0; s < ksteps; ++s) {
    uint32_t lo, hi;
    std::memcpy(&lo, scales + 8u * s, 4);
    std::memcpy(&hi, scales + 8u * s + 4u, 4);
    sfold->add(dpmx_gather(lo, hi, 0));
    sfold->add(dpmx_gather(lo, hi, 1));
  }
}

// B as the fill writes it: dwords [col][K/8], scale bytes [col][K/32], the scaled integers [k][col], B x for the two
// vectors, the folds per column half
struct MxB {
  uint32_t ksteps, K;
  std::vector<uint32_t> dwords;
  std::vector<uint8_t> scales;
  std::vector<int16_t> units;
  std::vector<int64_t> bx[2];
  int64_t x[2][MI355X_DPMX_TILE];
  int32_t sbase[MI355X_DPMX_TILE];  // SB_j: an output's quantum is 2^(SA_i + SB_j - 257), dpmx_qx
  MxFold fold[2], sfold[2];

  MxB(uint32_t nonce, uint32_t ksteps_) : ksteps(ksteps_), K(ksteps_ * MI355X_DPMX_KSTEP) {
    dwords.resize(static_cast<size_t>(MI355X_DPMX_TILE) * (K / 8u));
    scales.resize(static_cast<size_t>(MI355X_DPMX_TILE) * (K / 32u));
    units.resize(static_cast<size_t>(K) * MI355X_DPMX_TILE);
    std::vector<int16_t> col(K);
    for (auto& v : bx) v.assign(K, 0);
    for (uint32_t j = 0; j < MI355X_DPMX_TILE; ++j) {
      sbase[j] = static_cast<int32_t>(dpmx_scale_base(nonce, 1u, j));
      x[0][j] = 1;
      x[1][j] = static_cast<int64_t>((dpbf_hash(nonce, MI355X_DPMX_SPACE_X, j) & 0xFFu) | 1u);
      datapath_mxgemm_line(nonce, 1u, ksteps, j, &dwords[static_cast<size_t>(j) * (K / 8u)],
                           &scales[static_cast<size_t>(j) * (K / 32u)], col.data(), &fold[j >> 6], &sfold[j >> 6]);
      for (uint32_t k = 0; k < K; ++k) {
        units[static_cast<size_t>(k) * MI355X_DPMX_TILE + j] = col[k];
        bx[0][k] += col[k] * x[0][j];
        bx[1][k] += col[k] * x[1][j];
      }
    }
  }
};

// n of a D word that is n * 2^qx with n an integer, |n| < 2^24; false for any other word
inline bool datapath_mxgemm_quanta(uint32_t word, int32_t qx, int64_t* n) {
  const int32_t e = static_cast<int32_t>((word >> 23) & 0xFFu);
  const int32_t down = qx - (e - 150);  // the significand, an integer of 24 bits, is in units of 2^(e-150)
  if (e == 0 || e == 255 || down < 0 || down > 23) return false;
  const int64_t sig = static_cast<int64_t>((word & 0x7FFFFFu) | 0x800000u);
  if (sig & ((int64_t{1} << down) - 1)) return false;
  *n = (word >> 31) ? -(sig >> down) : (sig >> down);
  return true;
}

// the six fold words of wave v: A of its row half, B of its column half, the scale VGPRs of both
inline void datapath_mxgemm_wave_folds(const MxB& b, const MxFold* fa, const MxFold* sfa, uint32_t v, uint32_t* out) {
  out[0] = fa[v >> 1].x;
  out[1] = fa[v >> 1].s;
  out[2] = b.fold[v & 1].x;
  out[3] = b.fold[v & 1].s;
  out[4] = sfa[v >> 1].x ^ b.sfold[v & 1].x;
  out[5] = sfa[v >> 1].s + b.sfold[v & 1].s;
}

// the image of a correct run of workgroup wg: its 128 x 128 D words and the 24 fold words of its record
inline void datapath_mxgemm_expected(const MxB& b, uint32_t nonce, uint32_t wg, uint32_t* tile, uint32_t* folds) {
  const uint32_t seed = dpmx_wg_seed(nonce, wg);
  std::vector<uint32_t> ad(b.K / 8u);
  std::vector<uint8_t> as(b.K / 32u);
  std::vector<int16_t> au(b.K);
  MxFold fa[2], sfa[2];
  for (uint32_t i = 0; i < MI355X_DPMX_TILE; ++i) {
    const int32_t sa_i = static_cast<int32_t>(dpmx_scale_base(seed, 0u, i));
    datapath_mxgemm_line(seed, 0u, b.ksteps, i, ad.data(), as.data(), au.data(), &fa[i >> 6], &sfa[i >> 6]);
    int64_t n[MI355X_DPMX_TILE] = {};
    for (uint32_t k = 0; k < b.K; ++k) {
      const int16_t* bu = &b.units[static_cast<size_t>(k) * MI355X_DPMX_TILE];
      for (uint32_t j = 0; j < MI355X_DPMX_TILE; ++j) n[j] += au[k] * bu[j];
    }
    for (uint32_t j = 0; j < MI355X_DPMX_TILE; ++j)
      tile[i * MI355X_DPMX_TILE + j] =
          dpbf_scaled_int(static_cast<int32_t>(dpmx_ga(seed, i, j) + 2 * n[j]), sa_i + b.sbase[j] - 257);
  }
  for (uint32_t v = 0; v < 4; ++v) datapath_mxgemm_wave_folds(b, fa, sfa, v, folds + v * 6u);
}

// `records`: grid * MI355X_DPMX_REC_WORDS words, `tiles`: grid *
// MI355X_DPMX_WG_WORDS words, as mi355x_mfma_datapath_mxgemm left them. The
// caller has set out->nonce; every verdict field must be zero.
inline void datapath_mxgemm_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid, uint32_t ksteps,
                                    mi355x_datapath_mxgemm_result* out) {
  const uint32_t nonce = out->nonce;
  const MxB b(nonce, ksteps);
  std::vector<uint32_t> cu_keys, simd_keys;
  std::vector<uint32_t> ad(b.K / 8u);
  std::vector<uint8_t> as(b.K / 32u);
  std::vector<int16_t> au(b.K);
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
    const uint32_t* r = records + static_cast<size_t>(w) * MI355X_DPMX_REC_WORDS;
    if (r[MI355X_DPMXREC_MAGIC] != MI355X_DPMX_MAGIC || r[MI355X_DPMXREC_WG] != w ||
        r[MI355X_DPMXREC_NONCE] != (nonce ^ w) || (r[MI355X_DPMXREC_XCC] >> 8) != ksteps)
      continue;
    const uint32_t xcc = r[MI355X_DPMXREC_XCC] & 0xF;
    xmask |= 1u << xcc;
    cu_keys.push_back((xcc << 16) | ((r[MI355X_DPMXREC_HWID] >> 8) & 0xFF));
    for (int v = 0; v < MI355X_DPMX_THREADS / 64; ++v) {
      const uint32_t h = r[MI355X_DPMXREC_HWID + v];
      simd_keys.push_back((xcc << 16) | (((h >> 8) & 0xFF) << 2) | ((h >> 4) & 0x3));
    }
    const uint32_t before = bad_words();
    const uint32_t seed = dpmx_wg_seed(nonce, w);
    const uint32_t* tile = tiles + static_cast<size_t>(w) * MI355X_DPMX_WG_WORDS;
    MxFold fa[2], sfa[2];
    for (uint32_t i = 0; i < MI355X_DPMX_TILE; ++i) {
      const int32_t sa_i = static_cast<int32_t>(dpmx_scale_base(seed, 0u, i));
      datapath_mxgemm_line(seed, 0u, ksteps, i, ad.data(), as.data(), au.data(), &fa[i >> 6], &sfa[i >> 6]);
      int64_t want[2] = {0, 0}, got[2] = {0, 0};
      for (uint32_t k = 0; k < b.K; ++k) {
        want[0] += 2 * au[k] * b.bx[0][k];
        want[1] += 2 * au[k] * b.bx[1][k];
      }
      bool row_ok = true;
      for (uint32_t j = 0; j < MI355X_DPMX_TILE; ++j) {
        const int64_t ga = dpmx_ga(seed, i, j);
        int64_t n = 0;
        row_ok = datapath_mxgemm_quanta(tile[i * MI355X_DPMX_TILE + j], sa_i + b.sbase[j] - 257, &n) && row_ok;
        for (int v = 0; v < 2; ++v) {
          want[v] += ga * b.x[v][j];
          got[v] += n * b.x[v][j];
        }
      }
      if (row_ok && got[0] == want[0] && got[1] == want[1]) continue;
      for (uint32_t j = 0; j < MI355X_DPMX_TILE; ++j) {  // the whole row, to name and count its wrong words
        int64_t n = 0;
        for (uint32_t k = 0; k < b.K; ++k) n += au[k] * b.units[static_cast<size_t>(k) * MI355X_DPMX_TILE + j];
        const uint32_t word = dpbf_scaled_int(static_cast<int32_t>(dpmx_ga(seed, i, j) + 2 * n), sa_i + b.sbase[j] - 257);
        const uint32_t at = i * MI355X_DPMX_TILE + j;
        if (tile[at] != word) note(w, 3, w * MI355X_DPMX_WG_WORDS + at, tile[at], word);
      }
    }
    for (uint32_t v = 0; v < 4; ++v) {
      uint32_t want[6];
      datapath_mxgemm_wave_folds(b, fa, sfa, v, want);
      for (uint32_t stage = 0; stage < 3; ++stage)
        for (uint32_t xs = 0; xs < 2; ++xs) {
          const uint32_t got = r[dpmx_fold_slot(stage, v * 2u + xs)];
          if (got != want[stage * 2u + xs]) note(w, static_cast<int>(stage), w * 16u + v * 2u + xs, got, want[stage * 2u + xs]);
        }
    }
    if (bad_words() == before) ++out->records_ok;
  }
  out->mfma_bad = out->stage_bad[0] + out->stage_bad[1] + out->stage_bad[2];
  out->tile_bad = out->stage_bad[3];
  std::sort(cu_keys.begin(), cu_keys.end());
  out->cus_covered = static_cast<int>(std::unique(cu_keys.begin(), cu_keys.end()) - cu_keys.begin());
  std::sort(simd_keys.begin(), simd_keys.end());
  out->simds_covered = static_cast<int>(std::unique(simd_keys.begin(), simd_keys.end()) - simd_keys.begin());
  out->xccs_covered = __builtin_popcount(xmask);
  out->ok = out->records_ok == static_cast<int>(grid);
  if (out->ok) return;
  int n = std::snprintf(out->error, sizeof(out->error), "%d/%u workgroups exact (feed_bad=%u scale_bad=%u d_bad=%u)",
                        out->records_ok, grid, out->stage_bad[0] + out->stage_bad[1], out->stage_bad[2], out->tile_bad);
  if (out->first_bad_wg >= 0 && n > 0 && n < static_cast<int>(sizeof(out->error))) {
    const uint32_t x = out->first_bad_xor;
    n += std::snprintf(out->error + n, sizeof(out->error) - n, "; first bad: wg %d stage %d word %d xor 0x%08x",
                       out->first_bad_wg, out->first_bad_stage, out->first_bad_word, x);
    if ((x & (x - 1)) == 0 && n < static_cast<int>(sizeof(out->error)))
      std::snprintf(out->error + n, sizeof(out->error) - n, " (bit %d)", __builtin_ctz(x));
  }
}

}  // namespace mi355x
