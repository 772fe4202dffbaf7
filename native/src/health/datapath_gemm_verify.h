// The verdict of the bf16 GEMM pipeline check: what the host decides from the
// records and D tiles mi355x_mfma_datapath_gemm wrote (shared by hsa_chip.cpp and
// native/tests/datapath_gemm_contract_cli.cpp). Host only, no HSA: the caller
// owns the dispatches and hands over plain memory.
//
// Recomputing grid * 128 * 128 * K products is seconds, so:
//   1. every D word must be n * q with n an integer, |n| < 2^24 (q is the
//      output's quantum, datapath_gemm_kernel.h); anything else is wrong at once;
//   2. the integers of a row are checked exactly by projection on two integer
//      vectors x with no zero entry (all ones, and odd hash values):
//        sum_j n_ij x_j == ga_i . x + sum_k a_ik (B x)_k        in int64_t
//      with B x computed once. One wrong word in a row always fails; several
//      cancel only if they do so for both vectors;
//   3. only a failing row is recomputed in full, to name and count its wrong words;
//   4. the folds of the fragments each wave read are compared with the folds of
//      the elements that should have arrived.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "datapath_gemm_kernel.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

// xor and sum modulo 2^32 over 16-bit elements
struct GemmFold {
  uint32_t x = 0, s = 0;
  void add(uint32_t elem) {
    x ^= elem;
    s += elem;
  }
};

// B as the fill writes it: elements [k][col], their integers in quanta, B x for the two vectors, the folds per column half
struct GemmB {
  uint32_t ksteps, K;
  std::vector<uint16_t> elem;
  std::vector<int16_t> units;
  std::vector<int64_t> bx[2];
  int64_t x[2][MI355X_DPGM_TILE];
  uint32_t eb[MI355X_DPGM_TILE];
  GemmFold fold[2];

  GemmB(uint32_t nonce, uint32_t ksteps_) : ksteps(ksteps_), K(ksteps_ * MI355X_DPGM_KSTEP) {
    elem.resize(static_cast<size_t>(K) * MI355X_DPGM_TILE);
    units.resize(elem.size());
    for (uint32_t j = 0; j < MI355X_DPGM_TILE; ++j) {
      eb[j] = dpgm_exp_field(nonce, MI355X_DPGM_SPACE_EB, j);
      x[0][j] = 1;
      x[1][j] = static_cast<int64_t>((dpbf_hash(nonce, MI355X_DPGM_SPACE_X, j) & 0xFFu) | 1u);
    }
    for (auto& v : bx) v.assign(K, 0);
    for (uint32_t k = 0; k < K; ++k)
      for (uint32_t j = 0; j < MI355X_DPGM_TILE; ++j) {
        const uint32_t e = dpgm_b_elem(nonce, k, j);
        const int32_t u = dpgm_units(e, eb[j]);
        elem[static_cast<size_t>(k) * MI355X_DPGM_TILE + j] = static_cast<uint16_t>(e);
        units[static_cast<size_t>(k) * MI355X_DPGM_TILE + j] = static_cast<int16_t>(u);
        fold[j >> 6].add(e);
        bx[0][k] += u * x[0][j];
        bx[1][k] += u * x[1][j];
      }
  }
};

// row `row` of A of the workgroup with seed `seed`: elements and their integers in quanta
inline void datapath_gemm_a_row(uint32_t seed, uint32_t ksteps, uint32_t row, uint16_t* elem, int16_t* units) {
  const uint32_t K = ksteps * MI355X_DPGM_KSTEP, ea = dpgm_exp_field(seed, MI355X_DPGM_SPACE_EA, row);
  for (uint32_t k = 0; k < K; k += 2) {
    const uint32_t w = dpgm_a_dword(seed, ksteps, row, k);
    elem[k] = static_cast<uint16_t>(w);
    elem[k + 1] = static_cast<uint16_t>(w >> 16);
    units[k] = static_cast<int16_t>(dpgm_units(w & 0xFFFFu, ea));
    units[k + 1] = static_cast<int16_t>(dpgm_units(w >> 16, ea));
  }
}

// n of a D word that is n * 2^qx with n an integer, |n| < 2^24; false for any other word
inline bool datapath_gemm_quanta(uint32_t word, int32_t qx, int64_t* n) {
  const int32_t e = static_cast<int32_t>((word >> 23) & 0xFFu);
  const int32_t down = qx - (e - 150);  // the significand, an integer of 24 bits, is in units of 2^(e-150)
  if (e == 0 || e == 255 || down < 0 || down > 23) return false;
  const int64_t sig = static_cast<int64_t>((word & 0x7FFFFFu) | 0x800000u);
  if (sig & ((int64_t{1} << down) - 1)) return false;
  *n = (word >> 31) ? -(sig >> down) : (sig >> down);
  return true;
}

// the word of n * 2^qx, 0 < |n| < 2^24
inline uint32_t datapath_gemm_word(int64_t n, int32_t qx) { return dpbf_scaled_int(static_cast<int32_t>(n), qx); }

// the image of a correct run of workgroup wg: its 128 x 128 D words and the 16 fold words of its record
inline void datapath_gemm_expected(const GemmB& b, uint32_t nonce, uint32_t wg, uint32_t* tile, uint32_t* folds) {
  const uint32_t seed = dpgm_wg_seed(nonce, wg);
  std::vector<uint16_t> ae(b.K);
  std::vector<int16_t> au(b.K);
  GemmFold fa[2];
  for (uint32_t i = 0; i < MI355X_DPGM_TILE; ++i) {
    datapath_gemm_a_row(seed, b.ksteps, i, ae.data(), au.data());
    int64_t n[MI355X_DPGM_TILE];
    for (uint32_t j = 0; j < MI355X_DPGM_TILE; ++j) n[j] = dpgm_ga(seed, i, j);
    for (uint32_t k = 0; k < b.K; ++k) {
      fa[i >> 6].add(ae[k]);
      const int16_t* bu = &b.units[static_cast<size_t>(k) * MI355X_DPGM_TILE];
      for (uint32_t j = 0; j < MI355X_DPGM_TILE; ++j) n[j] += au[k] * bu[j];
    }
    for (uint32_t j = 0; j < MI355X_DPGM_TILE; ++j)
      tile[i * MI355X_DPGM_TILE + j] = datapath_gemm_word(n[j], dpgm_qx(seed, nonce, i, j));
  }
  for (uint32_t v = 0; v < 4; ++v) {
    folds[v * 4 + 0] = (fa[v >> 1].x ^ (fa[v >> 1].x >> 16)) & 0xFFFFu;
    folds[v * 4 + 1] = fa[v >> 1].s;
    folds[v * 4 + 2] = b.fold[v & 1].x;
    folds[v * 4 + 3] = b.fold[v & 1].s;
  }
}

// `records`: grid * MI355X_DPGM_REC_WORDS words, `tiles`: grid *
// MI355X_DPGM_WG_WORDS words, as mi355x_mfma_datapath_gemm left them. The caller
// has set out->nonce; every verdict field must be zero. stage_bad: wrong fold
// words of the A feed, of the B feed, wrong D words; mfma_bad is the feeds' sum.
inline void datapath_gemm_verdict(const uint32_t* records, const uint32_t* tiles, uint32_t grid, uint32_t ksteps,
                                  mi355x_datapath_gemm_result* out) {
  const uint32_t nonce = out->nonce;
  const GemmB b(nonce, ksteps);
  std::vector<uint32_t> cu_keys, simd_keys;
  std::vector<uint16_t> ae(b.K);
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
  for (uint32_t w = 0; w < grid; ++w) {
    const uint32_t* r = records + static_cast<size_t>(w) * MI355X_DPGM_REC_WORDS;
    if (r[MI355X_DPGMREC_MAGIC] != MI355X_DPGM_MAGIC || r[MI355X_DPGMREC_WG] != w ||
        r[MI355X_DPGMREC_NONCE] != (nonce ^ w) || r[MI355X_DPGMREC_KSTEPS] != ksteps)
      continue;
    const uint32_t xcc = r[MI355X_DPGMREC_XCC] & 0xF;
    xmask |= 1u << xcc;
    cu_keys.push_back((xcc << 16) | ((r[MI355X_DPGMREC_HWID] >> 8) & 0xFF));
    for (int v = 0; v < MI355X_DPGM_THREADS / 64; ++v) {
      const uint32_t h = r[MI355X_DPGMREC_HWID + v];
      simd_keys.push_back((xcc << 16) | (((h >> 8) & 0xFF) << 2) | ((h >> 4) & 0x3));
    }
    const uint32_t before = out->stage_bad[0] + out->stage_bad[1] + out->stage_bad[2];
    const uint32_t seed = dpgm_wg_seed(nonce, w);
    const uint32_t* tile = tiles + static_cast<size_t>(w) * MI355X_DPGM_WG_WORDS;
    GemmFold fa[2];
    for (uint32_t i = 0; i < MI355X_DPGM_TILE; ++i) {
      datapath_gemm_a_row(seed, ksteps, i, ae.data(), au.data());
      int64_t want[2] = {0, 0}, got[2] = {0, 0};
      for (uint32_t k = 0; k < b.K; ++k) {
        fa[i >> 6].add(ae[k]);
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
        const uint32_t word = datapath_gemm_word(n, dpgm_qx(seed, nonce, i, j));
        if (tile[i * MI355X_DPGM_TILE + j] != word) note(w, 2, i * MI355X_DPGM_TILE + j, tile[i * MI355X_DPGM_TILE + j], word);
      }
    }
    for (uint32_t word = 0; word < 8; ++word)
      for (uint32_t stage = 0; stage < 2; ++stage) {
        const GemmFold& f = stage ? b.fold[(word >> 1) & 1] : fa[word >> 2];
        const uint32_t want = (word & 1) ? f.s : stage ? f.x : (f.x ^ (f.x >> 16)) & 0xFFFFu;
        const uint32_t got = r[dpgm_fold_slot(stage, word)];
        if (got != want) note(w, static_cast<int>(stage), word, got, want);
      }
    if (out->stage_bad[0] + out->stage_bad[1] + out->stage_bad[2] == before) ++out->records_ok;
  }
  out->mfma_bad = out->stage_bad[0] + out->stage_bad[1];
  out->tile_bad = out->stage_bad[2];
  std::sort(cu_keys.begin(), cu_keys.end());
  out->cus_covered = static_cast<int>(std::unique(cu_keys.begin(), cu_keys.end()) - cu_keys.begin());
  std::sort(simd_keys.begin(), simd_keys.end());
  out->simds_covered = static_cast<int>(std::unique(simd_keys.begin(), simd_keys.end()) - simd_keys.begin());
  out->xccs_covered = __builtin_popcount(xmask);
  out->ok = out->records_ok == static_cast<int>(grid);
  if (out->ok) return;
  int n = std::snprintf(out->error, sizeof(out->error), "%d/%u workgroups exact (feed_bad=%u tile_bad=%u)",
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
