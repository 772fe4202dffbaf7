// The verdict of the fused attention check: what the host decides from the
// records, the m / l words and the O words mi355x_mfma_datapath_attn wrote (shared
// by hsa_chip.cpp and native/tests/datapath_attn_contract_cli.cpp). Host only, no
// HSA: the caller owns the dispatches and hands over plain memory.
//
// Recomputing heads * qblocks * 128 * N * 64 products is too slow, so S comes from
// the three live terms (dpat_score's rule, on tables made once a head):
//   1. m and l are compared word for word;
//   2. every O word must be n * q_d with n an integer, |n| < 2^23;
//   3. the integers of a row are checked exactly by projection on two integer
//      vectors over d (all ones, and odd hash values) against
//      sum_j 2^(S_ij - m_i + 12) * (V x)_j, in int64_t; V x is made once a head;
//   4. only a failing row is recomputed in full, to name and count its wrong words;
//   5. each wave's folds are compared with the folds of the head's K and V.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "datapath_attn_kernel.h"
#include "datapath_gemm_verify.h"
#include "mi355x/liveness_probe.h"

namespace mi355x {

// what the host needs of one head: a per (query, pair), the live pairs and t per key, V's integers, V x, the folds
struct AttnHead {
  uint32_t seed, nq, nk;
  std::vector<int8_t> a;        // nq * 32
  std::vector<uint8_t> live;    // nk * 3
  std::vector<int8_t> t;        // nk * 3
  std::vector<int8_t> v;        // nk * 64: +-{1,2,3}
  std::vector<int64_t> vx[2];   // nk each: V's integers projected on the two vectors
  int32_t qx[MI355X_DPAT_D];    // log2 of the quantum of O's column d
  int64_t x[2][MI355X_DPAT_D];
  GemmFold fk, fv;

  AttnHead(uint32_t nonce, uint32_t head, uint32_t qblocks, uint32_t kblocks)
      : seed(dpat_head_seed(nonce, head)), nq(qblocks * MI355X_DPAT_QBLOCK), nk(kblocks * MI355X_DPAT_KBLOCK),
        a(static_cast<size_t>(nq) * 32), live(static_cast<size_t>(nk) * 3), t(static_cast<size_t>(nk) * 3),
        v(static_cast<size_t>(nk) * MI355X_DPAT_D) {
    for (uint32_t d = 0; d < MI355X_DPAT_D; ++d) {
      qx[d] = static_cast<int32_t>(dpat_ev(seed, d)) - 139;
      x[0][d] = 1;
      x[1][d] = static_cast<int64_t>((dpbf_hash(nonce, MI355X_DPAT_SPACE_X, d) & 0xFFu) | 1u);
    }
    for (uint32_t i = 0; i < nq; ++i)
      for (uint32_t p = 0; p < 32; ++p) a[i * 32 + p] = static_cast<int8_t>(dpat_a(seed, i, p));
    vx[0].assign(nk, 0);
    vx[1].assign(nk, 0);
    for (uint32_t j = 0; j < nk; ++j) {
      uint32_t lp[3];
      int32_t lt[3];
      dpat_live(seed, j, lp, lt);
      for (uint32_t e = 0; e < 3; ++e) {
        live[j * 3 + e] = static_cast<uint8_t>(lp[e]);
        t[j * 3 + e] = static_cast<int8_t>(lt[e]);
      }
      for (uint32_t p = 0; p < 32; ++p) {
        const uint32_t w = dpat_k_dword(nonce, seed, j, p);
        fk.add(static_cast<uint16_t>(w & 0xFFFFu));
        fk.add(static_cast<uint16_t>(w >> 16));
      }
      for (uint32_t d = 0; d < MI355X_DPAT_D; ++d) {
        const int32_t n = dpat_v_int(seed, j, d);
        v[j * MI355X_DPAT_D + d] = static_cast<int8_t>(n);
        vx[0][j] += n * x[0][d];
        vx[1][j] += n * x[1][d];
        fv.add(static_cast<uint16_t>(dpat_v_elem(seed, j, d)));
      }
    }
  }

  // S of (query, key): dpat_score, from the tables
  int32_t score(uint32_t i, uint32_t j) const {
    const int8_t* ai = &a[static_cast<size_t>(i) * 32];
    return ai[live[j * 3]] * t[j * 3] + ai[live[j * 3 + 1]] * t[j * 3 + 1] + ai[live[j * 3 + 2]] * t[j * 3 + 2];
  }
};

// the 16 fold words of a record: every wave reads the head's whole K and V
inline void datapath_attn_folds(const AttnHead& h, uint32_t* folds) {
  for (uint32_t v = 0; v < 4; ++v) {
    folds[v * 4 + 0] = h.fk.x;
    folds[v * 4 + 1] = h.fk.s;
    folds[v * 4 + 2] = h.fv.x;
    folds[v * 4 + 3] = h.fv.s;
  }
}

// the scores of query i of the head into s[nk]; returns their maximum
inline int32_t datapath_attn_scores(const AttnHead& h, uint32_t i, int32_t* s) {
  int32_t m = -64;
  for (uint32_t j = 0; j < h.nk; ++j) m = std::max(m, s[j] = h.score(i, j));
  return m;
}

// the m and l words and the 64 O words of a query whose scores are s[nk], maximum m
inline void datapath_attn_row(const AttnHead& h, const int32_t* s, int32_t m, uint32_t* ml, uint32_t* o) {
  int64_t l = 0, n[MI355X_DPAT_D] = {};
  for (uint32_t j = 0; j < h.nk; ++j) {
    const int64_t p = int64_t{1} << (s[j] - m + 12);
    l += p;
    for (uint32_t d = 0; d < MI355X_DPAT_D; ++d) n[d] += p * h.v[j * MI355X_DPAT_D + d];
  }
  ml[0] = dpat_word(m, 0);
  ml[1] = dpat_word(static_cast<int32_t>(l), -12);
  for (uint32_t d = 0; d < MI355X_DPAT_D; ++d) o[d] = dpat_word(static_cast<int32_t>(n[d]), h.qx[d]);
}

// the integer n of an O word got = n * 2^x, |n| < 2^23; +0 is 0. False for any other word.
inline bool datapath_attn_quanta(uint32_t got, int32_t x, int64_t* n) {
  if (got == 0u) return *n = 0, true;
  return datapath_gemm_quanta(got, x, n) && *n > -(int64_t{1} << 23) && *n < (int64_t{1} << 23);
}

// `records`: grid * MI355X_DPAT_REC_WORDS words, `ml`: grid * 256 words, `o`: grid * 8192 words, as the kernel left
// them. The caller has set out->nonce; every verdict field must be zero. stage_bad: wrong fold words of the K feed, of
// the V feed, wrong m / l words, wrong O words; mfma_bad is the feeds' sum, tile_bad the m / l and O words. records_ok
// counts exact workgroups; exp_inexact is the sum of the records' word, reported and not judged.
inline void datapath_attn_verdict(const uint32_t* records, const uint32_t* ml, const uint32_t* o, uint32_t heads,
                                  uint32_t qblocks, uint32_t kblocks, mi355x_datapath_attn_result* out) {
  const uint32_t nonce = out->nonce, grid = heads * qblocks;
  std::vector<uint32_t> cu_keys, simd_keys;
  std::vector<int32_t> s(kblocks * MI355X_DPAT_KBLOCK);
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
  const auto bad_total = [out] { return out->stage_bad[0] + out->stage_bad[1] + out->stage_bad[2] + out->stage_bad[3]; };
  for (uint32_t head = 0; head < heads; ++head) {
    const AttnHead h(nonce, head, qblocks, kblocks);
    uint32_t folds[16];
    datapath_attn_folds(h, folds);
    for (uint32_t qb = 0; qb < qblocks; ++qb) {
      const uint32_t wg = head * qblocks + qb, before = bad_total();
      const uint32_t* r = records + static_cast<size_t>(wg) * MI355X_DPAT_REC_WORDS;
      const bool here = r[MI355X_DPATREC_MAGIC] == MI355X_DPAT_MAGIC && r[MI355X_DPATREC_WG] == wg &&
                        r[MI355X_DPATREC_NONCE] == (nonce ^ wg) && r[MI355X_DPATREC_HEADS] == heads &&
                        r[MI355X_DPATREC_QBLOCKS] == qblocks && r[MI355X_DPATREC_KBLOCKS] == kblocks;
      if (!here) continue;
      const uint32_t xcc = r[MI355X_DPATREC_XCC] & 0xF;
      xmask |= 1u << xcc;
      cu_keys.push_back((xcc << 16) | ((r[MI355X_DPATREC_HWID] >> 8) & 0xFF));
      for (int v = 0; v < MI355X_DPAT_THREADS / 64; ++v) {
        const uint32_t hw = r[MI355X_DPATREC_HWID + v];
        simd_keys.push_back((xcc << 16) | (((hw >> 8) & 0xFF) << 2) | ((hw >> 4) & 0x3));
      }
      out->exp_inexact += r[MI355X_DPATREC_EXP_INEXACT];
      for (uint32_t word = 0; word < 8; ++word)
        for (uint32_t stage = 0; stage < 2; ++stage) {
          const uint32_t slot = dpat_fold_slot(stage, word);
          if (r[slot] != folds[slot - MI355X_DPATREC_FOLD])
            note(wg, static_cast<int>(stage), wg * 8 + word, r[slot], folds[slot - MI355X_DPATREC_FOLD]);
        }
      for (uint32_t qi = 0; qi < MI355X_DPAT_QBLOCK; ++qi) {
        const uint32_t* got_ml = ml + (static_cast<size_t>(wg) * MI355X_DPAT_QBLOCK + qi) * 2;
        const uint32_t* got_o = o + (static_cast<size_t>(wg) * MI355X_DPAT_QBLOCK + qi) * MI355X_DPAT_D;
        const int32_t m = datapath_attn_scores(h, qb * MI355X_DPAT_QBLOCK + qi, s.data());
        int64_t l = 0, want[2] = {0, 0}, got[2] = {0, 0};
        for (uint32_t j = 0; j < h.nk; ++j) {
          const int64_t p = int64_t{1} << (s[j] - m + 12);
          l += p;
          want[0] += p * h.vx[0][j];
          want[1] += p * h.vx[1][j];
        }
        const uint32_t want_ml[2] = {dpat_word(m, 0), dpat_word(static_cast<int32_t>(l), -12)};
        for (uint32_t e = 0; e < 2; ++e)
          if (got_ml[e] != want_ml[e]) note(wg, 2, wg * MI355X_DPAT_ML_WORDS + qi * 2 + e, got_ml[e], want_ml[e]);
        bool row_ok = true;
        for (uint32_t d = 0; d < MI355X_DPAT_D; ++d) {
          int64_t n = 0;
          row_ok = datapath_attn_quanta(got_o[d], h.qx[d], &n) && row_ok;
          got[0] += n * h.x[0][d];
          got[1] += n * h.x[1][d];
        }
        if (row_ok && got[0] == want[0] && got[1] == want[1]) continue;
        uint32_t full_ml[2], full_o[MI355X_DPAT_D];  // the whole row, to name and count its wrong words
        datapath_attn_row(h, s.data(), m, full_ml, full_o);
        for (uint32_t d = 0; d < MI355X_DPAT_D; ++d)
          if (got_o[d] != full_o[d]) note(wg, 3, wg * MI355X_DPAT_O_WORDS + qi * MI355X_DPAT_D + d, got_o[d], full_o[d]);
      }
      if (bad_total() == before) ++out->records_ok;
    }
  }
  out->mfma_bad = out->stage_bad[0] + out->stage_bad[1];
  out->tile_bad = out->stage_bad[2] + out->stage_bad[3];
  std::sort(cu_keys.begin(), cu_keys.end());
  out->cus_covered = static_cast<int>(std::unique(cu_keys.begin(), cu_keys.end()) - cu_keys.begin());
  std::sort(simd_keys.begin(), simd_keys.end());
  out->simds_covered = static_cast<int>(std::unique(simd_keys.begin(), simd_keys.end()) - simd_keys.begin());
  out->xccs_covered = __builtin_popcount(xmask);
  out->ok = out->records_ok == static_cast<int>(grid);
  if (out->ok) return;
  int n = std::snprintf(out->error, sizeof(out->error), "%d/%u workgroups exact (feed_bad=%u stat_bad=%u o_bad=%u)",
                        out->records_ok, grid, out->mfma_bad, out->stage_bad[2], out->stage_bad[3]);
  if (out->first_bad_wg >= 0 && n > 0 && n < static_cast<int>(sizeof(out->error))) {
    const uint32_t x = out->first_bad_xor;
    n += std::snprintf(out->error + n, sizeof(out->error) - n, "; first bad: workgroup %d stage %d word %d xor 0x%08x",
                       out->first_bad_wg, out->first_bad_stage, out->first_bad_word, x);
    if ((x & (x - 1)) == 0 && n < static_cast<int>(sizeof(out->error)))
      std::snprintf(out->error + n, sizeof(out->error) - n, " (bit %d)", __builtin_ctz(x));
  }
}

}  // namespace mi355x
