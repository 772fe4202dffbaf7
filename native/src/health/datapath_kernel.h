// Shared between the gfx950 MFMA datapath kernel (mi355x_mfma_datapath), the
// host verdict (datapath_verify.h) and native/tests/datapath_contract_cli.cpp.
//
// The liveness tile uses small integers: a few low exponent values and the top
// mantissa bits. This check drives v_mfma_f32_32x32x2_f32 with operands whose
// words toggle all 32 bits, in four stages per wave, and every stage is exact
// by construction (every product and partial sum, in either k order, is a
// normal fp32; see docs/health.md), so the tile can be compared bit for bit:
//
//   stage 0  A = full-band words, B = +-2^f selecting one k per column, C = +0:
//            D[i][j] = A[i][j&1] * +-2^f_j    (A input path, every D bit)
//   stage 1  A = +-2^e selecting one k per row, B = full-band words, C = +0:
//            D[i][j] = +-2^e_i * B[i&1][j]    (B input path)
//   stage 2  A = al * 2^e_i, B = be * 2^f_j, C = ga * 2^(e_i + f_j) with signed
//            integers al, be == 1 (mod 4), |al|, |be| < 2^11, ga == 0 (mod 4),
//            0 < |ga| < 2^22: the sum is an integer below 2^24 at one common
//            scale (multiplier array, accumulate adder with cancellation); the
//            residues keep every partial sum non-zero (1, 1 and 2 mod 4)
//   stage 3  A = 0, B = full-band words, C = any sign, exponent field 1..254,
//            all mantissa bits: D = C        (C-in -> D-out, whole exponent range)
//
// "Full-band": any sign, all 23 mantissa bits, exponent field 97..158, so a
// product with 2^-90..2^90 stays normal. Both bands are closed under bitwise
// complement and word 1 of a full-band operand is the complement of word 0:
// every one of the 32 bits takes both values in A (stage 0), B (stage 1),
// C and D (stage 3) for every nonce, not just very probably.
#pragma once

#include <stdint.h>

#define MI355X_DP_THREADS 256
#define MI355X_DP_STAGES 4
#define MI355X_DP_M 32
#define MI355X_DP_N 32
#define MI355X_DP_K 2
#define MI355X_DP_TILE (MI355X_DP_M * MI355X_DP_N)
#define MI355X_DP_WG_WORDS (MI355X_DP_STAGES * MI355X_DP_TILE)  // tiles[wg][stage][32][32]
#define MI355X_DP_REC_WORDS 16
#define MI355X_DP_MAGIC 0x44505448u /* "DPTH" */
// record words (one record per workgroup); 12..15 are written as zero
#define MI355X_DPREC_MAGIC 0
#define MI355X_DPREC_WG 1
#define MI355X_DPREC_NONCE 2   // nonce ^ wg
#define MI355X_DPREC_XCC 3
#define MI355X_DPREC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPREC_BAD 8     // 4 words: per stage, MFMA elements (all waves) differing from the VALU chain

// explicit kernel arguments (24 bytes; the kernel uses no hidden args)
struct mi355x_datapath_args {
  uint32_t* records;  // host-visible, grid * MI355X_DP_REC_WORDS
  uint32_t* tiles;    // host-visible, grid * MI355X_DP_WG_WORDS (wave 0's four tiles per workgroup)
  uint32_t nonce;
  uint32_t grid;      // workgroups launched; a workgroup beyond it writes nothing
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it):
  // one wrong accumulator word after a stage's MFMA, before the comparison and
  // the tile store, so the tests can see ctr[stage] fire. Runtime arguments; an
  // index outside 0..63 does nothing. The fields mirror mi355x_sweep_args'.
  uint32_t inject_kind;   // MI355X_DP_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;   // 0..3
  uint32_t inject_lane;   // 0..63
  uint32_t inject_index;  // stage * 16 + accumulator register
  uint32_t inject_mask;   // xor-ed into that word
#endif
};

#define MI355X_DP_INJECT_NONE 0
#define MI355X_DP_INJECT_MFMA 1

#if defined(__HIPCC__)
#define MI355X_DP_HD __host__ __device__ inline
#else
#define MI355X_DP_HD static inline
#endif

// operand index spaces of dp_hash
#define MI355X_DP_IDX_A 0x0000u   // + i * 2 + k
#define MI355X_DP_IDX_B 0x0100u   // + k * 32 + j
#define MI355X_DP_IDX_C 0x1000u   // + i * 32 + j
#define MI355X_DP_IDX_ROW 0x2000u // + i: the row's power of two
#define MI355X_DP_IDX_COL 0x3000u // + j: the column's power of two

#define MI355X_DP_BAND_LO 97u     // full-band exponent field 97..158
#define MI355X_DP_POW_RANGE 90    // selector powers 2^-90..2^90
#define MI355X_DP_SCALE_RANGE 40  // stage 2 scales 2^-40..2^40

MI355X_DP_HD uint32_t dp_wave_nonce(uint32_t nonce, uint32_t wg, uint32_t wave) {
  return (nonce ^ (wg * 0x9E3779B1u)) + wave * 0x85EBCA77u;
}

MI355X_DP_HD uint32_t dp_hash(uint32_t nw, uint32_t stage, uint32_t idx) {
  uint32_t h = nw ^ ((stage + 1u) * 0x9E3779B1u) ^ (idx * 0x85EBCA77u);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

// A word with any sign and mantissa and an exponent field in lo..255-lo. Word
// `base + 1` is the complement of word `base`.
MI355X_DP_HD uint32_t dp_band_word(uint32_t nw, uint32_t stage, uint32_t base, uint32_t off, uint32_t lo) {
  const uint32_t h = dp_hash(nw, stage, base + (off == 1u ? 0u : off));
  const uint32_t e = lo + ((h >> 23) & 0xFFu) % (256u - 2u * lo);
  const uint32_t w = (h & 0x807FFFFFu) | (e << 23);
  return off == 1u ? ~w : w;
}

// +-2^p, p in -range..range
MI355X_DP_HD uint32_t dp_pow2_word(uint32_t h, int range) {
  const uint32_t e = 127u - (uint32_t)range + (h & 0x7FFFFFFFu) % (2u * (uint32_t)range + 1u);
  return (h & 0x80000000u) | (e << 23);
}

MI355X_DP_HD float dp_as_float(uint32_t w) {
  union {
    uint32_t u;
    float f;
  } v;
  v.u = w;
  return v.f;
}
MI355X_DP_HD uint32_t dp_as_word(float f) {
  union {
    uint32_t u;
    float f;
  } v;
  v.f = f;
  return v.u;
}

// stage 2: the signed odd integer of an operand, == 1 (mod 4), magnitude < 2^11
MI355X_DP_HD int dp_odd(uint32_t h) {
  const int neg = (int)(h >> 31);
  const int m = (int)(h & 0x7FCu) | (neg ? 3 : 1);
  return neg ? -m : m;
}
// stage 2: the row / column scale, a power of two
MI355X_DP_HD float dp_scale(uint32_t nw, uint32_t base, uint32_t off) {
  const uint32_t h = dp_hash(nw, 2u, base + off);
  return dp_as_float((127u - MI355X_DP_SCALE_RANGE + h % (2u * MI355X_DP_SCALE_RANGE + 1u)) << 23);
}

MI355X_DP_HD uint32_t dp_a_word(uint32_t stage, uint32_t i, uint32_t k, uint32_t nw) {
  switch (stage) {
    case 0:
      return dp_band_word(nw, 0u, MI355X_DP_IDX_A, i * 2u + k, MI355X_DP_BAND_LO);
    case 1:
      return k == (i & 1u) ? dp_pow2_word(dp_hash(nw, 1u, MI355X_DP_IDX_ROW + i), MI355X_DP_POW_RANGE) : 0u;
    case 2:
      return dp_as_word((float)dp_odd(dp_hash(nw, 2u, MI355X_DP_IDX_A + i * 2u + k)) *
                        dp_scale(nw, MI355X_DP_IDX_ROW, i));
    default:
      return 0u;
  }
}

MI355X_DP_HD uint32_t dp_b_word(uint32_t stage, uint32_t k, uint32_t j, uint32_t nw) {
  switch (stage) {
    case 0:
      return k == (j & 1u) ? dp_pow2_word(dp_hash(nw, 0u, MI355X_DP_IDX_COL + j), MI355X_DP_POW_RANGE) : 0u;
    case 2:
      return dp_as_word((float)dp_odd(dp_hash(nw, 2u, MI355X_DP_IDX_B + k * 32u + j)) *
                        dp_scale(nw, MI355X_DP_IDX_COL, j));
    default:
      return dp_band_word(nw, stage, MI355X_DP_IDX_B, k * 32u + j, MI355X_DP_BAND_LO);
  }
}

MI355X_DP_HD uint32_t dp_c_word(uint32_t stage, uint32_t i, uint32_t j, uint32_t nw) {
  switch (stage) {
    case 2: {
      const uint32_t h = dp_hash(nw, 2u, MI355X_DP_IDX_C + i * 32u + j);
      const int q = (int)(((h & 0x7FFFFFFFu) % 0xFFFFFu + 1u) << 2);  // 4 .. 2^22 - 4, == 0 (mod 4)
      return dp_as_word((float)((h >> 31) ? -q : q) * dp_scale(nw, MI355X_DP_IDX_ROW, i) *
                        dp_scale(nw, MI355X_DP_IDX_COL, j));
    }
    case 3:
      return dp_band_word(nw, 3u, MI355X_DP_IDX_C, i * 32u + j, 1u);
    default:
      return 0u;
  }
}
