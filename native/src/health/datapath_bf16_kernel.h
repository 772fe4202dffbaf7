// Shared between the gfx950 bf16 MFMA datapath kernel (mi355x_mfma_datapath_bf16),
// the host verdict (datapath_bf16_verify.h) and
// native/tests/datapath_bf16_contract_cli.cpp.
//
// The f32 check (datapath_kernel.h) drives the one-VGPR form and the int8 check
// (datapath_i8_kernel.h) the wide integer form. This one drives the two
// instructions pods mostly run, v_mfma_f32_32x32x16_bf16 and
// v_mfma_f32_16x16x32_bf16, whose internal summation order, tree shape and
// alignment are not documented -- with operands chosen so that every correct
// implementation must return the same bits.
//
// A lane hands the instruction four dwords (eight bf16) of A and four of B;
// element e = 0..7 of a fragment is half e&1 (0 = low) of dword e>>1:
//   32x32x16: lane l holds row / column l&31, k = 8*(l>>5) + e  (2 K-blocks)
//   16x16x32: lane l holds row / column l&15, k = 8*(l>>4) + e  (4 K-blocks)
//   D[i][j] = C[i][j] + sum over k of A[i][k] * B[k][j]
//
// A bf16 "band word" is a 16-bit pattern with any sign, exponent field 97..158
// and any 7 mantissa bits: |x| in [2^-30, 2^32). The band is closed under
// 16-bit complement (exponent e -> 255-e) and holds no zero, subnormal, Inf or
// NaN. In a band fragment dword 1 is the complement of dword 0 and dword 3 of
// dword 2, so all 32 bits of the operand path take both values in every
// fragment, for every nonce.
//
//   stage 0  32x32x16  A = band words; B = one-hot: column j holds +-2^f (f in
//            -90..90, per column) at k = (j + rot) mod 16 and bf16 +0 elsewhere;
//            C = +0. One product per output is not zero: D = +-A[i][k_j] * 2^f,
//            an 8-bit significand with exponent in -120..122, a normal f32.
//   stage 1  32x32x16  A = one-hot per row, likewise; B = band words; C = +0.
//   stage 2  32x32x16  A[i][k] = +-(128+m) * 2^(Ea_i-134), m odd in 1..127 per
//            element, Ea_i the row's exponent field (97..158); B[k][j] =
//            +-(128+m') * 2^(Eb_j-134) likewise per column; C = ga * q with
//            q = 2^(Ea_i+Eb_j-268), ga odd, |ga| < 2^20.
//   stage 3  32x32x16  A = bf16 +0; B = band words; C = any sign, exponent field
//            1..254, 23 mantissa bits, word 1 of each row the complement of
//            word 0 (the band 1..254 is closed under complement): every product
//            is a zero and C is not, so D = C, all 32 bits.
//   stage 4  16x16x32  as stage 2 with 32 terms.
//
// Why stages 2 and 4 are exact. Every product is +-(128+m)(128+m') q: an odd
// integer in [129^2, 255^2] times q, exact in 16 bits. C and all 16 (32)
// products are integer multiples of q below 2^20 q (products below 2^16 q), so
// in every summation order and tree shape every partial sum is an integer
// multiple of q below 2^21 q (stage 4: 2^22 q) < 2^24 q: it fits an f32
// significand, and a unit that keeps at least 24 significant bits below its
// largest term when it aligns loses nothing. A partial sum may be zero; the
// final sum is an odd number of q (an even count of odd products plus the odd
// ga), so it is not zero. q lies in 2^-74..2^48: no subnormal, no overflow.
// Stages 0, 1 and 3 have one non-zero term each and are exact under any
// correct implementation whatsoever.
//
// No output word of any stage is zero -- stage 0/1: a band word times a power
// of two; stage 2/4: an odd multiple of q; stage 3: C, whose exponent field is
// at least 1 -- so no signed-zero question arises in D.
//
// The same argument makes a k-ordered f32 fmaf chain over the widened operands
// (bf16 << 16) exact: the kernel's on-device comparison and the host's
// recomputation both use one, and compare words, not floats.
#pragma once

#include <stdint.h>

#define MI355X_DPBF_THREADS 256
#define MI355X_DPBF_STAGES 5
#define MI355X_DPBF_WIDE_STAGES 4                  // stages 0..3: 32x32x16, a 32x32 tile each
#define MI355X_DPBF_TILE 1024                      // words of a 32x32 tile
#define MI355X_DPBF_TILE16 256                     // words of the 16x16 tile of stage 4
#define MI355X_DPBF_WG_WORDS (MI355X_DPBF_WIDE_STAGES * MI355X_DPBF_TILE + MI355X_DPBF_TILE16)
#define MI355X_DPBF_REC_WORDS 16
#define MI355X_DPBF_MAGIC 0x44504246u /* "DPBF" */
// record words (one record per workgroup); 13..15 are written as zero
#define MI355X_DPBFREC_MAGIC 0
#define MI355X_DPBFREC_WG 1
#define MI355X_DPBFREC_NONCE 2   // nonce ^ wg
#define MI355X_DPBFREC_XCC 3
#define MI355X_DPBFREC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPBFREC_BAD 8     // 5 words: per stage, MFMA elements (all waves) differing from the recomputation

// explicit kernel arguments (24 bytes; the kernel uses no hidden args)
struct mi355x_datapath_bf16_args {
  uint32_t* records;  // host-visible, grid * MI355X_DPBF_REC_WORDS
  uint32_t* tiles;    // host-visible, grid * MI355X_DPBF_WG_WORDS (wave 0's five tiles per workgroup)
  uint32_t nonce;
  uint32_t grid;      // workgroups launched; a workgroup beyond it writes nothing
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it):
  // one wrong accumulator word after a stage's MFMA, before the comparison and
  // the tile store. Runtime arguments; an index that names no accumulator
  // register does nothing. The fields mirror mi355x_datapath_i8_args'.
  uint32_t inject_kind;   // MI355X_DPBF_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;   // 0..3
  uint32_t inject_lane;   // 0..63
  uint32_t inject_index;  // stage * 16 + accumulator register (stage 4 has registers 0..3)
  uint32_t inject_mask;   // xor-ed into that word
#endif
};

#define MI355X_DPBF_INJECT_NONE 0
#define MI355X_DPBF_INJECT_MFMA 1

#if defined(__HIPCC__)
#define MI355X_DPBF_HD __host__ __device__ inline
#else
#define MI355X_DPBF_HD static inline
#endif

// operand index spaces of dpbf_hash
#define MI355X_DPBF_IDX_A 0x0000u    // + (row * 4 + block) * 4 + dword
#define MI355X_DPBF_IDX_B 0x1000u    // + (col * 4 + block) * 4 + dword
#define MI355X_DPBF_IDX_C 0x2000u    // + row * 32 + col
#define MI355X_DPBF_IDX_SIGN 0x3000u // + row / col of a one-hot operand: bit 31 = minus, low bits: f
#define MI355X_DPBF_IDX_ROT 0x3800u  // low 4 bits: the rotation of the one-hot positions
#define MI355X_DPBF_IDX_EA 0x3900u   // + row: the row's exponent field in stages 2 and 4
#define MI355X_DPBF_IDX_EB 0x3A00u   // + col: the column's

#define MI355X_DPBF_BAND_LO 97u      // exponent fields of a band word: 97..158
#define MI355X_DPBF_BAND_N 62u

MI355X_DPBF_HD uint32_t dpbf_blocks(uint32_t stage) { return stage == 4u ? 4u : 2u; }
MI355X_DPBF_HD uint32_t dpbf_dim(uint32_t stage) { return stage == 4u ? 16u : 32u; }
MI355X_DPBF_HD uint32_t dpbf_tile_offset(uint32_t stage) { return stage * MI355X_DPBF_TILE; }

MI355X_DPBF_HD uint32_t dpbf_wave_nonce(uint32_t nonce, uint32_t wg, uint32_t wave) {
  return (nonce ^ (wg * 0x9E3779B1u)) + wave * 0x85EBCA77u;
}

MI355X_DPBF_HD uint32_t dpbf_hash(uint32_t nw, uint32_t stage, uint32_t idx) {
  uint32_t h = nw ^ ((stage + 0x21u) * 0x9E3779B1u) ^ (idx * 0x85EBCA77u);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

// a 16-bit hash value as a band word: sign and mantissa kept, the 8 exponent
// bits scaled onto 97..158
MI355X_DPBF_HD uint32_t dpbf_band16(uint32_t h16) {
  const uint32_t e = MI355X_DPBF_BAND_LO + ((((h16 >> 7) & 0xFFu) * MI355X_DPBF_BAND_N) >> 8);
  return (h16 & 0x807Fu) | (e << 7);
}

// band words: dword 1 is the complement of dword 0, dword 3 of dword 2
MI355X_DPBF_HD uint32_t dpbf_band_word(uint32_t nw, uint32_t stage, uint32_t base, uint32_t rc, uint32_t block,
                                       uint32_t dword) {
  const uint32_t h = dpbf_hash(nw, stage, base + (rc * 4u + block) * 4u + (dword & 2u));
  const uint32_t w = dpbf_band16(h & 0xFFFFu) | (dpbf_band16(h >> 16) << 16);
  return (dword & 1u) ? ~w : w;
}

// one-hot over the 16 k positions of a 32x32x16 fragment: row / column rc has
// +-2^f at k = (rc + rot) mod 16 (block k>>3, element k&7), bf16 +0 elsewhere
MI355X_DPBF_HD uint32_t dpbf_onehot_word(uint32_t nw, uint32_t stage, uint32_t rc, uint32_t block, uint32_t dword) {
  const uint32_t pos = (rc + (dpbf_hash(nw, stage, MI355X_DPBF_IDX_ROT) & 15u)) & 15u;
  if ((pos >> 1) != block * 4u + dword) return 0u;
  const uint32_t h = dpbf_hash(nw, stage, MI355X_DPBF_IDX_SIGN + rc);
  const uint32_t e = 127u - 90u + (h & 0xFFFFu) % 181u;  // 2^f, f = -90..90
  return (((h >> 31) << 15) | (e << 7)) << (16u * (pos & 1u));
}

// stages 2 and 4: two elements +-(128+m) * 2^(E-134), m odd, E the row's / column's exponent field
MI355X_DPBF_HD uint32_t dpbf_exp_field(uint32_t nw, uint32_t stage, uint32_t base, uint32_t rc) {
  return MI355X_DPBF_BAND_LO + dpbf_hash(nw, stage, base + rc) % MI355X_DPBF_BAND_N;
}

MI355X_DPBF_HD uint32_t dpbf_odd_word(uint32_t nw, uint32_t stage, uint32_t base, uint32_t rc, uint32_t block,
                                      uint32_t dword, uint32_t e) {
  const uint32_t h = dpbf_hash(nw, stage, base + (rc * 4u + block) * 4u + dword);
  return (h & 0x807F807Fu) | 0x00010001u | (e << 7) | (e << 23);
}

MI355X_DPBF_HD uint32_t dpbf_a_word(uint32_t stage, uint32_t row, uint32_t block, uint32_t dword, uint32_t nw) {
  if (stage == 1u) return dpbf_onehot_word(nw, 1u, row, block, dword);
  if (stage == 3u) return 0u;
  if (stage == 0u) return dpbf_band_word(nw, 0u, MI355X_DPBF_IDX_A, row, block, dword);
  return dpbf_odd_word(nw, stage, MI355X_DPBF_IDX_A, row, block, dword,
                       dpbf_exp_field(nw, stage, MI355X_DPBF_IDX_EA, row));
}

MI355X_DPBF_HD uint32_t dpbf_b_word(uint32_t stage, uint32_t col, uint32_t block, uint32_t dword, uint32_t nw) {
  if (stage == 0u) return dpbf_onehot_word(nw, 0u, col, block, dword);
  if (stage == 1u || stage == 3u) return dpbf_band_word(nw, stage, MI355X_DPBF_IDX_B, col, block, dword);
  return dpbf_odd_word(nw, stage, MI355X_DPBF_IDX_B, col, block, dword,
                       dpbf_exp_field(nw, stage, MI355X_DPBF_IDX_EB, col));
}

// the f32 bit pattern of ga * 2^x for an odd ga, 0 < |ga| < 2^20: built from
// integers (normalise, then place the exponent), the same on host and device
MI355X_DPBF_HD uint32_t dpbf_scaled_int(int32_t ga, int32_t x) {
  const uint32_t sign = ga < 0 ? 0x80000000u : 0u;
  const uint32_t mag = static_cast<uint32_t>(ga < 0 ? -ga : ga);
  const uint32_t top = 31u - static_cast<uint32_t>(__builtin_clz(mag));  // position of the leading one
  return sign | (static_cast<uint32_t>(127 + static_cast<int32_t>(top) + x) << 23) | ((mag << (23u - top)) & 0x7FFFFFu);
}

MI355X_DPBF_HD uint32_t dpbf_c_word(uint32_t stage, uint32_t row, uint32_t col, uint32_t nw) {
  if (stage == 2u || stage == 4u) {
    const uint32_t h = dpbf_hash(nw, stage, MI355X_DPBF_IDX_C + row * 32u + col);
    const int32_t mag = static_cast<int32_t>((h & 0xFFFFFu) | 1u);  // odd, < 2^20
    const int32_t x = static_cast<int32_t>(dpbf_exp_field(nw, stage, MI355X_DPBF_IDX_EA, row) +
                                           dpbf_exp_field(nw, stage, MI355X_DPBF_IDX_EB, col)) - 268;
    return dpbf_scaled_int((h >> 31) ? -mag : mag, x);
  }
  if (stage == 3u) {
    const uint32_t h = dpbf_hash(nw, 3u, MI355X_DPBF_IDX_C + row * 32u + (col == 1u ? 0u : col));
    // exponent field scaled onto 1..254, a band closed under complement
    const uint32_t w = (h & 0x807FFFFFu) | ((1u + ((((h >> 23) & 0xFFu) * 254u) >> 8)) << 23);
    return col == 1u ? ~w : w;
  }
  return 0u;
}

// element `half` (0 = low) of a fragment dword, widened to the f32 with the same value
MI355X_DPBF_HD uint32_t dpbf_widen(uint32_t word, uint32_t half) {
  return half ? (word & 0xFFFF0000u) : (word << 16);
}
