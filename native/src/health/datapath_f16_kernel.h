// Shared between the gfx950 f16 MFMA datapath kernel (mi355x_mfma_datapath_f16),
// the host verdict (datapath_f16_verify.h) and
// native/tests/datapath_f16_contract_cli.cpp.
//
// The bf16 check (datapath_bf16_kernel.h) drives an 8-bit significand and the
// fp8 check (datapath_fp8_kernel.h) 4 bits at most. This one drives the IEEE
// half path: a decoder with a 5-bit exponent and a 10-bit mantissa, an 11 x 11
// bit significand multiplier, and four instructions -- the two pods mostly run,
// v_mfma_f32_32x32x16_f16 and v_mfma_f32_16x16x32_f16, and the 64-bit-operand
// forms of the previous generations, v_mfma_f32_32x32x8_f16 and
// v_mfma_f32_16x16x16_f16. Their summation order, tree shape and alignment are
// not documented; the operands are chosen so that every correct implementation
// must return the same bits.
//
// A lane hands the x16 / x32 forms four dwords (eight halves) of A and four of
// B, the legacy forms two dwords (four halves) each; element e of a fragment is
// half e&1 (0 = low) of dword e>>1:
//   32x32x16: lane l holds row / column l&31, k = 8*(l>>5) + e  (2 K-blocks)
//   16x16x32: lane l holds row / column l&15, k = 8*(l>>4) + e  (4 K-blocks)
//   32x32x8:  lane l holds row / column l&31, k = 4*(l>>5) + e  (2 K-blocks)
//   16x16x16: lane l holds row / column l&15, k = 4*(l>>4) + e  (4 K-blocks)
//   D[i][j] = C[i][j] + sum over k of A[i][k] * B[k][j]
// Only the pairing is assumed: half e of dword d of lane group h of A meets the
// same half of B. C and D use the maps every 32x32 / 16x16 f32 accumulator uses.
//
// An f16 normal is +-(1024+m) * 2^(E-25), m of 10 bits, E the exponent field.
// A "band half" has any sign, any 10 mantissa bits and E in 1..30: |x| in
// [2^-14, 2^16). The band is closed under 16-bit complement (E -> 31-E) and
// holds no zero, subnormal, Inf or NaN; nothing here depends on how the unit
// treats f16 subnormals. In a band fragment dword 1 is the complement of dword
// 0 and dword 3 of dword 2, so all 32 bits of the operand path take both values
// in every fragment, for every nonce.
// A "narrow" element is +-(32+m') * 2^(E-20), m' odd in 1..31: only the top five
// mantissa bits can be set and the lowest of those is. A "full odd" element is
// +-(1024+m) * 2^(E-25) with m odd.
//
//   stage 0  32x32x16  A = band halves; B = one-hot: column j holds +-2^f (E in
//            1..30, per column) at k = (j + rot) mod 16 and f16 +0 elsewhere;
//            C = +0. One product per output is not zero: D = +-A[i][k_j] * 2^f.
//   stage 1  32x32x16  A = one-hot per row, likewise; B = band halves; C = +0.
//   stage 2  32x32x16  as stage 0, but the hot element is a band half: D is the
//            exact 22-bit product of two 11-bit significands.
//   stage 3  32x32x16  A = full odd with the row's exponent field Ea_i; B =
//            narrow with the column's Eb_j; C = ga * q, q = 2^(Ea_i+Eb_j-45),
//            ga odd, |ga| < 2^21.
//   stage 4  16x16x32  A = narrow, B = full odd, C as stage 3: 32 terms.
//   stage 5  32x32x8   A = full odd (two dwords a lane), B = narrow, C as stage 3.
//   stage 6  16x16x16  A = narrow, B = full odd, C as stage 3.
//
// Why every stage is exact. Stages 0, 1 and 2 have one non-zero product per
// output; it needs at most 22 significant bits and its magnitude lies in
// [2^-28, 2^32), a normal f32: exact under any correct implementation
// whatsoever. In stages 3..6 every product is +-(1024+m)(32+m') q, an odd
// integer of at most 2047 * 63 < 2^17 times q. 16 terms stay below 2^21 q and 32
// below 2^22 q; with |C| < 2^21 q every partial sum, in every order and tree
// shape, is an integer multiple of q below 2^23 q < 2^24 q: it fits an f32
// significand, and a unit that keeps at least 24 significant bits below its
// largest term when it aligns loses nothing (the one assumption, the bf16
// check's). A partial sum may be zero; the final sum is an even count of odd
// terms plus the odd ga, so it is odd and not zero. q lies in 2^-43..2^15: no
// subnormal, no overflow.
//
// No output word of any stage is zero -- stages 0..2: a band half times a band
// half or a power of two; stages 3..6: an odd multiple of q -- so no signed-zero
// question arises in D. C-in to D-out over the whole exponent range stays with
// the f32, int8 and bf16 checks, and so does a stuck-at-0 in bit 0 of D, which
// neither a 22-bit product nor an odd sum below 2^23 q sets (bit 1 needs a sum
// of 2^22 q or more).
//
// The same argument makes a k-ordered f32 fmaf chain over the widened operands
// exact. The halves are widened by integer arithmetic (sign << 31 |
// (E + 112) << 23 | m << 13; +0 stays +0), not by a conversion instruction:
// the kernel's on-device comparison and the host's recomputation both use the
// chain, and compare words, not floats.
#pragma once

#include <stdint.h>

#define MI355X_DPHF_THREADS 256
#define MI355X_DPHF_STAGES 7
#define MI355X_DPHF_WIDE_STAGES 4                  // stages 0..3: 32x32x16, a 32x32 tile each
#define MI355X_DPHF_TILE 1024                      // words of a 32x32 tile
#define MI355X_DPHF_TILE16 256                     // words of a 16x16 tile (stages 4 and 6)
#define MI355X_DPHF_WG_WORDS (5 * MI355X_DPHF_TILE + 2 * MI355X_DPHF_TILE16)
#define MI355X_DPHF_REC_WORDS 16
#define MI355X_DPHF_MAGIC 0x44504846u /* "DPHF" */
// record words (one record per workgroup); 15 is written as zero
#define MI355X_DPHFREC_MAGIC 0
#define MI355X_DPHFREC_WG 1
#define MI355X_DPHFREC_NONCE 2   // nonce ^ wg
#define MI355X_DPHFREC_XCC 3
#define MI355X_DPHFREC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPHFREC_BAD 8     // 7 words: per stage, MFMA elements (all waves) differing from the recomputation

// explicit kernel arguments (24 bytes; the kernel uses no hidden args)
struct mi355x_datapath_f16_args {
  uint32_t* records;  // host-visible, grid * MI355X_DPHF_REC_WORDS
  uint32_t* tiles;    // host-visible, grid * MI355X_DPHF_WG_WORDS (wave 0's seven tiles per workgroup)
  uint32_t nonce;
  uint32_t grid;      // workgroups launched; a workgroup beyond it writes nothing
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it):
  // one wrong accumulator word after a stage's MFMA, before the comparison and
  // the tile store. Runtime arguments; an index that names no accumulator
  // register does nothing. The fields mirror mi355x_datapath_bf16_args'.
  uint32_t inject_kind;   // MI355X_DPHF_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;   // 0..3
  uint32_t inject_lane;   // 0..63
  uint32_t inject_index;  // stage * 16 + accumulator register (stages 4 and 6 have registers 0..3)
  uint32_t inject_mask;   // xor-ed into that word
#endif
};

#define MI355X_DPHF_INJECT_NONE 0
#define MI355X_DPHF_INJECT_MFMA 1

#if defined(__HIPCC__)
#define MI355X_DPHF_HD __host__ __device__ inline
#else
#define MI355X_DPHF_HD static inline
#endif

// operand index spaces of dphf_hash
#define MI355X_DPHF_IDX_A 0x0000u    // + (row * 4 + block) * 4 + dword
#define MI355X_DPHF_IDX_B 0x1000u    // + (col * 4 + block) * 4 + dword
#define MI355X_DPHF_IDX_C 0x2000u    // + row * 32 + col
#define MI355X_DPHF_IDX_HOT 0x3000u  // + row / col of a one-hot operand: the hot element
#define MI355X_DPHF_IDX_ROT 0x3800u  // low 4 bits: the rotation of the one-hot positions
#define MI355X_DPHF_IDX_EA 0x3900u   // + row: the row's exponent field in stages 3..6
#define MI355X_DPHF_IDX_EB 0x3A00u   // + col: the column's

#define MI355X_DPHF_BAND_LO 1u       // exponent fields of a band half: 1..30
#define MI355X_DPHF_BAND_N 30u

// K-blocks (lane groups) of a fragment, dwords a lane holds, rows / columns of the tile
MI355X_DPHF_HD uint32_t dphf_blocks(uint32_t stage) { return (stage == 4u || stage == 6u) ? 4u : 2u; }
MI355X_DPHF_HD uint32_t dphf_dwords(uint32_t stage) { return stage >= 5u ? 2u : 4u; }
MI355X_DPHF_HD uint32_t dphf_dim(uint32_t stage) { return (stage == 4u || stage == 6u) ? 16u : 32u; }
MI355X_DPHF_HD uint32_t dphf_tile_offset(uint32_t stage) {
  return stage * MI355X_DPHF_TILE - (stage > 4u ? MI355X_DPHF_TILE - MI355X_DPHF_TILE16 : 0u);
}
// stages 3 and 5: A full odd, B narrow; stages 4 and 6: the roles swapped
MI355X_DPHF_HD uint32_t dphf_a_is_narrow(uint32_t stage) { return stage == 4u || stage == 6u; }

MI355X_DPHF_HD uint32_t dphf_wave_nonce(uint32_t nonce, uint32_t wg, uint32_t wave) {
  return (nonce ^ (wg * 0x9E3779B1u)) + wave * 0x85EBCA77u;
}

MI355X_DPHF_HD uint32_t dphf_hash(uint32_t nw, uint32_t stage, uint32_t idx) {
  uint32_t h = nw ^ ((stage + 0x51u) * 0x9E3779B1u) ^ (idx * 0x85EBCA77u);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

// a 16-bit hash value as a band half: sign and mantissa kept, the 5 exponent
// bits scaled onto 1..30
MI355X_DPHF_HD uint32_t dphf_band16(uint32_t h16) {
  const uint32_t e = MI355X_DPHF_BAND_LO + ((((h16 >> 10) & 0x1Fu) * MI355X_DPHF_BAND_N) >> 5);
  return (h16 & 0x83FFu) | (e << 10);
}

// band halves: dword 1 is the complement of dword 0, dword 3 of dword 2
MI355X_DPHF_HD uint32_t dphf_band_word(uint32_t nw, uint32_t stage, uint32_t base, uint32_t rc, uint32_t block,
                                       uint32_t dword) {
  const uint32_t h = dphf_hash(nw, stage, base + (rc * 4u + block) * 4u + (dword & 2u));
  const uint32_t w = dphf_band16(h & 0xFFFFu) | (dphf_band16(h >> 16) << 16);
  return (dword & 1u) ? ~w : w;
}

// the k position (0..15) of the hot element of row / column rc
MI355X_DPHF_HD uint32_t dphf_onehot_pos(uint32_t nw, uint32_t stage, uint32_t rc) {
  return (rc + (dphf_hash(nw, stage, MI355X_DPHF_IDX_ROT) & 15u)) & 15u;
}

// the hot element: +-2^f with exponent field 1..30 (stages 0 and 1), a band half (stage 2)
MI355X_DPHF_HD uint32_t dphf_onehot_half(uint32_t nw, uint32_t stage, uint32_t rc) {
  const uint32_t h = dphf_hash(nw, stage, MI355X_DPHF_IDX_HOT + rc);
  if (stage == 2u) return dphf_band16(h >> 16);
  return ((h >> 31) << 15) | ((MI355X_DPHF_BAND_LO + (h & 0xFFFFu) % MI355X_DPHF_BAND_N) << 10);
}

// one-hot over the 16 k positions of a 32x32x16 fragment: the hot element at
// k = (rc + rot) mod 16 (block k>>3, element k&7), f16 +0 elsewhere
MI355X_DPHF_HD uint32_t dphf_onehot_word(uint32_t nw, uint32_t stage, uint32_t rc, uint32_t block, uint32_t dword) {
  const uint32_t pos = dphf_onehot_pos(nw, stage, rc);
  if ((pos >> 1) != block * 4u + dword) return 0u;
  return dphf_onehot_half(nw, stage, rc) << (16u * (pos & 1u));
}

// stages 3..6: the exponent field of a row / column
MI355X_DPHF_HD uint32_t dphf_exp_field(uint32_t nw, uint32_t stage, uint32_t base, uint32_t rc) {
  return MI355X_DPHF_BAND_LO + dphf_hash(nw, stage, base + rc) % MI355X_DPHF_BAND_N;
}

// two full odd elements +-(1024+m) * 2^(E-25), m odd, or two narrow ones
// +-(32+m') * 2^(E-20), m' odd (mantissa bits 5..9, bit 5 set)
MI355X_DPHF_HD uint32_t dphf_odd_word(uint32_t nw, uint32_t stage, uint32_t base, uint32_t rc, uint32_t block,
                                      uint32_t dword, uint32_t e, uint32_t narrow) {
  const uint32_t h = dphf_hash(nw, stage, base + (rc * 4u + block) * 4u + dword);
  const uint32_t w = narrow ? ((h & 0x83E083E0u) | 0x00200020u) : ((h & 0x83FF83FFu) | 0x00010001u);
  return w | (e << 10) | (e << 26);
}

MI355X_DPHF_HD uint32_t dphf_a_word(uint32_t stage, uint32_t row, uint32_t block, uint32_t dword, uint32_t nw) {
  if (stage == 1u) return dphf_onehot_word(nw, 1u, row, block, dword);
  if (stage == 0u || stage == 2u) return dphf_band_word(nw, stage, MI355X_DPHF_IDX_A, row, block, dword);
  return dphf_odd_word(nw, stage, MI355X_DPHF_IDX_A, row, block, dword,
                       dphf_exp_field(nw, stage, MI355X_DPHF_IDX_EA, row), dphf_a_is_narrow(stage));
}

MI355X_DPHF_HD uint32_t dphf_b_word(uint32_t stage, uint32_t col, uint32_t block, uint32_t dword, uint32_t nw) {
  if (stage == 0u || stage == 2u) return dphf_onehot_word(nw, stage, col, block, dword);
  if (stage == 1u) return dphf_band_word(nw, 1u, MI355X_DPHF_IDX_B, col, block, dword);
  return dphf_odd_word(nw, stage, MI355X_DPHF_IDX_B, col, block, dword,
                       dphf_exp_field(nw, stage, MI355X_DPHF_IDX_EB, col), !dphf_a_is_narrow(stage));
}

// the f32 bit pattern of ga * 2^x for an odd ga, 0 < |ga| < 2^21: built from
// integers (normalise, then place the exponent), the same on host and device
MI355X_DPHF_HD uint32_t dphf_scaled_int(int32_t ga, int32_t x) {
  const uint32_t sign = ga < 0 ? 0x80000000u : 0u;
  const uint32_t mag = static_cast<uint32_t>(ga < 0 ? -ga : ga);
  const uint32_t top = 31u - static_cast<uint32_t>(__builtin_clz(mag));  // position of the leading one
  return sign | (static_cast<uint32_t>(127 + static_cast<int32_t>(top) + x) << 23) | ((mag << (23u - top)) & 0x7FFFFFu);
}

MI355X_DPHF_HD uint32_t dphf_c_word(uint32_t stage, uint32_t row, uint32_t col, uint32_t nw) {
  if (stage < 3u) return 0u;
  const uint32_t h = dphf_hash(nw, stage, MI355X_DPHF_IDX_C + row * 32u + col);
  const int32_t mag = static_cast<int32_t>((h & 0x1FFFFFu) | 1u);  // odd, < 2^21
  const int32_t x = static_cast<int32_t>(dphf_exp_field(nw, stage, MI355X_DPHF_IDX_EA, row) +
                                         dphf_exp_field(nw, stage, MI355X_DPHF_IDX_EB, col)) - 45;
  return dphf_scaled_int((h >> 31) ? -mag : mag, x);
}

// element `half` (0 = low) of a fragment dword, widened to the f32 with the
// same value by integer arithmetic: a normal half +-(1024+m) * 2^(E-25) becomes
// sign, exponent field E + 112, mantissa m << 13; +-0 stays +-0. The recipe
// holds no subnormal, Inf or NaN.
MI355X_DPHF_HD uint32_t dphf_widen(uint32_t word, uint32_t half) {
  const uint32_t h = half ? (word >> 16) : (word & 0xFFFFu);
  const uint32_t sign = (h & 0x8000u) << 16;
  if ((h & 0x7FFFu) == 0u) return sign;
  return sign | ((((h >> 10) & 0x1Fu) + 112u) << 23) | ((h & 0x3FFu) << 13);
}
