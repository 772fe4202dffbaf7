// Shared between the gfx950 f64 MFMA datapath kernel (mi355x_mfma_datapath_f64),
// the host verdict (datapath_f64_verify.h) and
// native/tests/datapath_f64_contract_cli.cpp.
//
// The f32, int8, bf16, fp8 and f16 checks leave the double-precision matrix
// path untouched: a 53 x 53 bit significand multiplier, an 11-bit exponent
// datapath, 64-bit operand and accumulator lanes, the 4-block form
// v_mfma_f64_4x4x4_4b_f64 and the three `neg` bits only the f64 forms have.
// This check drives v_mfma_f64_16x16x4_f64 (what DGEMM runs) and
// v_mfma_f64_4x4x4_4b_f64. Their summation order, tree shape and alignment are
// not documented; the operands are chosen so that every correct implementation
// must return the same bits.
//
// A lane hands either form one double of A and one of B. Both are described
// here as 16 "rows" of A and 16 "columns" of B with 4 k positions each:
//   16x16x4:    lane l holds A[l&15][l>>4] and B[l&15][l>>4];
//               D[i][j] = C[i][j] + sum over k of A[i][k] * B[j][k];
//               accumulator double r of lane l is D[4*r + (l>>4)][l&15]
//   4x4x4_4b:   four independent 4x4x4 blocks b; row 4b+i of A and column 4b+j
//               of B belong to block b; lane l holds A[l&15][l>>4] and
//               B[l&15][l>>4] (i or j = l&3, b = (l>>2)&3, k = l>>4);
//               D[b][i][j] = C + sum over k of A[4b+i][k] * B[4b+j][k],
//               held by lane 16i + 4b + j (dpd_4x4_* below)
// These are the maps an MI355X showed in the one-hot tiles of stages 0 and 5;
// the recipe assumes them and nothing else about the unit's layout.
// A double is two words, the low one first. Nothing converts an integer or a
// float to a double: every operand is a bit pattern built by integer arithmetic.
//
// A normal double is +-(2^52+m) * 2^(E-1075), m of 52 bits, E the exponent field.
//   band double   any sign, any 52 mantissa bits, E in 512..1535. The band is
//                 closed under 64-bit complement (E -> 2047-E) and holds no
//                 zero, subnormal, Inf or NaN.
//   hot power     +-2^(E-1023), E in 513..1534 (stages 0, 1, 5).
//   wide double   as a band double with the low 26 mantissa bits zero: a 27-bit
//                 significand (stage 2's A).
//   hot 26        +-, E in 513..1533, the low 27 mantissa bits zero: a 26-bit
//                 significand (stage 2's B; the range is one short of the hot
//                 powers' because the significand product may carry).
//   odd 27 / 20   +-, the row's or column's exponent field E in 535..1511, an
//                 odd 27-bit (mantissa bit 26 set, none below) or odd 20-bit
//                 (bit 33 set, none below) significand.
//
//   stage 0  16x16x4   A = band doubles; B = one-hot: column j holds a hot
//            power at k = (j + rot) mod 4 and +0 elsewhere; C = +0. Two passes,
//            the second with all 64 bits of every band double complemented:
//            two tiles. D = +-A[i][k_j] * 2^f.
//   stage 1  16x16x4   A = one-hot per row, likewise; B = band doubles; C = +0;
//            two passes: two tiles.
//   stage 2  16x16x4   A = wide doubles; B = one-hot, the hot element a hot 26;
//            C = +0: one tile. D is the exact product, of up to 53 bits.
//   stage 3  16x16x4   A = odd 27 with the row's exponent Ea_i; B = odd 20 with
//            the column's Eb_j; C = ga * q, q = 2^((Ea_i-1023)+(Eb_j-1023)-45),
//            ga odd, |ga| < 2^49: one tile.
//   stage 4  16x16x4   operands as stage 3 (hashed under stage 4); three
//            independent MFMAs with neg:[1,0,0], [0,1,0] and [0,0,1]
//            (blgp 1, 2, 4): -A.B+C, -A.B+C and A.B-C: three tiles.
//   stage 5  4x4x4_4b  as stage 0 (one-hot position (j + rot) mod 4 within the
//            block), two passes: two tiles of 64 doubles.
//   stage 6  4x4x4_4b  as stage 3: one tile of 64 doubles.
//
// Why every stage is exact. Stages 0, 1, 2 and 5 have one non-zero product per
// output. A band double times a hot power keeps the 53-bit significand and has
// the exponent field Ea + Ef - 1023 in 2..2046; a 27-bit times a 26-bit
// significand has at most 53 bits and the field Ea + Ef - 1023 (+1 on a carry)
// in 2..2046: a normal double, exact under any correct implementation
// whatsoever. The complemented pass of stages 0, 1 and 5 makes every one of
// the 64 bits of the A path (stage 0, 5) and of the B path (stage 1) take both
// values in every lane, for every nonce, and complements sign and mantissa of
// every output, so D's 52 mantissa bits and its sign take both values in every
// accumulator register; the 11 exponent bits of D take both values across a
// tile (E and its mirror 2047-E shifted by the hot power's). The recipe leaves
// no bit of D unset.
// In stages 3, 4 and 6 an odd 27 is sa * 2^(Ea-1023-26) and an odd 20 is
// sb * 2^(Eb-1023-19) with sa < 2^27 and sb < 2^20 odd: every product is an odd
// integer below 2^47 times q. Four products stay below 2^49 q and with
// |C| < 2^49 q every partial sum, in every order and tree shape, is an integer
// multiple of q below 2^50 q < 2^53 q: it fits a double's significand, and a
// unit that keeps at least 53 significant bits below its largest term when it
// aligns loses nothing (the one assumption, the bf16 and f16 checks' at 24
// bits). A partial sum may be zero; the final sum is an even count of odd terms
// plus the odd ga, so it is odd and not zero. The exponent of q lies in
// -1021..931 and 2^50 q below 2^982: no subnormal, no overflow.
//
// The same argument makes a k-ordered v_fma_f64 chain exact; the kernel
// compares its accumulator words with that chain, and stage 2's also with the
// integer product of the two significands, so that a fault common to the f64
// VALU and the MFMA multiplier does not hide. The host uses integers only.
#pragma once

#include <stdint.h>

#define MI355X_DPD_THREADS 256
#define MI355X_DPD_STAGES 7
#define MI355X_DPD_TILE 512                        // words of a 16x16 tile of doubles
#define MI355X_DPD_TILE4 128                       // words of a 4-block 4x4 tile (stages 5 and 6)
#define MI355X_DPD_WG_WORDS (9 * MI355X_DPD_TILE + 3 * MI355X_DPD_TILE4)
#define MI355X_DPD_REC_WORDS 16
#define MI355X_DPD_MAGIC 0x44504446u /* "DPDF" */
// record words (one record per workgroup); 15 is written as zero
#define MI355X_DPDREC_MAGIC 0
#define MI355X_DPDREC_WG 1
#define MI355X_DPDREC_NONCE 2   // nonce ^ wg
#define MI355X_DPDREC_XCC 3
#define MI355X_DPDREC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPDREC_BAD 8     // 7 words: per stage, accumulator words (all waves) differing from the recomputation

// explicit kernel arguments (24 bytes; the kernel uses no hidden args)
struct mi355x_datapath_f64_args {
  uint32_t* records;  // host-visible, grid * MI355X_DPD_REC_WORDS
  uint32_t* tiles;    // host-visible, grid * MI355X_DPD_WG_WORDS (wave 0's twelve tiles per workgroup)
  uint32_t nonce;
  uint32_t grid;      // workgroups launched; a workgroup beyond it writes nothing
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it):
  // one wrong accumulator word after a stage's MFMAs, before the comparison and
  // the tile store. Runtime arguments; an index that names no accumulator
  // word does nothing. The fields mirror mi355x_datapath_f16_args'.
  uint32_t inject_kind;   // MI355X_DPD_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;   // 0..3
  uint32_t inject_lane;   // 0..63
  uint32_t inject_index;  // stage * 32 + accumulator word: (tile * doubles a lane holds + double) * 2 + high
  uint32_t inject_mask;   // xor-ed into that word
#endif
};

#define MI355X_DPD_INJECT_NONE 0
#define MI355X_DPD_INJECT_MFMA 1

#if defined(__HIPCC__)
#define MI355X_DPD_HD __host__ __device__ inline
#else
#define MI355X_DPD_HD static inline
#endif

// operand index spaces of dpd_hash
#define MI355X_DPD_IDX_A 0x0000u    // + (row * 4 + k) * 2 + word
#define MI355X_DPD_IDX_B 0x1000u    // + (col * 4 + k) * 2 + word
#define MI355X_DPD_IDX_C 0x2000u    // + (row * 16 + col) * 2 + word
#define MI355X_DPD_IDX_HOT 0x3000u  // + (row / col of a one-hot operand) * 2 + word: the hot element
#define MI355X_DPD_IDX_ROT 0x3800u  // low 2 bits: the rotation of the one-hot positions
#define MI355X_DPD_IDX_EA 0x3900u   // + row: the row's exponent field in stages 3, 4, 6
#define MI355X_DPD_IDX_EB 0x3A00u   // + col: the column's

#define MI355X_DPD_BAND_LO 512u     // exponent fields of a band double: 512..1535
#define MI355X_DPD_HOT_LO 513u      // of a hot power: 513..1534; of stage 2's hot 26: 513..1533
#define MI355X_DPD_HOT_N 1022u
#define MI355X_DPD_SUM_LO 535u      // of a row or column of the sum stages: 535..1511
#define MI355X_DPD_SUM_N 977u

// tiles of a stage, doubles of a tile, the stage's first word among a workgroup's tile words
MI355X_DPD_HD uint32_t dpd_tiles(uint32_t stage) {
  return stage == 4u ? 3u : (stage == 0u || stage == 1u || stage == 5u) ? 2u : 1u;
}
MI355X_DPD_HD uint32_t dpd_is_4x4(uint32_t stage) { return stage >= 5u; }
MI355X_DPD_HD uint32_t dpd_tile_doubles(uint32_t stage) { return stage >= 5u ? 64u : 256u; }
MI355X_DPD_HD uint32_t dpd_stage_words(uint32_t stage) { return dpd_tiles(stage) * dpd_tile_doubles(stage) * 2u; }
MI355X_DPD_HD uint32_t dpd_tile_offset(uint32_t stage) {
  const uint32_t before = stage < 2u ? 2u * stage : stage < 5u ? stage + 2u : 9u;  // 16x16 tiles before the stage
  return before * MI355X_DPD_TILE + (stage == 6u ? 2u * MI355X_DPD_TILE4 : 0u);
}
// stages 0, 2, 5: A band or wide, B one-hot; stage 1: the roles swapped; 3, 4, 6: sums
MI355X_DPD_HD uint32_t dpd_is_sum(uint32_t stage) { return stage == 3u || stage == 4u || stage == 6u; }
// row of A and column of B behind double `d` of a tile
MI355X_DPD_HD uint32_t dpd_row_of(uint32_t stage, uint32_t d) {
  return dpd_is_4x4(stage) ? 4u * (d >> 4) + ((d >> 2) & 3u) : d >> 4;
}
MI355X_DPD_HD uint32_t dpd_col_of(uint32_t stage, uint32_t d) {
  return dpd_is_4x4(stage) ? 4u * (d >> 4) + (d & 3u) : d & 15u;
}

// the 4x4x4_4b lane map: the row of A / column of B and the k a lane feeds, and
// the double of the tile (16b + 4i + j) its accumulator holds
MI355X_DPD_HD uint32_t dpd_4x4_rc(uint32_t lane) { return lane & 15u; }
MI355X_DPD_HD uint32_t dpd_4x4_k(uint32_t lane) { return lane >> 4; }
MI355X_DPD_HD uint32_t dpd_4x4_d(uint32_t lane) { return 16u * ((lane >> 2) & 3u) + 4u * (lane >> 4) + (lane & 3u); }

MI355X_DPD_HD uint32_t dpd_wave_nonce(uint32_t nonce, uint32_t wg, uint32_t wave) {
  return (nonce ^ (wg * 0x9E3779B1u)) + wave * 0x85EBCA77u;
}

MI355X_DPD_HD uint32_t dpd_hash(uint32_t nw, uint32_t stage, uint32_t idx) {
  uint32_t h = nw ^ ((stage + 0x64u) * 0x9E3779B1u) ^ (idx * 0x85EBCA77u);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

MI355X_DPD_HD uint64_t dpd_pack(uint32_t hi, uint32_t lo) { return (static_cast<uint64_t>(hi) << 32) | lo; }

// a band double (stages 0, 1, 5; `flip`: the complemented pass) or a wide one
// (stage 2): sign and mantissa from two hash words, the 11 exponent bits halved
// onto 512..1535
MI355X_DPD_HD uint64_t dpd_band(uint32_t nw, uint32_t stage, uint32_t base, uint32_t rc, uint32_t k, uint32_t flip) {
  const uint32_t h = dpd_hash(nw, stage, base + (rc * 4u + k) * 2u);
  const uint32_t l = dpd_hash(nw, stage, base + (rc * 4u + k) * 2u + 1u);
  const uint32_t e = MI355X_DPD_BAND_LO + (((h >> 20) & 0x7FFu) >> 1);
  const uint64_t v = dpd_pack((h & 0x800FFFFFu) | (e << 20), stage == 2u ? (l & 0xFC000000u) : l);
  return flip ? ~v : v;
}

// the k position (0..3) of the hot element of row / column rc
MI355X_DPD_HD uint32_t dpd_onehot_pos(uint32_t nw, uint32_t stage, uint32_t rc) {
  return (rc + dpd_hash(nw, stage, MI355X_DPD_IDX_ROT)) & 3u;
}

// the hot element: a hot power, or stage 2's hot 26
MI355X_DPD_HD uint64_t dpd_hot(uint32_t nw, uint32_t stage, uint32_t rc) {
  const uint32_t h = dpd_hash(nw, stage, MI355X_DPD_IDX_HOT + rc * 2u);
  if (stage != 2u) return dpd_pack((h & 0x80000000u) | ((MI355X_DPD_HOT_LO + (h & 0xFFFFu) % MI355X_DPD_HOT_N) << 20), 0u);
  const uint32_t l = dpd_hash(nw, stage, MI355X_DPD_IDX_HOT + rc * 2u + 1u);
  const uint32_t e = MI355X_DPD_HOT_LO + ((h >> 20) & 0x7FFu) % (MI355X_DPD_HOT_N - 1u);
  return dpd_pack((h & 0x800FFFFFu) | (e << 20), l & 0xF8000000u);
}

MI355X_DPD_HD uint64_t dpd_onehot(uint32_t nw, uint32_t stage, uint32_t rc, uint32_t k) {
  return dpd_onehot_pos(nw, stage, rc) == k ? dpd_hot(nw, stage, rc) : 0u;
}

// the sum stages: the exponent field of a row / column
MI355X_DPD_HD uint32_t dpd_exp_field(uint32_t nw, uint32_t stage, uint32_t base, uint32_t rc) {
  return MI355X_DPD_SUM_LO + dpd_hash(nw, stage, base + rc) % MI355X_DPD_SUM_N;
}

// an odd 27 (mantissa bits 51..26, bit 26 set) or an odd 20 (bits 51..33, bit 33 set)
MI355X_DPD_HD uint64_t dpd_odd(uint32_t nw, uint32_t stage, uint32_t base, uint32_t rc, uint32_t k, uint32_t e,
                               uint32_t narrow) {
  const uint32_t h = dpd_hash(nw, stage, base + (rc * 4u + k) * 2u);
  if (narrow) return dpd_pack((h & 0x800FFFFCu) | 2u | (e << 20), 0u);
  return dpd_pack((h & 0x800FFFFFu) | (e << 20), ((h << 6) & 0xF8000000u) | 0x04000000u);
}

// A[row][k] and B[col][k] of `stage` as bit patterns; `pass` 1 complements the band operands
MI355X_DPD_HD uint64_t dpd_a_bits(uint32_t stage, uint32_t pass, uint32_t row, uint32_t k, uint32_t nw) {
  if (stage == 1u) return dpd_onehot(nw, 1u, row, k);
  if (!dpd_is_sum(stage)) return dpd_band(nw, stage, MI355X_DPD_IDX_A, row, k, pass);
  return dpd_odd(nw, stage, MI355X_DPD_IDX_A, row, k, dpd_exp_field(nw, stage, MI355X_DPD_IDX_EA, row), 0u);
}

MI355X_DPD_HD uint64_t dpd_b_bits(uint32_t stage, uint32_t pass, uint32_t col, uint32_t k, uint32_t nw) {
  if (stage == 1u) return dpd_band(nw, 1u, MI355X_DPD_IDX_B, col, k, pass);
  if (!dpd_is_sum(stage)) return dpd_onehot(nw, stage, col, k);
  return dpd_odd(nw, stage, MI355X_DPD_IDX_B, col, k, dpd_exp_field(nw, stage, MI355X_DPD_IDX_EB, col), 1u);
}

// the bit pattern of v * 2^x for 0 < |v| < 2^53: built from integers (normalise,
// then place the exponent), the same on host and device
MI355X_DPD_HD uint64_t dpd_scaled_int(int64_t v, int32_t x) {
  const uint64_t sign = v < 0 ? 0x8000000000000000ull : 0ull;
  const uint64_t mag = static_cast<uint64_t>(v < 0 ? -v : v);
  const uint32_t top = 63u - static_cast<uint32_t>(__builtin_clzll(mag));  // position of the leading one
  return sign | (static_cast<uint64_t>(1023 + static_cast<int32_t>(top) + x) << 52) |
         ((mag << (52u - top)) & 0xFFFFFFFFFFFFFull);
}

// C[row][col]: +0, or ga * q in the sum stages
MI355X_DPD_HD uint64_t dpd_c_bits(uint32_t stage, uint32_t row, uint32_t col, uint32_t nw) {
  if (!dpd_is_sum(stage)) return 0u;
  const uint32_t h = dpd_hash(nw, stage, MI355X_DPD_IDX_C + (row * 16u + col) * 2u);
  const uint32_t l = dpd_hash(nw, stage, MI355X_DPD_IDX_C + (row * 16u + col) * 2u + 1u);
  const int64_t mag = static_cast<int64_t>(dpd_pack(h & 0x1FFFFu, l) | 1u);  // odd, < 2^49
  const int32_t x = static_cast<int32_t>(dpd_exp_field(nw, stage, MI355X_DPD_IDX_EA, row) +
                                         dpd_exp_field(nw, stage, MI355X_DPD_IDX_EB, col)) - 2046 - 45;
  return dpd_scaled_int((h >> 31) ? -mag : mag, x);
}

// what `neg` does in tile t of stage 4: the sign bit xor-ed into every A (tiles
// 0 and 1 both give -A.B+C, through neg A and through neg B) or into C (tile 2)
MI355X_DPD_HD uint64_t dpd_neg_ab(uint32_t stage, uint32_t t) { return (stage == 4u && t < 2u) ? 1ull << 63 : 0ull; }
MI355X_DPD_HD uint64_t dpd_neg_c(uint32_t stage, uint32_t t) { return (stage == 4u && t == 2u) ? 1ull << 63 : 0ull; }

// stage 2's output from the integer product of the 27-bit and the 26-bit
// significand: normalise the 52- or 53-bit product and place the exponent
MI355X_DPD_HD uint64_t dpd_wide_product(uint64_t a, uint64_t hot) {
  const uint64_t sa = (1ull << 26) | ((a >> 26) & 0x3FFFFFFull);
  const uint64_t sb = (1ull << 25) | ((hot >> 27) & 0x1FFFFFFull);
  const uint64_t p = sa * sb;  // in [2^51, 2^53)
  const uint32_t carry = static_cast<uint32_t>(p >> 52);
  const uint64_t e = ((a >> 52) & 0x7FFu) + ((hot >> 52) & 0x7FFu) - 1023u + carry;
  return ((a ^ hot) & 0x8000000000000000ull) | (e << 52) | ((carry ? p : p << 1) & 0xFFFFFFFFFFFFFull);
}
