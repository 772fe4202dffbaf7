// Shared between the gfx950 sparse (2:4) MFMA datapath kernel
// (mi355x_mfma_datapath_sparse), the host verdict (datapath_sparse_verify.h)
// and native/tests/datapath_sparse_contract_cli.cpp.
//
// The other datapath checks drive the dense v_mfma_* forms only. The sparse
// forms, v_smfmac_*, take a compressed A (two of every four K positions), a
// third register operand -- the index -- and a dense B; per group of four K
// positions the index steers a 4-to-2 selection in front of B. The index
// operand path, the selection muxes and the K-doubled sparse issue path of
// CDNA4 are hardware no dense instruction toggles. This check drives them with
// operands chosen so that every correct implementation must return the same
// bits.
//
// Fragments. A lane hands the instruction four dwords of compressed A, eight
// dwords of dense B and one index dword. With 16-bit data a lane holds 8
// compressed elements (4 groups, 16 index bits) and 16 dense elements of B;
// with 8-bit data 16 compressed elements (8 groups, 32 index bits) and 32 of B.
// Element e of a fragment is field e of its little-endian bit stream.
//   32x32: lane l holds row / column l&31 and lane group l>>5  (2 groups)
//   16x16: lane l holds row / column l&15 and lane group l>>4  (4 groups)
// KB = 16 (16-bit) or 32 (8-bit) dense K positions belong to a lane group, so
// K = 32 / 64 (16-bit) and 64 / 128 (8-bit).
//
// Measured on an MI355X (docs/health.md has the table and how it was read):
//   index   lane l's index register describes lane l's own compressed
//           elements: elements 2t and 2t+1 belong to group t of the lane's KB
//           positions, and their positions within the group are the 2-bit
//           fields idx[4t+1:4t] and idx[4t+3:4t+2]. As assumed.
//   abid    with 16 index bits and cbsz = 0, abid = 0 reads idx[15:0] and
//           abid = 1 reads idx[31:16]. As assumed. (With cbsz = 1 abid is
//           ignored and idx[15:0] is read; the check keeps cbsz = 0.) With 32
//           index bits abid changes nothing.
//   K       not as assumed. B is plain: element e of lane group h' is
//           k = KB*h' + e. A is interleaved in two runs of R = KB/2, as the
//           8-bit f8f6f4 fragments are: position p (0..KB-1, p = 4t + field) of
//           lane group h of A is
//             k = KB * (2*(h mod m) + p/R) + R * (h/m) + p mod R,   m = groups/2
//           so for 32x32 lane group h of A holds the runs [R*h, R*h+R) of both
//           halves of K, and for 16x16 lane groups h and h+2 share two KB
//           blocks. A group of four stays four consecutive k.
// The accumulator maps are the dense ones.
//
// Index pairs: only pairs with first < second are used, six per group:
// (0,1) (0,2) (0,3) (1,2) (1,3) (2,3). Pair number (row + offset of the group
// position) mod 6 makes every group position see all six pairs over any six
// consecutive rows of a tile. Stage 1's indices do not depend on the row; there
// the eight group positions take pair numbers (position + offset) mod 6. The
// 16 index bits abid does not select hold another legal pattern that differs in
// every group.
//
// Stages (one instruction each; "hot" = one-hot, band / full odd / narrow as in
// datapath_f16_kernel.h, bf16 and fp8 elements as in their headers):
//   0  32x32x32_f16   selection, A hot: row i holds +-2^f (exponent field
//      1..30) at compressed slot (i + rot) mod 16 of its 16 (lane group,
//      element) slots and +0 elsewhere; B = band halves at all 32 k (odd dwords
//      the complements of the even ones); indices per (row, group); C = +0.
//      D[i][j] = hot_i * B[k(i)][j]: the tile names the row of B each index
//      selected.
//   1  32x32x32_f16   selection, B hot: A = band halves (dword 1 = ~dword 0,
//      dword 3 = ~dword 2: every bit of A's 128-bit path toggles); indices per
//      group only; column j of B holds +-2^f at the dense k that slot
//      (j + rot) mod 16 of A selects, +0 elsewhere; C = +0. No output is zero.
//   2  32x32x32_f16, abid = 1: as stage 0 with the index in idx[31:16].
//   3  32x32x32_f16   sum of 16 terms: A full odd, B narrow (all 32 k, the
//      unselected ones too), C = ga * q.
//   4  16x16x64_f16   sum of 32 terms, A narrow, B full odd.
//   5  32x32x32_bf16  sum of 16 terms: +-(128+m) * 2^(E-134), m odd, both sides.
//   6  16x16x64_bf16  selection, A hot over 32 slots (+-2^f, f in -90..90), B = bf16 band words.
//   7  32x32x64_i8    sum of 32 terms, any bytes (odd dwords the complements of
//      the even ones), C = a hash word >> 1 (arithmetic).
//   8  16x16x128_i8   sum of 64 terms, likewise.
//   9  32x32x64_fp8_bf8  sum of 32 terms: A e4m3 +-(8+m) * 2^(Ea-10), B e5m2
//      +-(4+m') * 2^(Eb-17), m and m' odd, unscaled.
//
// Why every stage is exact. Stages 0, 1, 2 and 6 have exactly one non-zero
// product per output -- the compressed operand or the selected column is
// one-hot and no band element is zero -- of an 11-bit (8-bit) significand and a
// power of two, in [2^-28, 2^31) (bf16: 2^-120..2^122): a normal f32, exact
// under any correct implementation. In stages 3, 4, 5 and 9 the exponent field
// is per row of A (Ea_i) and per column of B (Eb_j), so every product is an odd
// integer times q = 2^(Ea_i+Eb_j-45) (bf16: -268; fp8: -27), C = ga * q with ga
// odd and |ga| < 2^20, and the sum of the magnitudes of all terms and C, in
// units of q, is at most
//   stage 3:  16 * 2047 * 63 + 2^20 = 3 111 952
//   stage 4:  32 * 2047 * 63 + 2^20 = 5 175 328
//   stage 5:  16 * 255 * 255 + 2^20 = 2 088 976
//   stage 9:  32 * 15 * 7    + 2^20 = 1 051 936
// all below 2^24. So every partial sum in every order and tree shape is an
// integer multiple of q below 2^24 q: it fits an f32 significand, and a unit
// that keeps at least 24 significant bits below its largest term when it aligns
// loses nothing (the bf16 check's one assumption). The term count is even and
// ga is odd, so the final sum is odd and not zero. q lies in 2^-74..2^48. In
// stages 7 and 8 the sum of magnitudes is at most 64 * 2^14 + 2^30 < 2^31: no
// order of summation leaves int32.
//
// The same argument makes an f32 fmaf chain over the integer-widened operands
// exact in any order. dpsp_expected walks the compressed elements of A's row
// and picks B's element through the same index words; the kernel's on-device
// comparison and the host's recomputation both call it, and compare words.
#pragma once

#include <stdint.h>

#include "datapath_bf16_kernel.h"
#include "datapath_f16_kernel.h"
#include "datapath_fp8_kernel.h"
#include "datapath_i8_kernel.h"

#define MI355X_DPSP_THREADS 256
#define MI355X_DPSP_STAGES 10
#define MI355X_DPSP_TILE 1024                      // words of a 32x32 tile
#define MI355X_DPSP_TILE16 256                     // words of the 16x16 tiles of stages 4, 6 and 8
#define MI355X_DPSP_WG_WORDS (7 * MI355X_DPSP_TILE + 3 * MI355X_DPSP_TILE16)
// ten counters do not fit beside the eight header words of the siblings' 16-word record: 32 words
#define MI355X_DPSP_REC_WORDS 32
#define MI355X_DPSP_MAGIC 0x44505350u /* "DPSP" */
// record words (one record per workgroup); 18..31 are written as zero
#define MI355X_DPSPREC_MAGIC 0
#define MI355X_DPSPREC_WG 1
#define MI355X_DPSPREC_NONCE 2   // nonce ^ wg
#define MI355X_DPSPREC_XCC 3
#define MI355X_DPSPREC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPSPREC_BAD 8     // 10 words: per stage, MFMA elements (all waves) differing from the recomputation

// explicit kernel arguments (24 bytes; the kernel uses no hidden args)
struct mi355x_datapath_sparse_args {
  uint32_t* records;  // host-visible, grid * MI355X_DPSP_REC_WORDS
  uint32_t* tiles;    // host-visible, grid * MI355X_DPSP_WG_WORDS (wave 0's ten tiles per workgroup)
  uint32_t nonce;
  uint32_t grid;      // workgroups launched; a workgroup beyond it writes nothing
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it):
  // one wrong accumulator word after a stage's MFMA, before the comparison and
  // the tile store. Runtime arguments; an index that names no accumulator
  // register does nothing. The fields mirror mi355x_datapath_f16_args'.
  uint32_t inject_kind;   // MI355X_DPSP_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;   // 0..3
  uint32_t inject_lane;   // 0..63
  uint32_t inject_index;  // stage * 16 + accumulator register (stages 4, 6 and 8 have registers 0..3)
  uint32_t inject_mask;   // xor-ed into that word
#endif
};

#define MI355X_DPSP_INJECT_NONE 0
#define MI355X_DPSP_INJECT_MFMA 1

#if defined(__HIPCC__)
#define MI355X_DPSP_HD __host__ __device__ inline
#else
#define MI355X_DPSP_HD static inline
#endif

// operand index spaces of dpsp_hash
#define MI355X_DPSP_IDX_A 0x0000u     // + (row * 4 + lane group) * 4 + dword
#define MI355X_DPSP_IDX_B 0x1000u     // + (col * 4 + lane group) * 8 + dword
#define MI355X_DPSP_IDX_C 0x2000u     // + row * 32 + col
#define MI355X_DPSP_IDX_HOT 0x3000u   // + row / col of a one-hot operand: the hot element
#define MI355X_DPSP_IDX_ROT 0x3800u   // low 5 bits: the rotation of the one-hot slots
#define MI355X_DPSP_IDX_EA 0x3900u    // + row: the row's exponent field in the f32 sum stages
#define MI355X_DPSP_IDX_EB 0x3A00u    // + col: the column's
#define MI355X_DPSP_IDX_PAIR 0x3B00u  // the offsets of the index pairs

#define MI355X_DPSP_F16 0u   // data kinds
#define MI355X_DPSP_BF16 1u
#define MI355X_DPSP_I8 2u
#define MI355X_DPSP_FP8 3u   // A e4m3, B e5m2
#define MI355X_DPSP_SEL_A 0u  // modes: selection with A hot, selection with B hot, sum
#define MI355X_DPSP_SEL_B 1u
#define MI355X_DPSP_SUM 2u

MI355X_DPSP_HD uint32_t dpsp_kind(uint32_t stage) { return (0x3221100000ull >> (4u * stage)) & 15u; }
MI355X_DPSP_HD uint32_t dpsp_dim(uint32_t stage) { return (stage == 4u || stage == 6u || stage == 8u) ? 16u : 32u; }
MI355X_DPSP_HD uint32_t dpsp_mode(uint32_t stage) {
  return (stage == 0u || stage == 2u || stage == 6u) ? MI355X_DPSP_SEL_A : stage == 1u ? MI355X_DPSP_SEL_B : MI355X_DPSP_SUM;
}
MI355X_DPSP_HD uint32_t dpsp_abid(uint32_t stage) { return stage == 2u ? 1u : 0u; }
MI355X_DPSP_HD uint32_t dpsp_groups(uint32_t stage) { return 64u / dpsp_dim(stage); }            // lane groups
MI355X_DPSP_HD uint32_t dpsp_bits(uint32_t stage) { return dpsp_kind(stage) >= MI355X_DPSP_I8 ? 8u : 16u; }
MI355X_DPSP_HD uint32_t dpsp_kb(uint32_t stage) { return 256u / dpsp_bits(stage); }              // dense K of a lane group
MI355X_DPSP_HD uint32_t dpsp_per(uint32_t stage) { return 32u / dpsp_bits(stage); }              // elements of a dword
MI355X_DPSP_HD uint32_t dpsp_depth(uint32_t stage) { return dpsp_groups(stage) * dpsp_kb(stage); }  // K
// stage 4: A narrow, B full odd; stage 3: the roles swapped
MI355X_DPSP_HD uint32_t dpsp_narrow(uint32_t stage, uint32_t which) { return stage == 4u ? !which : which; }
MI355X_DPSP_HD uint32_t dpsp_tile_offset(uint32_t stage) {
  uint32_t off = 0;
  for (uint32_t s = 0; s < stage; ++s) off += dpsp_dim(s) * dpsp_dim(s);
  return off;
}

MI355X_DPSP_HD uint32_t dpsp_wave_nonce(uint32_t nonce, uint32_t wg, uint32_t wave) {
  return (nonce ^ (wg * 0x9E3779B1u)) + wave * 0x85EBCA77u;
}

MI355X_DPSP_HD uint32_t dpsp_hash(uint32_t nw, uint32_t stage, uint32_t idx) {
  uint32_t h = nw ^ ((stage + 0x83u) * 0x9E3779B1u) ^ (idx * 0x85EBCA77u);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

// the dense k of position p (0..KB-1: 4 * group + index field) of lane group h of A (measured, see above);
// element e of lane group h' of B is k = KB * h' + e
MI355X_DPSP_HD uint32_t dpsp_k_of(uint32_t stage, uint32_t h, uint32_t p) {
  const uint32_t kb = dpsp_kb(stage), r = kb / 2u, m = dpsp_groups(stage) / 2u;
  return kb * (2u * (h % m) + p / r) + r * (h / m) + p % r;
}

// the index pair number (0..5) of group t of lane group h of row `row`, and its 4-bit field
// (first | second << 2) for the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
MI355X_DPSP_HD uint32_t dpsp_pair(uint32_t stage, uint32_t row, uint32_t h, uint32_t t, uint32_t nw) {
  const uint32_t hp = dpsp_hash(nw, stage, MI355X_DPSP_IDX_PAIR);
  if (dpsp_mode(stage) == MI355X_DPSP_SEL_B) return (h * 4u + t + (hp & 7u)) % 6u;
  return (row + ((hp >> ((h * 8u + t) % 29u)) & 7u)) % 6u;
}
MI355X_DPSP_HD uint32_t dpsp_pair_field(uint32_t pair) { return (0xED9C84u >> (4u * pair)) & 15u; }

// the index bits the instruction reads for (row, lane group h): 16 (16-bit data) or 32
MI355X_DPSP_HD uint32_t dpsp_index_bits(uint32_t stage, uint32_t row, uint32_t h, uint32_t nw) {
  uint32_t w = 0;
  for (uint32_t t = 0; t < dpsp_kb(stage) / 4u; ++t) w |= dpsp_pair_field(dpsp_pair(stage, row, h, t, nw)) << (4u * t);
  return w;
}

// the index register of that lane: with 16-bit data the bits sit in the half abid selects, and the other
// half holds pair numbers 1..4 further on, so another legal pair in every group
MI355X_DPSP_HD uint32_t dpsp_index_word(uint32_t stage, uint32_t row, uint32_t h, uint32_t nw) {
  const uint32_t w = dpsp_index_bits(stage, row, h, nw);
  if (dpsp_bits(stage) == 8u) return w;
  const uint32_t step = 1u + ((dpsp_hash(nw, stage, MI355X_DPSP_IDX_PAIR) >> 29) & 3u);
  uint32_t other = 0;
  for (uint32_t t = 0; t < 4u; ++t)
    other |= dpsp_pair_field((dpsp_pair(stage, row, h, t, nw) + step) % 6u) << (4u * t);
  return dpsp_abid(stage) ? (w << 16) | other : w | (other << 16);
}

// a hash word as the band elements of the stage's kind
MI355X_DPSP_HD uint32_t dpsp_band(uint32_t stage, uint32_t h) {
  const uint32_t kind = dpsp_kind(stage);
  if (kind == MI355X_DPSP_F16) return dphf_band16(h & 0xFFFFu) | (dphf_band16(h >> 16) << 16);
  if (kind == MI355X_DPSP_BF16) return dpbf_band16(h & 0xFFFFu) | (dpbf_band16(h >> 16) << 16);
  return h;
}

// the hot element of row / column rc: +-2^f
MI355X_DPSP_HD uint32_t dpsp_hot(uint32_t stage, uint32_t rc, uint32_t nw) {
  const uint32_t h = dpsp_hash(nw, stage, MI355X_DPSP_IDX_HOT + rc);
  if (dpsp_kind(stage) == MI355X_DPSP_BF16) return ((h >> 31) << 15) | ((37u + (h & 0xFFFFu) % 181u) << 7);
  return ((h >> 31) << 15) | ((1u + (h & 0xFFFFu) % 30u) << 10);
}

// the compressed slot (lane group * 8 + element) of the one-hot row or of the column rc's hot position
MI355X_DPSP_HD uint32_t dpsp_hot_slot(uint32_t stage, uint32_t rc, uint32_t nw) {
  return (rc + (dpsp_hash(nw, stage, MI355X_DPSP_IDX_ROT) & 31u)) % (dpsp_groups(stage) * 8u);
}

// the exponent field of row (which = 0) / column (which = 1) rc in the f32 sum stages
MI355X_DPSP_HD uint32_t dpsp_exp_field(uint32_t stage, uint32_t which, uint32_t rc, uint32_t nw) {
  const uint32_t h = dpsp_hash(nw, stage, (which ? MI355X_DPSP_IDX_EB : MI355X_DPSP_IDX_EA) + rc);
  const uint32_t kind = dpsp_kind(stage);
  if (kind == MI355X_DPSP_BF16) return 97u + h % 62u;
  return 1u + h % ((kind == MI355X_DPSP_FP8 && !which) ? 14u : 30u);
}

// a dword of a sum stage's operand: any sign, an odd mantissa (f16: full odd or narrow), exponent field e
MI355X_DPSP_HD uint32_t dpsp_odd_word(uint32_t stage, uint32_t which, uint32_t h, uint32_t e) {
  const uint32_t kind = dpsp_kind(stage);
  if (kind == MI355X_DPSP_F16)
    return (dpsp_narrow(stage, which) ? ((h & 0x83E083E0u) | 0x00200020u) : ((h & 0x83FF83FFu) | 0x00010001u)) |
           (e << 10) | (e << 26);
  if (kind == MI355X_DPSP_BF16) return (h & 0x807F807Fu) | 0x00010001u | (e << 7) | (e << 23);
  if (which) return (h & 0x83838383u) | 0x01010101u | (e * 0x04040404u);  // e5m2
  return (h & 0x87878787u) | 0x01010101u | (e * 0x08080808u);             // e4m3
}

// dword d (0..3) of the compressed A fragment of (row, lane group h)
MI355X_DPSP_HD uint32_t dpsp_a_word(uint32_t stage, uint32_t row, uint32_t h, uint32_t d, uint32_t nw) {
  const uint32_t mode = dpsp_mode(stage);
  if (mode == MI355X_DPSP_SEL_A) {
    const uint32_t slot = dpsp_hot_slot(stage, row, nw);
    return slot == h * 8u + d * 2u ? dpsp_hot(stage, row, nw) : slot == h * 8u + d * 2u + 1u ? dpsp_hot(stage, row, nw) << 16 : 0u;
  }
  if (mode == MI355X_DPSP_SEL_B || dpsp_kind(stage) == MI355X_DPSP_I8) {
    const uint32_t w = dpsp_band(stage, dpsp_hash(nw, stage, MI355X_DPSP_IDX_A + (row * 4u + h) * 4u + (d & 2u)));
    return (d & 1u) ? ~w : w;
  }
  return dpsp_odd_word(stage, 0u, dpsp_hash(nw, stage, MI355X_DPSP_IDX_A + (row * 4u + h) * 4u + d),
                       dpsp_exp_field(stage, 0u, row, nw));
}

// dword d (0..7) of the dense B fragment of (col, lane group h): k = KB * h + d * per .. + per - 1
MI355X_DPSP_HD uint32_t dpsp_b_word(uint32_t stage, uint32_t col, uint32_t h, uint32_t d, uint32_t nw) {
  const uint32_t mode = dpsp_mode(stage);
  if (mode == MI355X_DPSP_SEL_B) {  // hot at the k that slot (lane group ha, element c) of A selects
    const uint32_t slot = dpsp_hot_slot(stage, col, nw), ha = slot >> 3, c = slot & 7u;
    const uint32_t p = 4u * (c >> 1) + ((dpsp_index_bits(stage, 0u, ha, nw) >> (2u * c)) & 3u);
    const uint32_t k = dpsp_k_of(stage, ha, p);
    return k >> 1 == h * 8u + d ? dpsp_hot(stage, col, nw) << (16u * (k & 1u)) : 0u;
  }
  if (mode == MI355X_DPSP_SEL_A || dpsp_kind(stage) == MI355X_DPSP_I8) {
    const uint32_t w = dpsp_band(stage, dpsp_hash(nw, stage, MI355X_DPSP_IDX_B + (col * 4u + h) * 8u + (d & 6u)));
    return (d & 1u) ? ~w : w;
  }
  return dpsp_odd_word(stage, 1u, dpsp_hash(nw, stage, MI355X_DPSP_IDX_B + (col * 4u + h) * 8u + d),
                       dpsp_exp_field(stage, 1u, col, nw));
}

MI355X_DPSP_HD uint32_t dpsp_c_word(uint32_t stage, uint32_t row, uint32_t col, uint32_t nw) {
  if (dpsp_mode(stage) != MI355X_DPSP_SUM) return 0u;
  const uint32_t h = dpsp_hash(nw, stage, MI355X_DPSP_IDX_C + row * 32u + col);
  const uint32_t kind = dpsp_kind(stage);
  if (kind == MI355X_DPSP_I8) return (h >> 1) | (h & 0x80000000u);  // arithmetic shift right by one: |C| <= 2^30
  const int32_t mag = static_cast<int32_t>((h & 0xFFFFFu) | 1u);    // odd, < 2^20
  const int32_t x = static_cast<int32_t>(dpsp_exp_field(stage, 0u, row, nw) + dpsp_exp_field(stage, 1u, col, nw)) -
                    (kind == MI355X_DPSP_F16 ? 45 : kind == MI355X_DPSP_BF16 ? 268 : 27);
  return dphf_scaled_int((h >> 31) ? -mag : mag, x);
}

// element x of a fragment dword of A (which = 0) or B (1), widened to the f32 word with the same value by
// integer arithmetic (no conversion instruction)
MI355X_DPSP_HD uint32_t dpsp_widen(uint32_t stage, uint32_t which, uint32_t word, uint32_t x) {
  const uint32_t kind = dpsp_kind(stage);
  if (kind == MI355X_DPSP_F16) return dphf_widen(word, x);
  if (kind == MI355X_DPSP_BF16) return dpbf_widen(word, x);
  return dpf8_decode((word >> (8u * x)) & 0xFFu, which);
}

// D[row][col] of the stage, as a word, without the matrix unit: C, then one term per compressed element of
// A's row, in (lane group, element) order, each times the element of B's column at the k the index names.
// One trip per dword of A, rolled, so that the kernel stays in registers.
MI355X_DPSP_HD uint32_t dpsp_expected(uint32_t stage, uint32_t row, uint32_t col, uint32_t nw) {
  const uint32_t per = dpsp_per(stage), kb = dpsp_kb(stage), i8 = dpsp_kind(stage) == MI355X_DPSP_I8;
  uint32_t c = dpsp_c_word(stage, row, col, nw);
  float s;
  __builtin_memcpy(&s, &c, sizeof(s));
  int32_t si = static_cast<int32_t>(c);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint32_t hd = 0; hd < dpsp_groups(stage) * 4u; ++hd) {
    const uint32_t h = hd >> 2, d = hd & 3u;
    const uint32_t aw = dpsp_a_word(stage, row, h, d, nw), idx = dpsp_index_bits(stage, row, h, nw);
    for (uint32_t x = 0; x < per; ++x) {
      const uint32_t e = d * per + x;  // compressed element
      const uint32_t k = dpsp_k_of(stage, h, 4u * (e >> 1) + ((idx >> (2u * e)) & 3u));
      const uint32_t bw = dpsp_b_word(stage, col, k / kb, (k % kb) / per, nw), y = k % per;
      if (i8) {
        si += static_cast<int32_t>(static_cast<int8_t>(aw >> (8u * x))) * static_cast<int32_t>(static_cast<int8_t>(bw >> (8u * y)));
      } else {
        const uint32_t fa = dpsp_widen(stage, 0u, aw, x), fb = dpsp_widen(stage, 1u, bw, y);
        float a, b;
        __builtin_memcpy(&a, &fa, sizeof(a));
        __builtin_memcpy(&b, &fb, sizeof(b));
        s = __builtin_fmaf(a, b, s);
      }
    }
  }
  if (i8) return static_cast<uint32_t>(si);
  __builtin_memcpy(&c, &s, sizeof(c));
  return c;
}
