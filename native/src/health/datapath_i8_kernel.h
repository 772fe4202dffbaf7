// Shared between the gfx950 int8 MFMA datapath kernel (mi355x_mfma_datapath_i8),
// the host verdict (datapath_i8_verify.h) and
// native/tests/datapath_i8_contract_cli.cpp.
//
// The f32 datapath check (datapath_kernel.h) drives the one-VGPR operand form.
// This one drives the wide form every bf16 / fp8 / int8 GEMM goes through --
// 4-VGPR (128-bit) A and B operands and the deep K reduction -- with the one
// wide format whose numerics are fully defined: without overflow a 32-bit
// integer sum has no rounding, no order dependence and no alignment question.
//
// Operands are defined by fragment position, not by k. A lane hands the
// instruction four dwords of A and four of B:
//   v_mfma_i32_32x32x32_i8: row / column = lane & 31, K-block = lane >> 5 (2 blocks)
//   v_mfma_i32_16x16x64_i8: row / column = lane & 15, K-block = lane >> 4 (4 blocks)
// and the expected result is
//   D[i][j] = C[i][j] + sum over block, dword, byte of sext(A byte) * sext(B byte)
// with byte e of dword d of block h of A's row i multiplying byte e of dword d
// of block h of B's column j. That pairing is all that is assumed of the A/B
// lane map; an integer sum does not depend on the order of k.
//
//   stage 0  32x32x32  A = any bytes, B = one-hot (+-1 at one of the column's 32
//            positions, position (j + rot) mod 32), C = 0: D = +-A byte
//            (every bit of the 128-bit A path; each position picked once)
//   stage 1  32x32x32  A = one-hot per row, B = any bytes, C = 0  (the B path)
//   stage 2  32x32x32  A, B = any bytes, C = a hash word >> 1 (arithmetic):
//            |sum| <= 32 * 128 * 128 = 2^19, |C| <= 2^30, so |D| < 2^31
//            (multiplier array, 32-term adder tree with mixed signs, carries)
//   stage 3  32x32x32  A = 0, B = any bytes, C = any word: D = C (all 32 bits)
//   stage 4  16x16x64  A, B = any bytes, C as stage 2; |sum| <= 2^20
//            (the other instruction, its 4-block lane routing, a 16x16 tile)
//
// No stage comes within reach of int32 overflow under any summation order.
// In an "any bytes" fragment dword 1 is the complement of dword 0 and dword 3
// of dword 2; in stage 3, C word 1 of each row is the complement of word 0:
// every one of the 32 bits takes both values in A (stage 0), B (stage 1), C
// and D (stage 3) for every nonce, not just very probably.
#pragma once

#include <stdint.h>

#define MI355X_DPI8_THREADS 256
#define MI355X_DPI8_STAGES 5
#define MI355X_DPI8_WIDE_STAGES 4                  // stages 0..3: 32x32x32, a 32x32 tile each
#define MI355X_DPI8_TILE 1024                      // words of a 32x32 tile
#define MI355X_DPI8_TILE16 256                     // words of the 16x16 tile of stage 4
#define MI355X_DPI8_WG_WORDS (MI355X_DPI8_WIDE_STAGES * MI355X_DPI8_TILE + MI355X_DPI8_TILE16)
#define MI355X_DPI8_REC_WORDS 16
#define MI355X_DPI8_MAGIC 0x44504938u /* "DPI8" */
// record words (one record per workgroup); 13..15 are written as zero
#define MI355X_DPI8REC_MAGIC 0
#define MI355X_DPI8REC_WG 1
#define MI355X_DPI8REC_NONCE 2   // nonce ^ wg
#define MI355X_DPI8REC_XCC 3
#define MI355X_DPI8REC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPI8REC_BAD 8     // 5 words: per stage, MFMA elements (all waves) differing from the recomputation

// explicit kernel arguments (24 bytes; the kernel uses no hidden args)
struct mi355x_datapath_i8_args {
  uint32_t* records;  // host-visible, grid * MI355X_DPI8_REC_WORDS
  uint32_t* tiles;    // host-visible, grid * MI355X_DPI8_WG_WORDS (wave 0's five tiles per workgroup)
  uint32_t nonce;
  uint32_t grid;      // workgroups launched; a workgroup beyond it writes nothing
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it):
  // one wrong accumulator word after a stage's MFMA, before the comparison and
  // the tile store. Runtime arguments; an index that names no accumulator
  // register does nothing. The fields mirror mi355x_datapath_args'.
  uint32_t inject_kind;   // MI355X_DPI8_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;   // 0..3
  uint32_t inject_lane;   // 0..63
  uint32_t inject_index;  // stage * 16 + accumulator register (stage 4 has registers 0..3)
  uint32_t inject_mask;   // xor-ed into that word
#endif
};

#define MI355X_DPI8_INJECT_NONE 0
#define MI355X_DPI8_INJECT_MFMA 1

#if defined(__HIPCC__)
#define MI355X_DPI8_HD __host__ __device__ inline
#else
#define MI355X_DPI8_HD static inline
#endif

// operand index spaces of dpi8_hash
#define MI355X_DPI8_IDX_A 0x0000u    // + (row * 4 + block) * 4 + dword
#define MI355X_DPI8_IDX_B 0x1000u    // + (col * 4 + block) * 4 + dword
#define MI355X_DPI8_IDX_C 0x2000u    // + row * 32 + col
#define MI355X_DPI8_IDX_SIGN 0x3000u // + row / col of a one-hot operand: bit 31 = minus
#define MI355X_DPI8_IDX_ROT 0x3800u  // low 5 bits: the rotation of the one-hot positions

MI355X_DPI8_HD uint32_t dpi8_blocks(uint32_t stage) { return stage == 4u ? 4u : 2u; }
MI355X_DPI8_HD uint32_t dpi8_dim(uint32_t stage) { return stage == 4u ? 16u : 32u; }
MI355X_DPI8_HD uint32_t dpi8_tile_offset(uint32_t stage) { return stage * MI355X_DPI8_TILE; }

MI355X_DPI8_HD uint32_t dpi8_wave_nonce(uint32_t nonce, uint32_t wg, uint32_t wave) {
  return (nonce ^ (wg * 0x9E3779B1u)) + wave * 0x85EBCA77u;
}

MI355X_DPI8_HD uint32_t dpi8_hash(uint32_t nw, uint32_t stage, uint32_t idx) {
  uint32_t h = nw ^ ((stage + 0x11u) * 0x9E3779B1u) ^ (idx * 0x85EBCA77u);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

// "any bytes": dword 1 is the complement of dword 0, dword 3 of dword 2
MI355X_DPI8_HD uint32_t dpi8_any_word(uint32_t nw, uint32_t stage, uint32_t base, uint32_t rc, uint32_t block,
                                      uint32_t dword) {
  const uint32_t h = dpi8_hash(nw, stage, base + (rc * 4u + block) * 4u + (dword & 2u));
  return (dword & 1u) ? ~h : h;
}

// one-hot over the 32 (block, dword, byte) positions of a 32x32x32 fragment:
// row / column rc has +1 or -1 at position (rc + rot) mod 32, 0 elsewhere
MI355X_DPI8_HD uint32_t dpi8_onehot_word(uint32_t nw, uint32_t stage, uint32_t rc, uint32_t block, uint32_t dword) {
  const uint32_t pos = (rc + (dpi8_hash(nw, stage, MI355X_DPI8_IDX_ROT) & 31u)) & 31u;
  if ((pos >> 2) != block * 4u + dword) return 0u;
  const uint32_t minus = dpi8_hash(nw, stage, MI355X_DPI8_IDX_SIGN + rc) >> 31;
  return (minus ? 0xFFu : 0x01u) << (8u * (pos & 3u));
}

MI355X_DPI8_HD uint32_t dpi8_a_word(uint32_t stage, uint32_t row, uint32_t block, uint32_t dword, uint32_t nw) {
  if (stage == 1u) return dpi8_onehot_word(nw, 1u, row, block, dword);
  if (stage == 3u) return 0u;
  return dpi8_any_word(nw, stage, MI355X_DPI8_IDX_A, row, block, dword);
}

MI355X_DPI8_HD uint32_t dpi8_b_word(uint32_t stage, uint32_t col, uint32_t block, uint32_t dword, uint32_t nw) {
  if (stage == 0u) return dpi8_onehot_word(nw, 0u, col, block, dword);
  return dpi8_any_word(nw, stage, MI355X_DPI8_IDX_B, col, block, dword);
}

MI355X_DPI8_HD uint32_t dpi8_c_word(uint32_t stage, uint32_t row, uint32_t col, uint32_t nw) {
  if (stage == 2u || stage == 4u) {
    const uint32_t h = dpi8_hash(nw, stage, MI355X_DPI8_IDX_C + row * 32u + col);
    return (h >> 1) | (h & 0x80000000u);  // arithmetic shift right by one: |C| <= 2^30
  }
  if (stage == 3u) {
    const uint32_t h = dpi8_hash(nw, 3u, MI355X_DPI8_IDX_C + row * 32u + (col == 1u ? 0u : col));
    return col == 1u ? ~h : h;
  }
  return 0u;
}

// sum over the four bytes of sext(a byte) * sext(b byte), plus c; plain
// integer arithmetic (the kernel uses v_dot4 for the same sum)
MI355X_DPI8_HD int32_t dpi8_dot4(uint32_t a, uint32_t b, int32_t c) {
  for (uint32_t e = 0; e < 4u; ++e)
    c += (int32_t)(int8_t)(a >> (8u * e)) * (int32_t)(int8_t)(b >> (8u * e));
  return c;
}
