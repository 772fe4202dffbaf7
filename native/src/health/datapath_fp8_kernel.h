// Shared between the gfx950 fp8 / MX-scaled MFMA datapath kernel
// (mi355x_mfma_datapath_fp8), the host verdict (datapath_fp8_verify.h) and
// native/tests/datapath_fp8_contract_cli.cpp.
//
// The f32, int8 and bf16 checks (datapath_kernel.h, datapath_i8_kernel.h,
// datapath_bf16_kernel.h) leave the 8-bit float part of the matrix core
// untouched: the two OCP decoders (e4m3fn, e5m2), the 64-bit operand path of
// v_mfma_f32_32x32x16_{fp8,bf8}_{fp8,bf8} / v_mfma_f32_16x16x32_*, and the
// 256-bit operand path, the E8M0 scale path with its byte select and the 64- /
// 128-term reduction of v_mfma_scale_f32_32x32x64_f8f6f4 /
// v_mfma_scale_f32_16x16x128_f8f6f4. This check drives them with fp8 operands
// (fp6 and fp4 stay out) chosen so that every correct implementation must
// return the same bits.
//
// Formats. e4m3: sign.4.3, bias 7, a normal value is +-(8+m) * 2^(E-10).
// e5m2: sign.5.2, bias 15, +-(4+m) * 2^(E-17). A "band byte" has any sign, any
// mantissa and exponent field 1..14 (e4m3) or 1..30 (e5m2): both bands are
// closed under 8-bit complement and hold no zero, subnormal, Inf or NaN, so
// nothing depends on fp8 subnormal handling or NaN encodings. A "scale band
// byte" is an E8M0 value in 97..158 (2^-30..2^31), closed under complement;
// 255 (NaN) is never used.
//
// A lane hands the instruction a fragment of `dwords` dwords of A and of B: 2
// for the non-scaled forms, 8 for f8f6f4. Byte e of dword d of the fragment of
// K-block h is k = (h * dwords + d) * 4 + e:
//   32x32: lane l holds row / column l&31 and K-block l>>5  (2 blocks)
//   16x16: lane l holds row / column l&15 and K-block l>>4  (4 blocks)
//   D[i][j] = C[i][j] + sum over k of A[i][k] * B[k][j] * 2^(sa[i][g]-127) * 2^(sb[j][g]-127)
// where sa[i][g] / sb[j][g], the scaled forms only, is the E8M0 byte that lane
// (row / column, lane group g) selects (op_sel) from its scale VGPR, and g is
// the element's scale block. A scale block is 32 elements, but not one lane's
// fragment: it is one 16-byte half of the fragments of two lane groups
// (measured on an MI355X, docs/health.md; a lane's scale applied to its own 32
// bytes reproduces neither form):
//   32x32x64:  byte e of lane group h is in scale block e>>4            (the halves of groups 0 and 1)
//   16x16x128: byte e of lane group h is in scale block 2*(e>>4) + (h>>1)
// That A's byte meets the same byte of B's fragment of the same lane group
// holds as for int8 (the one-hot stages show it). In a band
// fragment each odd dword is the complement of the even dword before it, so
// every bit of the operand path takes both values in every fragment, for every
// nonce. The three bytes of a scale VGPR that are not selected hold three more
// band values, all four different, so a wrong byte select shows.
//
//   stage 0  32x32x16 fp8_fp8   A = e4m3 band bytes; B = one-hot: column j holds
//            +-2^f (an e4m3 power of two in the band) at position (j + rot) mod 16
//            of its 16 (block, byte) positions, +0 elsewhere; C = +0.
//            D = +-A[i][k_j] * 2^f, one non-zero product.
//   stage 1  32x32x16 bf8_bf8   A = one-hot per row, e5m2; B = e5m2 band bytes.
//   stage 2  32x32x16 fp8_bf8   A[i][k] = +-(8+m) * 2^(Ea_i-10), m odd, Ea_i per
//            row; B[k][j] = +-(4+m') * 2^(Eb_j-17), m' odd, Eb_j per column;
//            C = ga * q, ga odd, |ga| < 2^20, q = 2^(Ea_i+Eb_j-27).
//   stage 3  16x16x32 bf8_fp8   as stage 2 with the formats swapped, 32 terms.
//   stage 4  scale 32x32x64, A e4m3 (cbsz 0), B e5m2 (blgp 1): A = band bytes,
//            8 dwords; B = one-hot over the 64 positions of the column; scale
//            band bytes per lane (one per row / column and scale block) for A and B; C = +0.
//            D = +-A * 2^f * 2^(sa+sb-254), one non-zero product.
//   stage 5  scale 32x32x64, A e5m2 one-hot per row, B e4m3 band bytes.
//   stage 6  scale 32x32x64, e4m3 x e4m3: as stage 2 per row and per column;
//            scales SA_i + d and SB_j + d', d and d' in 0..3 per (row or column,
//            scale block), SA_i and SB_j in 112..142; C = ga * q, q the quantum at
//            d = d' = 0.
//   stage 7  scale 16x16x128, e5m2 x e5m2: as stage 6, 128 terms, 4 K-blocks.
// Scale byte select: stage s takes byte s-4 for A and byte 7-s for B, so the
// four stages use every position once for A and once for B. In stages 4 and 5
// wave v rotates the one-hot positions by 16 * (wave nonce & 3), which takes all
// four values over the waves of a workgroup: together they select every one of
// the 64 positions.
//
// Stages 0, 1, 4 and 5 have one non-zero term each and are exact under any
// correct implementation whatsoever; |D| lies in 2^-12..2^15 (stage 0),
// 2^-28..2^32 (stage 1) and 2^-80..2^86 (stages 4 and 5): normal f32.
//
// Why stages 2, 3, 6 and 7 are exact. Every product is an odd integer
// (8+m)(4+m') etc. below 2^8 times q, times 2^(d+d') <= 2^6 in the scaled
// stages; C is below 2^20 q. So every partial sum in every order and tree
// shape is an integer multiple of q below 2^21 q (stage 2: 16 terms), 2^21 q
// (stage 3), 2^22 q (stage 6: 64 terms below 2^14 q) and 2^23 q (stage 7), all
// below 2^24 q: it fits an f32 significand, and a unit that keeps at least 24
// significant bits below its largest term when it aligns loses nothing. The
// 32 elements of a scale block share one scale (16, 32 in the non-scaled
// stages share none), so the terms that are odd multiples of q come in even
// counts; ga is odd, so the final sum is odd and not zero. q lies in
// 2^-62..2^56.
//
// No output word of any stage is zero.
//
// The same argument makes a k-ordered f32 fmaf chain exact. The operands are
// decoded to f32 by integer bit arithmetic (dpf8_decode: no v_cvt of fp8, which
// would be another copy of the decoder under test) and a block's scale is
// applied as an exact power of two; the kernel's on-device comparison and the
// host's recomputation both do that, and compare words, not floats.
#pragma once

#include <stdint.h>

#define MI355X_DPF8_THREADS 256
#define MI355X_DPF8_STAGES 8
#define MI355X_DPF8_TILE 1024                      // words of a 32x32 tile
#define MI355X_DPF8_TILE16 256                     // words of the 16x16 tiles of stages 3 and 7
#define MI355X_DPF8_WG_WORDS (6 * MI355X_DPF8_TILE + 2 * MI355X_DPF8_TILE16)
#define MI355X_DPF8_REC_WORDS 16
#define MI355X_DPF8_MAGIC 0x44504638u /* "DPF8" */
// record words (one record per workgroup)
#define MI355X_DPF8REC_MAGIC 0
#define MI355X_DPF8REC_WG 1
#define MI355X_DPF8REC_NONCE 2   // nonce ^ wg
#define MI355X_DPF8REC_XCC 3
#define MI355X_DPF8REC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPF8REC_BAD 8     // 8 words: per stage, MFMA elements (all waves) differing from the recomputation

// explicit kernel arguments (24 bytes; the kernel uses no hidden args)
struct mi355x_datapath_fp8_args {
  uint32_t* records;  // host-visible, grid * MI355X_DPF8_REC_WORDS
  uint32_t* tiles;    // host-visible, grid * MI355X_DPF8_WG_WORDS (wave 0's eight tiles per workgroup)
  uint32_t nonce;
  uint32_t grid;      // workgroups launched; a workgroup beyond it writes nothing
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it):
  // one wrong accumulator word after a stage's MFMA, before the comparison and
  // the tile store. Runtime arguments; an index that names no accumulator
  // register does nothing. The fields mirror mi355x_datapath_bf16_args'.
  uint32_t inject_kind;   // MI355X_DPF8_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;   // 0..3
  uint32_t inject_lane;   // 0..63
  uint32_t inject_index;  // stage * 16 + accumulator register (stages 3 and 7 have registers 0..3)
  uint32_t inject_mask;   // xor-ed into that word
#endif
};

#define MI355X_DPF8_INJECT_NONE 0
#define MI355X_DPF8_INJECT_MFMA 1

#if defined(__HIPCC__)
#define MI355X_DPF8_HD __host__ __device__ inline
#else
#define MI355X_DPF8_HD static inline
#endif

// operand index spaces of dpf8_hash
#define MI355X_DPF8_IDX_A 0x0000u       // + (row * 4 + block) * 8 + dword
#define MI355X_DPF8_IDX_B 0x1000u       // + (col * 4 + block) * 8 + dword
#define MI355X_DPF8_IDX_C 0x2000u       // + row * 32 + col
#define MI355X_DPF8_IDX_SIGN 0x3000u    // + row / col of a one-hot operand: bit 31 = minus, low bits: f
#define MI355X_DPF8_IDX_ROT 0x3800u     // low 4 bits: the rotation of the one-hot positions of stages 0 and 1
#define MI355X_DPF8_IDX_EA 0x3900u      // + row: the row's exponent field in the product stages
#define MI355X_DPF8_IDX_EB 0x3A00u      // + col: the column's
#define MI355X_DPF8_IDX_SCALE_A 0x4000u // + row * 4 + scale block: the scale byte (stages 4, 5) or d (stages 6, 7)
#define MI355X_DPF8_IDX_SCALE_B 0x4800u // + col * 4 + block
#define MI355X_DPF8_IDX_SA 0x5000u      // + row: SA_i of stages 6 and 7
#define MI355X_DPF8_IDX_SB 0x5100u      // + col: SB_j

#define MI355X_DPF8_E4M3 0u
#define MI355X_DPF8_E5M2 1u
#define MI355X_DPF8_SCALE_LO 97u        // scale band bytes: 97..158
#define MI355X_DPF8_SCALE_N 62u
#define MI355X_DPF8_SBASE_LO 112u       // SA_i, SB_j: 112..142
#define MI355X_DPF8_SBASE_N 31u

MI355X_DPF8_HD uint32_t dpf8_dim(uint32_t stage) { return (stage == 3u || stage == 7u) ? 16u : 32u; }
MI355X_DPF8_HD uint32_t dpf8_blocks(uint32_t stage) { return (stage == 3u || stage == 7u) ? 4u : 2u; }
MI355X_DPF8_HD uint32_t dpf8_dwords(uint32_t stage) { return stage >= 4u ? 8u : 2u; }  // of one fragment
MI355X_DPF8_HD uint32_t dpf8_scaled(uint32_t stage) { return stage >= 4u; }
MI355X_DPF8_HD uint32_t dpf8_product(uint32_t stage) { return (stage & 3u) >= 2u; }     // stages 2, 3, 6, 7
MI355X_DPF8_HD uint32_t dpf8_fmt_a(uint32_t stage) { return stage & 1u; }               // MI355X_DPF8_E4M3 / _E5M2
MI355X_DPF8_HD uint32_t dpf8_fmt_b(uint32_t stage) { return (0x96u >> stage) & 1u; }    // e5m2 in stages 1, 2, 4, 7
MI355X_DPF8_HD uint32_t dpf8_onehot_a(uint32_t stage) { return stage == 1u || stage == 5u; }
MI355X_DPF8_HD uint32_t dpf8_onehot_b(uint32_t stage) { return stage == 0u || stage == 4u; }
MI355X_DPF8_HD uint32_t dpf8_tile_offset(uint32_t stage) {
  return stage * MI355X_DPF8_TILE - (stage > 3u ? MI355X_DPF8_TILE - MI355X_DPF8_TILE16 : 0u);
}
// the byte (op_sel) of the scale VGPR a scaled stage takes: `which` 0 = A, 1 = B
MI355X_DPF8_HD uint32_t dpf8_scale_sel(uint32_t stage, uint32_t which) { return which ? 7u - stage : stage - 4u; }

MI355X_DPF8_HD uint32_t dpf8_wave_nonce(uint32_t nonce, uint32_t wg, uint32_t wave) {
  return (nonce ^ (wg * 0x9E3779B1u)) + wave * 0x85EBCA77u;
}

MI355X_DPF8_HD uint32_t dpf8_hash(uint32_t nw, uint32_t stage, uint32_t idx) {
  uint32_t h = nw ^ ((stage + 0x41u) * 0x9E3779B1u) ^ (idx * 0x85EBCA77u);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

// exponent fields of a format's band: 1..14 (e4m3), 1..30 (e5m2)
MI355X_DPF8_HD uint32_t dpf8_band_n(uint32_t fmt) { return fmt ? 30u : 14u; }
MI355X_DPF8_HD uint32_t dpf8_mant_bits(uint32_t fmt) { return fmt ? 2u : 3u; }

// an 8-bit hash value as a band byte: sign and mantissa kept, the exponent bits scaled onto the band
MI355X_DPF8_HD uint32_t dpf8_band8(uint32_t h8, uint32_t fmt) {
  if (fmt) return (h8 & 0x83u) | ((1u + ((((h8 >> 2) & 0x1Fu) * 30u) >> 5)) << 2);
  return (h8 & 0x87u) | ((1u + ((((h8 >> 3) & 0xFu) * 14u) >> 4)) << 3);
}

// band bytes: each odd dword is the complement of the even dword before it
MI355X_DPF8_HD uint32_t dpf8_band_word(uint32_t nw, uint32_t stage, uint32_t base, uint32_t fmt, uint32_t rc,
                                       uint32_t block, uint32_t dword) {
  const uint32_t h = dpf8_hash(nw, stage, base + (rc * 4u + block) * 8u + (dword & ~1u));
  const uint32_t w = dpf8_band8(h & 0xFFu, fmt) | (dpf8_band8((h >> 8) & 0xFFu, fmt) << 8) |
                     (dpf8_band8((h >> 16) & 0xFFu, fmt) << 16) | (dpf8_band8(h >> 24, fmt) << 24);
  return (dword & 1u) ? ~w : w;
}

// the (block, byte) position, 0..15 or 0..63, where row / column rc of a one-hot operand is not zero
MI355X_DPF8_HD uint32_t dpf8_onehot_pos(uint32_t nw, uint32_t stage, uint32_t rc) {
  if (dpf8_scaled(stage)) return (rc + 16u * (nw & 3u)) & 63u;
  return (rc + (dpf8_hash(nw, stage, MI355X_DPF8_IDX_ROT) & 15u)) & 15u;
}

// the byte there: +-2^f, a power of two of the band
MI355X_DPF8_HD uint32_t dpf8_onehot_byte(uint32_t nw, uint32_t stage, uint32_t fmt, uint32_t rc) {
  const uint32_t h = dpf8_hash(nw, stage, MI355X_DPF8_IDX_SIGN + rc);
  const uint32_t e = 1u + (h & 0xFFFFu) % dpf8_band_n(fmt);
  return ((h >> 31) << 7) | (e << dpf8_mant_bits(fmt));
}

MI355X_DPF8_HD uint32_t dpf8_onehot_word(uint32_t nw, uint32_t stage, uint32_t fmt, uint32_t rc, uint32_t block,
                                         uint32_t dword) {
  const uint32_t pos = dpf8_onehot_pos(nw, stage, rc);
  if ((pos >> 2) != block * dpf8_dwords(stage) + dword) return 0u;
  return dpf8_onehot_byte(nw, stage, fmt, rc) << (8u * (pos & 3u));
}

// product stages: the row's / column's exponent field, in the format's band
MI355X_DPF8_HD uint32_t dpf8_exp_field(uint32_t nw, uint32_t stage, uint32_t base, uint32_t fmt, uint32_t rc) {
  return 1u + dpf8_hash(nw, stage, base + rc) % dpf8_band_n(fmt);
}

// four elements with any sign, an odd mantissa and exponent field e
MI355X_DPF8_HD uint32_t dpf8_odd_word(uint32_t nw, uint32_t stage, uint32_t base, uint32_t fmt, uint32_t rc,
                                      uint32_t block, uint32_t dword, uint32_t e) {
  const uint32_t h = dpf8_hash(nw, stage, base + (rc * 4u + block) * 8u + dword);
  if (fmt) return (h & 0x83838383u) | 0x01010101u | (e * 0x04040404u);
  return (h & 0x87878787u) | 0x01010101u | (e * 0x08080808u);
}

MI355X_DPF8_HD uint32_t dpf8_a_word(uint32_t stage, uint32_t row, uint32_t block, uint32_t dword, uint32_t nw) {
  const uint32_t fmt = dpf8_fmt_a(stage);
  if (dpf8_onehot_a(stage)) return dpf8_onehot_word(nw, stage, fmt, row, block, dword);
  if (dpf8_product(stage))
    return dpf8_odd_word(nw, stage, MI355X_DPF8_IDX_A, fmt, row, block, dword,
                         dpf8_exp_field(nw, stage, MI355X_DPF8_IDX_EA, fmt, row));
  return dpf8_band_word(nw, stage, MI355X_DPF8_IDX_A, fmt, row, block, dword);
}

MI355X_DPF8_HD uint32_t dpf8_b_word(uint32_t stage, uint32_t col, uint32_t block, uint32_t dword, uint32_t nw) {
  const uint32_t fmt = dpf8_fmt_b(stage);
  if (dpf8_onehot_b(stage)) return dpf8_onehot_word(nw, stage, fmt, col, block, dword);
  if (dpf8_product(stage))
    return dpf8_odd_word(nw, stage, MI355X_DPF8_IDX_B, fmt, col, block, dword,
                         dpf8_exp_field(nw, stage, MI355X_DPF8_IDX_EB, fmt, col));
  return dpf8_band_word(nw, stage, MI355X_DPF8_IDX_B, fmt, col, block, dword);
}

// the scale block of the bytes of dword `dword` (0..7) of the fragment of lane group `block`
MI355X_DPF8_HD uint32_t dpf8_scale_block(uint32_t stage, uint32_t block, uint32_t dword) {
  return dpf8_dim(stage) == 16u ? 2u * (dword >> 2) + (block >> 1) : (dword >> 2);
}

// stages 6 and 7: SA_i (which = 0) or SB_j (which = 1)
MI355X_DPF8_HD uint32_t dpf8_scale_base(uint32_t nw, uint32_t stage, uint32_t which, uint32_t rc) {
  return MI355X_DPF8_SBASE_LO +
         dpf8_hash(nw, stage, (which ? MI355X_DPF8_IDX_SB : MI355X_DPF8_IDX_SA) + rc) % MI355X_DPF8_SBASE_N;
}

// the E8M0 scale of scale block `block` of row / column rc of A (which = 0) or B (which = 1) in a scaled
// stage: what lane (rc, lane group `block`) holds in the selected byte of its scale VGPR
MI355X_DPF8_HD uint32_t dpf8_scale_byte(uint32_t nw, uint32_t stage, uint32_t which, uint32_t rc, uint32_t block) {
  const uint32_t h =
      dpf8_hash(nw, stage, (which ? MI355X_DPF8_IDX_SCALE_B : MI355X_DPF8_IDX_SCALE_A) + rc * 4u + block);
  if (dpf8_product(stage)) return dpf8_scale_base(nw, stage, which, rc) + (h & 3u);
  return MI355X_DPF8_SCALE_LO + h % MI355X_DPF8_SCALE_N;
}

// the scale VGPR of that lane: the scale in the byte
// the stage selects, three other band values, all four different, in the rest
MI355X_DPF8_HD uint32_t dpf8_scale_word(uint32_t nw, uint32_t stage, uint32_t which, uint32_t rc, uint32_t block) {
  const uint32_t s = dpf8_scale_byte(nw, stage, which, rc, block) - MI355X_DPF8_SCALE_LO;
  const uint32_t sel = dpf8_scale_sel(stage, which);
  uint32_t w = 0;
  for (uint32_t p = 0; p < 4u; ++p)
    w |= (MI355X_DPF8_SCALE_LO + (s + ((p - sel) & 3u) * 15u) % MI355X_DPF8_SCALE_N) << (8u * p);
  return w;
}

// product stages: x of q = 2^x, of which C and every product of D[row][col] are multiples
MI355X_DPF8_HD int32_t dpf8_quantum(uint32_t nw, uint32_t stage, uint32_t row, uint32_t col) {
  const uint32_t fa = dpf8_fmt_a(stage), fb = dpf8_fmt_b(stage);
  int32_t x = static_cast<int32_t>(dpf8_exp_field(nw, stage, MI355X_DPF8_IDX_EA, fa, row) +
                                   dpf8_exp_field(nw, stage, MI355X_DPF8_IDX_EB, fb, col)) -
              static_cast<int32_t>((fa ? 17u : 10u) + (fb ? 17u : 10u));
  if (dpf8_scaled(stage))
    x += static_cast<int32_t>(dpf8_scale_base(nw, stage, 0u, row) + dpf8_scale_base(nw, stage, 1u, col)) - 254;
  return x;
}

// the f32 bit pattern of ga * 2^x for an odd ga, 0 < |ga| < 2^20: built from
// integers (normalise, then place the exponent), the same on host and device
MI355X_DPF8_HD uint32_t dpf8_scaled_int(int32_t ga, int32_t x) {
  const uint32_t sign = ga < 0 ? 0x80000000u : 0u;
  const uint32_t mag = static_cast<uint32_t>(ga < 0 ? -ga : ga);
  const uint32_t top = 31u - static_cast<uint32_t>(__builtin_clz(mag));  // position of the leading one
  return sign | (static_cast<uint32_t>(127 + static_cast<int32_t>(top) + x) << 23) | ((mag << (23u - top)) & 0x7FFFFFu);
}

MI355X_DPF8_HD uint32_t dpf8_c_word(uint32_t stage, uint32_t row, uint32_t col, uint32_t nw) {
  if (!dpf8_product(stage)) return 0u;
  const uint32_t h = dpf8_hash(nw, stage, MI355X_DPF8_IDX_C + row * 32u + col);
  const int32_t mag = static_cast<int32_t>((h & 0xFFFFFu) | 1u);  // odd, < 2^20
  return dpf8_scaled_int((h >> 31) ? -mag : mag, dpf8_quantum(nw, stage, row, col));
}

// the f32 word with the value of an fp8 byte, by integer arithmetic alone;
// zero (the one-hot operands' filler) keeps its sign, subnormals do not occur
MI355X_DPF8_HD uint32_t dpf8_decode(uint32_t byte, uint32_t fmt) {
  const uint32_t sign = (byte & 0x80u) << 24;
  if ((byte & 0x7Fu) == 0u) return sign;
  if (fmt) return sign | ((((byte >> 2) & 0x1Fu) + 112u) << 23) | ((byte & 3u) << 21);
  return sign | ((((byte >> 3) & 0xFu) + 120u) << 23) | ((byte & 7u) << 20);
}

// the f32 word of 2^(s-127) for a scale band byte
MI355X_DPF8_HD uint32_t dpf8_scale_f32(uint32_t s) { return s << 23; }
