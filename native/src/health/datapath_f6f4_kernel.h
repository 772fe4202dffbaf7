// Shared between the gfx950 fp6 / fp4 MX-scaled MFMA datapath kernel
// (mi355x_mfma_datapath_f6f4), the host verdict (datapath_f6f4_verify.h) and
// native/tests/datapath_f6f4_contract_cli.cpp.
//
// The fp8 check (datapath_fp8_kernel.h) feeds v_mfma_scale_f32_32x32x64_f8f6f4
// and v_mfma_scale_f32_16x16x128_f8f6f4 256-bit operands of 8-bit elements
// only. It leaves untouched the e2m3, e3m2 and e2m1 decoders with their
// subnormals, the 192-bit and 128-bit operand paths, and the unpacking of
// 6-bit and 4-bit elements that straddle dword boundaries: what MXFP6 and
// MXFP4 weights run through. This check drives them with operands chosen so
// that every correct implementation must return the same bits.
//
// Formats (cbsz / blgp selector, layout, bias; every code is a finite number
// and a subnormal is a real value; u is the value in units of the quantum):
//   0  e4m3  sign.4.3  bias 7  quantum 2^-9  8 dwords  (stage 6's A only; exponent field 1..14, never NaN)
//   2  e2m3  sign.2.3  bias 1  quantum 2^-3  6 dwords  u = m (E = 0) or (8+m) * 2^(E-1), at most 60
//   3  e3m2  sign.3.2  bias 3  quantum 2^-4  6 dwords  u = m (E = 0) or (4+m) * 2^(E-1), at most 448
//   4  e2m1  sign.2.1  bias 1  quantum 2^-1  4 dwords  u = m (E = 0) or (2+m) * 2^(E-1), at most 12
// The builtin always takes eight dwords; the instruction encodes and reads
// only the low 8, 6 or 4, and the rest are handed over as zero.
//
// A lane hands the instruction a fragment of 32 elements of A and of B:
//   32x32: lane l holds row / column l&31 and lane group l>>5  (2 groups, K = 64)
//   16x16: lane l holds row / column l&15 and lane group l>>4  (4 groups, K = 128)
//   D[i][j] = C[i][j] + sum over k of A[i][k] * B[j][k] * 2^(sa[i][k>>5]-127) * 2^(sb[j][k>>5]-127)
// where sa[i][g] / sb[j][g], the scale of scale block g (32 consecutive k), is
// the E8M0 byte that lane (row / column, lane group g) selects (op_sel) from
// its scale VGPR.
//
// Packing: element e of a lane's 32 is the e-th 6-bit or 4-bit field of the
// fragment's little-endian bit stream: bits 6e..6e+5 (elements 5, 10, 21 and
// 26 straddle two dwords) or 4e..4e+3.
// Which k an element is depends on its width (dpf6_k), measured on an MI355X
// (docs/health.md):
//   6- and 4-bit: element e of lane group h is k = 32*h + e: a fragment is one
//                 whole scale block, and the lane's own scale applies to it.
//   8-bit:        byte e of lane group h is k = 32*(e>>4) + 16*h + (e&15)
//                 (32x32x64) or 64*(e>>4) + 16*h + (e&15) (16x16x128): two runs
//                 of 16, which is the fp8 check's scale-block rule e>>4 or
//                 2*(e>>4) + (h>>1).
// So in stage 6 byte e of A's fragment does not meet element e of B's. This
// check first assumed the fp8 rule for every width; the first run on the GPU
// returned the one-hot tiles of stages 0..3 exact wherever the two rules agree
// (the waves whose one-hot positions fall in scale block = lane group) and with
// the other block's scale elsewhere, and the rule above then reproduced every
// word of all eight stages.
//
// Codes. A "band code" is every code of its format but +-0 and their bitwise
// complements (the largest magnitudes, 0x1F / 0x3F or 0x7 / 0xF): 60 of 64 or
// 12 of 16. The band is closed under complement, holds the subnormals and
// makes no zero product. In a band fragment elements 16..31 are the
// complements of elements 0..15 (dwords 3..5 of dwords 0..2, or 2..3 of 0..1),
// so every operand bit takes both values in every fragment for every nonce. A "free code" is any code
// but +-0: the product stages 4, 5 and 7 use them and so exercise the largest
// magnitudes the band leaves out. +0 is the one-hot operands' filler; -0 is
// in no stage (its product could not be told from +0's in a sum). A "hot
// code" is +-2^p units, p in 0..5 (e2m3), 0..8 (e3m2) or 0..3 (e2m1): the
// subnormal powers of two too. A "scale band byte" is an E8M0 value in
// 97..158, as in the fp8 check; the three bytes of a scale VGPR that are not
// selected hold three more band values, all four different.
//
//   stage 0  32x32x64   A = e2m3 band codes (6 dwords); B = e2m1 one-hot (4 dwords):
//            column j holds a hot code at one of its 64 k positions and +0
//            elsewhere; scale band bytes per (row or column,
//            scale block); C = +0. D = +-ua * 2^p * 2^-4 * 2^(sa+sb-254).
//   stage 1  32x32x64   A = e3m2 one-hot per row (6 dwords); B = e2m1 band codes (4 dwords).
//   stage 2  32x32x64   A = e2m1 band codes (4 dwords); B = e2m3 one-hot (6 dwords).
//   stage 3  16x16x128  A = e2m1 one-hot per row (4 dwords), 128 positions; B = e3m2 band codes (6 dwords).
//   stage 4  32x32x64   e2m3 x e2m3, free codes; scales SA_i + d and SB_j + d',
//            SA_i and SB_j in 112..142, d in 0..3 and d' in 0..2 per (row or
//            column, scale block); C = ga * q, ga odd, |ga| < 2^20.
//   stage 5  32x32x64   e3m2 x e2m1 (6 x 4 dwords), free codes; d in 0..3, d' in 0..1.
//   stage 6  32x32x64   e4m3 x e2m1 (8 x 4 dwords), the MXFP4-weights by fp8-activations
//            pairing: A = any sign and mantissa with the row's exponent field
//            Ea_i in 1..14, B = free codes; d and d' in 0..3.
//   stage 7  16x16x128  e2m1 x e2m1, free codes, 128 terms, 4 scale blocks; d and d' in 0..3.
// Scale byte select: stage s takes byte s&3 for A and 3-(s&3) for B. The
// one-hot k of row / column rc is (rc + 16 * (wave nonce & 3)) mod 64
// in stages 0..2: the four waves of a workgroup take all four rotations and
// together select every one of the 64 positions. Stage 3 takes
// (rc + 16 * (wave nonce & 7)) mod 128: a workgroup's waves select 64
// consecutive positions and workgroups wg and wg ^ 4 together all 128.
//
// Stages 0..3 have one non-zero term each, a 9-bit integer at most times a
// power of two in 2^-65..2^70: a normal f32, exact under any correct
// implementation whatsoever.
//
// Why stages 4..7 are exact. Let U = (A's quantum) * (B's quantum) *
// 2^(SA_i+SB_j-254), in stage 6 times 2^(Ea_i-1), and q = U / 2. Every
// product is ua * ub * 2^(d+d') * U, an even integer multiple of q, and
// C = ga * q is an odd one. The sum of the magnitudes of all terms and C, in
// units of q, is at most
//   stage 4:  2 * 64 * 60 * 60 * 2^5  + 2^20 = 15 794 176
//   stage 5:  2 * 64 * 448 * 12 * 2^4 + 2^20 = 12 058 624
//   stage 6:  2 * 64 * 15 * 12 * 2^6  + 2^20 =  2 523 136
//   stage 7:  2 * 128 * 12 * 12 * 2^6 + 2^20 =  3 407 872
// all below 2^24 = 16 777 216. So every partial sum in every order and tree
// shape is an integer multiple of q below 2^24 q: it fits an f32 significand,
// and a unit that keeps at least 24 significant bits below its largest term
// when it aligns loses nothing (the fp8 check's one assumption). The final
// sum is odd, so never zero. q lies in 2^-41..2^32: every output is a normal
// f32. No output word of any stage is zero.
//
// The same argument makes a k-ordered f32 fmaf chain exact. The operands are
// decoded to f32 by integer bit arithmetic (dpf6_decode: no v_cvt of fp6 or
// fp4, which would be another copy of the decoder under test) and a block's
// scale is applied as an exact power of two; the kernel's on-device comparison
// and the host's recomputation both do that, and compare words, not floats.
#pragma once

#include <stdint.h>

#define MI355X_DPF6_THREADS 256
#define MI355X_DPF6_STAGES 8
#define MI355X_DPF6_TILE 1024                      // words of a 32x32 tile
#define MI355X_DPF6_TILE16 256                     // words of the 16x16 tiles of stages 3 and 7
#define MI355X_DPF6_WG_WORDS (6 * MI355X_DPF6_TILE + 2 * MI355X_DPF6_TILE16)
#define MI355X_DPF6_REC_WORDS 16
#define MI355X_DPF6_MAGIC 0x44504636u /* "DPF6" */
// record words (one record per workgroup)
#define MI355X_DPF6REC_MAGIC 0
#define MI355X_DPF6REC_WG 1
#define MI355X_DPF6REC_NONCE 2   // nonce ^ wg
#define MI355X_DPF6REC_XCC 3
#define MI355X_DPF6REC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPF6REC_BAD 8     // 8 words: per stage, MFMA elements (all waves) differing from the recomputation

// explicit kernel arguments (24 bytes; the kernel uses no hidden args)
struct mi355x_datapath_f6f4_args {
  uint32_t* records;  // host-visible, grid * MI355X_DPF6_REC_WORDS
  uint32_t* tiles;    // host-visible, grid * MI355X_DPF6_WG_WORDS (wave 0's eight tiles per workgroup)
  uint32_t nonce;
  uint32_t grid;      // workgroups launched; a workgroup beyond it writes nothing
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it):
  // one wrong accumulator word after a stage's MFMA, before the comparison and
  // the tile store. Runtime arguments; an index that names no accumulator
  // register does nothing. The fields mirror mi355x_datapath_fp8_args'.
  uint32_t inject_kind;   // MI355X_DPF6_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;   // 0..3
  uint32_t inject_lane;   // 0..63
  uint32_t inject_index;  // stage * 16 + accumulator register (stages 3 and 7 have registers 0..3)
  uint32_t inject_mask;   // xor-ed into that word
#endif
};

#define MI355X_DPF6_INJECT_NONE 0
#define MI355X_DPF6_INJECT_MFMA 1

#if defined(__HIPCC__)
#define MI355X_DPF6_HD __host__ __device__ constexpr
#else
#define MI355X_DPF6_HD static constexpr
#endif

// operand index spaces of dpf6_hash
#define MI355X_DPF6_IDX_A 0x0000u       // + (row * 4 + group) * 8 + element / 4: four 8-bit draws
#define MI355X_DPF6_IDX_B 0x1000u       // + (col * 4 + group) * 8 + element / 4
#define MI355X_DPF6_IDX_C 0x2000u       // + row * 32 + col
#define MI355X_DPF6_IDX_HOT 0x3000u     // + row / col of a one-hot operand: bit 31 = minus, low bits: p
#define MI355X_DPF6_IDX_EA 0x3900u      // + row: stage 6's e4m3 exponent field
#define MI355X_DPF6_IDX_SCALE_A 0x4000u // + row * 4 + scale block: the scale byte (stages 0..3) or d (stages 4..7)
#define MI355X_DPF6_IDX_SCALE_B 0x4800u // + col * 4 + scale block
#define MI355X_DPF6_IDX_SA 0x5000u      // + row: SA_i of stages 4..7
#define MI355X_DPF6_IDX_SB 0x5100u      // + col: SB_j

#define MI355X_DPF6_E4M3 0u             // the formats are named by their cbsz / blgp selector
#define MI355X_DPF6_E2M3 2u
#define MI355X_DPF6_E3M2 3u
#define MI355X_DPF6_E2M1 4u
#define MI355X_DPF6_SCALE_LO 97u        // scale band bytes: 97..158
#define MI355X_DPF6_SCALE_N 62u
#define MI355X_DPF6_SBASE_LO 112u       // SA_i, SB_j: 112..142
#define MI355X_DPF6_SBASE_N 31u

// per format (selector 1, e5m2, is not used): mantissa bits, exponent bits, bias, bits of an element
MI355X_DPF6_HD uint32_t dpf6_mant_bits(uint32_t fmt) { return (0x12323u >> (4u * fmt)) & 15u; }
MI355X_DPF6_HD uint32_t dpf6_exp_bits(uint32_t fmt) { return (0x23254u >> (4u * fmt)) & 15u; }
MI355X_DPF6_HD uint32_t dpf6_bias(uint32_t fmt) { return (0x131F7u >> (4u * fmt)) & 15u; }
MI355X_DPF6_HD uint32_t dpf6_width(uint32_t fmt) { return 1u + dpf6_exp_bits(fmt) + dpf6_mant_bits(fmt); }
MI355X_DPF6_HD uint32_t dpf6_dwords(uint32_t fmt) { return dpf6_width(fmt); }  // 32 elements: as many dwords as bits
// x of the format's quantum 2^x
MI355X_DPF6_HD int32_t dpf6_quantum_exp(uint32_t fmt) {
  return 1 - static_cast<int32_t>(dpf6_bias(fmt) + dpf6_mant_bits(fmt));
}
// hot codes: +-2^p units, p below this
MI355X_DPF6_HD uint32_t dpf6_hot_n(uint32_t fmt) { return dpf6_mant_bits(fmt) + (1u << dpf6_exp_bits(fmt)) - 1u; }

MI355X_DPF6_HD uint32_t dpf6_dim(uint32_t stage) { return (stage & 3u) == 3u ? 16u : 32u; }
MI355X_DPF6_HD uint32_t dpf6_groups(uint32_t stage) { return (stage & 3u) == 3u ? 4u : 2u; }  // lane groups = scale blocks
MI355X_DPF6_HD uint32_t dpf6_product(uint32_t stage) { return stage >= 4u; }
// the format of A (which = 0) or B (which = 1)
MI355X_DPF6_HD uint32_t dpf6_fmt(uint32_t stage, uint32_t which) {
  return ((which ? 0x44423244u : 0x40324432u) >> (4u * stage)) & 7u;
}
MI355X_DPF6_HD uint32_t dpf6_onehot(uint32_t stage, uint32_t which) {
  return which ? (stage == 0u || stage == 2u) : (stage == 1u || stage == 3u);
}
MI355X_DPF6_HD uint32_t dpf6_tile_offset(uint32_t stage) {
  return stage * MI355X_DPF6_TILE - (stage > 3u ? MI355X_DPF6_TILE - MI355X_DPF6_TILE16 : 0u);
}
// the byte (op_sel) of the scale VGPR a stage takes: `which` 0 = A, 1 = B
MI355X_DPF6_HD uint32_t dpf6_scale_sel(uint32_t stage, uint32_t which) { return which ? 3u - (stage & 3u) : stage & 3u; }
// the values d (which = 0) or d' (which = 1) of a product stage takes: 0 .. this - 1
MI355X_DPF6_HD uint32_t dpf6_delta_n(uint32_t stage, uint32_t which) {
  return which && stage == 4u ? 3u : which && stage == 5u ? 2u : 4u;
}

MI355X_DPF6_HD uint32_t dpf6_wave_nonce(uint32_t nonce, uint32_t wg, uint32_t wave) {
  return (nonce ^ (wg * 0x9E3779B1u)) + wave * 0x85EBCA77u;
}

MI355X_DPF6_HD uint32_t dpf6_hash(uint32_t nw, uint32_t stage, uint32_t idx) {
  uint32_t h = nw ^ ((stage + 0x6Fu) * 0x9E3779B1u) ^ (idx * 0x85EBCA77u);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

// the k of element e (0..31) of the fragment of lane group `group` of an operand of format fmt, and back
MI355X_DPF6_HD uint32_t dpf6_k(uint32_t stage, uint32_t fmt, uint32_t group, uint32_t e) {
  if (dpf6_width(fmt) != 8u) return 32u * group + e;
  return 16u * dpf6_groups(stage) * (e >> 4) + 16u * group + (e & 15u);
}
MI355X_DPF6_HD uint32_t dpf6_group_of(uint32_t stage, uint32_t fmt, uint32_t k) {
  return dpf6_width(fmt) != 8u ? k >> 5 : (k >> 4) & (dpf6_groups(stage) - 1u);
}
MI355X_DPF6_HD uint32_t dpf6_elem_of(uint32_t stage, uint32_t fmt, uint32_t k) {
  return dpf6_width(fmt) != 8u ? k & 31u : (k & 15u) + 16u * (k / (16u * dpf6_groups(stage)));
}

// the k, 0..63 or 0..127, where row / column rc of a one-hot operand is not zero
MI355X_DPF6_HD uint32_t dpf6_onehot_pos(uint32_t nw, uint32_t stage, uint32_t rc) {
  return dpf6_dim(stage) == 16u ? (rc + 16u * (nw & 7u)) & 127u : (rc + 16u * (nw & 3u)) & 63u;
}

// the code there: +-2^p units; below the first normal a single mantissa bit, from there on the exponent field
MI355X_DPF6_HD uint32_t dpf6_onehot_code(uint32_t nw, uint32_t stage, uint32_t fmt, uint32_t rc) {
  const uint32_t h = dpf6_hash(nw, stage, MI355X_DPF6_IDX_HOT + rc);
  const uint32_t mb = dpf6_mant_bits(fmt);
  const uint32_t p = (h & 0xFFFFu) % dpf6_hot_n(fmt);
  return ((h >> 31) << (dpf6_width(fmt) - 1u)) | (p < mb ? 1u << p : (p - mb + 1u) << mb);
}

// stage 6: the exponent field of row `row` of the e4m3 operand, 1..14
MI355X_DPF6_HD uint32_t dpf6_row_exp(uint32_t nw, uint32_t stage, uint32_t row) {
  return 1u + dpf6_hash(nw, stage, MI355X_DPF6_IDX_EA + row) % 14u;
}

// element e (0..31) of the fragment of (row / column rc, lane group `group`) of A (which = 0) or B (1): its code
MI355X_DPF6_HD uint32_t dpf6_elem(uint32_t stage, uint32_t which, uint32_t rc, uint32_t group, uint32_t e,
                                  uint32_t nw) {
  const uint32_t fmt = dpf6_fmt(stage, which);
  const uint32_t low = dpf6_width(fmt) - 1u;  // bits below the sign
  if (dpf6_onehot(stage, which))
    return dpf6_onehot_pos(nw, stage, rc) == dpf6_k(stage, fmt, group, e) ? dpf6_onehot_code(nw, stage, fmt, rc) : 0u;
  const uint32_t draw = dpf6_product(stage) ? e : e & 15u;  // a band fragment draws 16 codes
  const uint32_t h8 = (dpf6_hash(nw, stage, (which ? MI355X_DPF6_IDX_B : MI355X_DPF6_IDX_A) + (rc * 4u + group) * 8u +
                                                (draw >> 2)) >> (8u * (draw & 3u))) & 0xFFu;
  if (fmt == MI355X_DPF6_E4M3) return (h8 & 0x87u) | (dpf6_row_exp(nw, stage, rc) << 3);
  const uint32_t sign = (h8 >> 7) << low;
  if (dpf6_product(stage)) return sign | (1u + (((h8 & 0x7Fu) * ((1u << low) - 1u)) >> 7));  // free: 1 .. 2^low - 1
  const uint32_t code = sign | (1u + (((h8 & 0x7Fu) * ((1u << low) - 2u)) >> 7));            // band: 1 .. 2^low - 2
  return (e & 16u) ? code ^ ((2u << low) - 1u) : code;
}

// dword `dword` (0..7) of that fragment: the elements as the fields of a little-endian bit stream, zero
// beyond the format's dwords
MI355X_DPF6_HD uint32_t dpf6_word(uint32_t stage, uint32_t which, uint32_t rc, uint32_t group, uint32_t dword,
                                  uint32_t nw) {
  const int32_t w = static_cast<int32_t>(dpf6_width(dpf6_fmt(stage, which)));
  uint32_t out = 0;
  for (int32_t e = 0; e < 32; ++e) {
    const int32_t shift = e * w - 32 * static_cast<int32_t>(dword);
    if (shift <= -w || shift >= 32) continue;
    const uint32_t code = dpf6_elem(stage, which, rc, group, static_cast<uint32_t>(e), nw);
    out |= shift >= 0 ? code << shift : code >> -shift;
  }
  return out;
}

// SA_i (which = 0) or SB_j (which = 1) of the product stages; the scale band's low end in stages 0..3
MI355X_DPF6_HD uint32_t dpf6_scale_base(uint32_t nw, uint32_t stage, uint32_t which, uint32_t rc) {
  if (!dpf6_product(stage)) return MI355X_DPF6_SCALE_LO;
  return MI355X_DPF6_SBASE_LO +
         dpf6_hash(nw, stage, (which ? MI355X_DPF6_IDX_SB : MI355X_DPF6_IDX_SA) + rc) % MI355X_DPF6_SBASE_N;
}

// the E8M0 scale of scale block `block` of row / column rc of A (which = 0) or B (which = 1): what lane
// (rc, lane group `block`) holds in the selected byte of its scale VGPR
MI355X_DPF6_HD uint32_t dpf6_scale_byte(uint32_t nw, uint32_t stage, uint32_t which, uint32_t rc, uint32_t block) {
  const uint32_t h =
      dpf6_hash(nw, stage, (which ? MI355X_DPF6_IDX_SCALE_B : MI355X_DPF6_IDX_SCALE_A) + rc * 4u + block);
  return dpf6_scale_base(nw, stage, which, rc) +
         h % (dpf6_product(stage) ? dpf6_delta_n(stage, which) : MI355X_DPF6_SCALE_N);
}

// the scale VGPR of that lane: the scale in the byte the stage selects, three other band values, all four
// different, in the rest
MI355X_DPF6_HD uint32_t dpf6_scale_word(uint32_t nw, uint32_t stage, uint32_t which, uint32_t rc, uint32_t block) {
  const uint32_t s = dpf6_scale_byte(nw, stage, which, rc, block) - MI355X_DPF6_SCALE_LO;
  const uint32_t sel = dpf6_scale_sel(stage, which);
  uint32_t w = 0;
  for (uint32_t p = 0; p < 4u; ++p)
    w |= (MI355X_DPF6_SCALE_LO + (s + ((p - sel) & 3u) * 15u) % MI355X_DPF6_SCALE_N) << (8u * p);
  return w;
}

// product stages: x of q = 2^x, of which C and every product of D[row][col] are multiples
MI355X_DPF6_HD int32_t dpf6_quantum(uint32_t nw, uint32_t stage, uint32_t row, uint32_t col) {
  const uint32_t fa = dpf6_fmt(stage, 0u);
  int32_t x = dpf6_quantum_exp(fa) + dpf6_quantum_exp(dpf6_fmt(stage, 1u)) - 1;
  if (fa == MI355X_DPF6_E4M3) x += static_cast<int32_t>(dpf6_row_exp(nw, stage, row)) - 1;
  return x + static_cast<int32_t>(dpf6_scale_base(nw, stage, 0u, row) + dpf6_scale_base(nw, stage, 1u, col)) - 254;
}

// the f32 bit pattern of +-mag * 2^x, 0 < mag < 2^24: built from integers
// (normalise, then place the exponent), the same on host and device
MI355X_DPF6_HD uint32_t dpf6_int_f32(uint32_t sign, uint32_t mag, int32_t x) {
  const uint32_t top = 31u - static_cast<uint32_t>(__builtin_clz(mag));  // position of the leading one
  return (sign << 31) | (static_cast<uint32_t>(127 + static_cast<int32_t>(top) + x) << 23) |
         ((mag << (23u - top)) & 0x7FFFFFu);
}

MI355X_DPF6_HD uint32_t dpf6_c_word(uint32_t stage, uint32_t row, uint32_t col, uint32_t nw) {
  if (!dpf6_product(stage)) return 0u;
  const uint32_t h = dpf6_hash(nw, stage, MI355X_DPF6_IDX_C + row * 32u + col);
  return dpf6_int_f32(h >> 31, (h & 0xFFFFFu) | 1u, dpf6_quantum(nw, stage, row, col));  // ga odd, < 2^20
}

// the f32 word with the value of a code, by integer arithmetic alone: a normal
// keeps its mantissa under the rebiased exponent, a subnormal is normalised,
// zero keeps its sign
MI355X_DPF6_HD uint32_t dpf6_decode(uint32_t code, uint32_t fmt) {
  const uint32_t mb = dpf6_mant_bits(fmt);
  const uint32_t sign = code >> (dpf6_width(fmt) - 1u);
  const uint32_t field = (code >> mb) & ((1u << dpf6_exp_bits(fmt)) - 1u), m = code & ((1u << mb) - 1u);
  if (field) return (sign << 31) | ((field + 127u - dpf6_bias(fmt)) << 23) | (m << (23u - mb));
  return m ? dpf6_int_f32(sign, m, dpf6_quantum_exp(fmt)) : sign << 31;
}

// the f32 word of 2^(s-127) for a scale byte
MI355X_DPF6_HD uint32_t dpf6_scale_f32(uint32_t s) { return s << 23; }
