// Shared between the gfx950 MX quantise kernels (mi355x_mxquant_fill,
// mi355x_mfma_datapath_mxquant), the host verdict (datapath_mxquant_verify.h) and
// native/tests/datapath_mxquant_contract_cli.cpp.
//
// The twelve checks before this one take their low-precision operands ready-made.
// A tenant's MXFP4 MLP quantises its activations on the device, between two
// GEMMs: an f32 accumulator tile, the absolute maximum of each 32-wide block, the
// E8M0 scale from the maximum's exponent, the scaled conversion to packed e2m1
// (v_cvt_scalef32_pk_fp4_f32, new on gfx950), LDS, the next scaled MFMA. This
// check is that step, small and bit-exact; it is the one user of the scaled
// conversion unit among the checks.
//
// Problem. `grid` workgroups of 256 lanes; workgroup wg runs, for its own 128
// tokens,
//   for slab s in 0 .. hsteps-1:                       hidden columns 128 s .. 128 s + 127
//     H_s = X_wg . W1_s^T                               bf16 x bf16 -> f32, K1 = 128
//     (E, Q) = mx_quantise(H_s)                         per token and 32 hidden columns
//     Y += Q 2^(E-127) . (W2_s 2^(sb-127))^T            v_mfma_scale_f32_32x32x64_f8f6f4, e2m1 x e2m1
// X_wg [128][128] bf16 is the workgroup's own panel; W1 [128 hsteps][128] bf16,
// W2 [128][128 hsteps] e2m1 (K-major, element n in bits 4*(n&1).. of byte n/2)
// and W2's scale bytes sb [128][4 hsteps] are shared and read through L2.
// mi355x_mxquant_fill writes them from the hash, 16 bytes a store. Y (f32
// [wg][128][128]), the quantised image as the second GEMM read it out of LDS
// ([wg]: 128 x 64 hsteps code bytes, then 128 x 4 hsteps scale bytes) and the
// records go to host-visible memory.
//
// mx_quantise is the OCP MX rule in integers: with ef the exponent field of the
// block's f32 amax, E = max(ef, 3) - 2 (2 = e2m1's largest exponent; the clamp
// only defines a block of zeros or denormal-range values, which the recipe has
// none of), and every element is round_to_nearest_even(h * 2^-(E-127)) on the
// e2m1 grid 0, 0.5, 1, 1.5, 2, 3, 4, 6, saturated to +-6. The kernel takes ef by
// a shift of the amax word and hands the conversion the f32 word E << 23: no
// division, reciprocal or logarithm. Byte k of a block holds columns 2k (low
// nibble, the conversion's first source) and 2k + 1.
//
// Operands, and why every word is exact in any order.
//   X, W1   the attention check's device (dpat_score). K1 is 64 pairs (2p, 2p+1).
//           A hash bit per pair picks its shape: shape 0 has the X pair (a, a)
//           and the W1 pair (x, -x), shape 1 (a, 2a) and (2x, -x); every pair
//           cancels to 0. Hidden column n has two live pairs, p0 < 32 <= p1,
//           where W1's first element is increased by t0, t1. So
//             H[i][n] = S_in 2^(g_i + f_b),  S_in = a(i,p0) t0(n) + a(i,p1) t1(n)
//           with b = n >> 5, g_i in -24..24 the row's exponent, f_b = (b ^ r) & 1
//           the block's (neighbouring blocks always differ). X = a 2^g_i and
//           W1 = w 2^f_b with |a| <= 6, 1 <= |w| <= 25: non-zero, exact bf16;
//           every GEMM-1 partial sum is an integer below 2^15 times 2^(g_i+f_b).
//   S       a(i, p < 32) and t0 are odd, t1 is even: S is odd, so no element and
//           no block is zero. A row is low (|a| = 1) or high (|a| in 1, 3 for
//           p < 32; 1, 2, 3 for p >= 32); a block has class 0 (|t0| = 1,
//           |t1| = 2), 1 (|t0| in 1, 3) or 2 (|t0| in 1, 3, 5; |t1| in 2, 4).
//           |S| <= 27 (the issue's 31 narrowed by the even / odd split), and the
//           block maxima spread over the binades 1..4: lg = floor(log2 max|S|)
//           in 0..4 is the data-dependent part of E = 125 + lg + g_i + f_b, in
//           101..154. S / 2^(lg-2) is odd quarters, halves or whole numbers, which
//           lands on every case of the conversion's rule (exact, down, up, ties
//           to even both ways, the ties around 0.5, 0.25 -> 0, above 6).
//   W2, sb  free e2m1 codes (dpmx_codes: never +-0); sb = SB_j + d', SB_j in
//           112..142, d' in 0..1 per (column, block).
//   Y       with uq, uw the elements in units of 2^-1, a product is
//             uq uw 2^(lg + f_b + d') 2^(g_i + SB_j - 131),
//           an even multiple of q = 2^(g_i + SB_j - 132); C = ga q, ga odd,
//           |ga| < 2^20, so no output word is zero. |uq| 2^lg <= 12 * 16 (S = 27
//           saturates to 6 at lg = 4), so all magnitudes sum, in quanta, to at most
//             2 * 128 hsteps * 12 * 12 * 2^(4+1+1) + 2^20 = 10 485 760   at hsteps 4
//           below 2^24. f_b is one bit wide for that reason: a second bit would
//           need hsteps <= 3. Every partial sum of Y, in every order, is exact.
//
// Kernel design (datapath_mxquant_kernel.hip).
//   GEMM 1   transposed, as the attention check's S^T, so that one lane owns one
//            token: H_s^T = W1_s . X^T by v_mfma_f32_32x32x16_bf16. Wave w serves
//            tokens 32w..32w+31; its X fragments (8 k-chunks x 16 bytes a lane)
//            are loaded once from global memory and never enter LDS. A 32x32
//            accumulator is one quantisation block of 32 tokens: register r of
//            lane l is hidden column (r&3) + 8*(r>>2) + 4*(l>>5) of token l&31,
//            lane l^32 holds the other 16 columns.
//   W1 feed  a slab is 128 rows x 256 bytes: two k-halves, each a 128-row x
//            128-byte tile with the GEMM check's A swizzle (dpgm_lds_a), in two
//            LDS buffers of 32 KiB, filled by global_load_lds_dwordx4 a slab
//            ahead, read by ds_read_b128.
//   W2 feed  a slab is 128 columns x 64 bytes (8 KiB), two buffers, the same
//            loads; its four scale bytes a column come by global_load_dword a
//            slab ahead.
//   quantise v_max3_f32 over the 16 registers' magnitudes, one v_permlane32_swap
//            with lane l^32 and a final max; ef, E and the scale word by integer
//            ops; eight v_cvt_scalef32_pk_fp4_f32 on the register pairs (r, r+1),
//            four bytes a dword: d0 = columns {0..3, 8..11} + 4*(l>>5), d1 =
//            {16..19, 24..27} + 4*(l>>5).
//   Q tile   128 token rows x 64 bytes and 128 scale dwords. The block's 16
//            bytes interleave 2-byte pieces of lanes l and l^32. One
//            v_permlane32_swap gives lane pair (l, l^32) the two dwords of one
//            8-byte half each, two v_perm_b32 interleave them, one ds_write_b64
//            stores the half. Lanes with bit 4 set take the other half, so the
//            32 lanes of a write pass cover 16 chunks x 2 halves.
//   swizzle  of the Q tile and of the W2 tile (rows of 64 bytes, four 16-byte
//            chunks): position p = c ^ ((r >> 2) & 3). Bank arithmetic (64
//            banks of 4 bytes = 256 bytes). Read: a ds_read_b128 is served 16
//            lanes at a time, rows r0..r0+15 at one chunk c; row r starts at
//            byte 64 r, so r & 3 picks the 64-byte quarter and (r >> 2) & 3
//            takes all four values: 16 different 16-byte groups, no conflict.
//            Write: 32 lanes of a ds_write_b64 write rows r0..r0+31 of one
//            block; rows r and r+16 share a 16-byte group and the half bit
//            above separates them: all 64 banks once. (From the arithmetic;
//            the conflict counters were not read.)
//   GEMM 2   the mxgemm check's loop: waves as 2 x 2, wave v owns rows
//            64*(v>>1).., columns 64*(v&1).., four 32x32 accumulators; after a
//            barrier lane l reads the 16 bytes of row (l&31) at chunk
//            2*kk + (l>>5) (one read is one fragment, one scale block) and the
//            row's scale dword; v_perm_b32 gathers bytes (h, 2+h, h, 2+h) for
//            lane group h, and the MFMA of sub-step kk takes byte
//            2*(s&1) + kk (op_sel) of both scale VGPRs: two slabs use all four.
//            The tokens a wave quantised are not the tokens it multiplies.
//
// Record (32 words a workgroup): magic, workgroup, nonce ^ wg, XCC id with
// hsteps in bits 8.., HW_ID of the four waves, and per wave six fold words (xor
// and sum modulo 2^32 over dwords): of the W1 fragments, of the W2 fragments, of
// the four gathered scale VGPRs (once a slab) it fed to its MFMAs.
// Stages: 0 = W1 feed (word = wg * 16 + wave * 2 + {0 xor, 1 sum}), 1 = W2 and
// scale feed (wg * 16 + wave * 4 + {W2 xor, W2 sum, scale xor, scale sum}),
// 2 = the quantised image in dwords (wg * 2176 hsteps + index: 128 rows of
// 16 hsteps code dwords, then 128 rows of hsteps scale dwords), 3 = Y words
// (wg * 16384 + row * 128 + column).
#pragma once

#include <stdint.h>

#include "datapath_attn_kernel.h"
#include "datapath_mxgemm_kernel.h"

#define MI355X_DPMQ_THREADS 256
#define MI355X_DPMQ_TILE 128                       // tokens = output columns = hidden columns of a slab = K1
#define MI355X_DPMQ_HSTEPS 4                       // production: hidden 512
#define MI355X_DPMQ_HSTEPS_MAX 4                   // the bound above
#define MI355X_DPMQ_WG_WORDS (MI355X_DPMQ_TILE * MI355X_DPMQ_TILE)
#define MI355X_DPMQ_IMG_WORDS(hsteps) (2176u * (hsteps))  // 128 * 16 code dwords + 128 scale dwords a slab
#define MI355X_DPMQ_REC_WORDS 32
#define MI355X_DPMQ_MAGIC 0x44504D51u /* "DPMQ" */
#define MI355X_DPMQ_STAGES 4                       // 0 = W1 feed, 1 = W2 and scale feed, 2 = quantised image, 3 = Y words
// record words (one record per workgroup)
#define MI355X_DPMQREC_MAGIC 0
#define MI355X_DPMQREC_WG 1
#define MI355X_DPMQREC_NONCE 2   // nonce ^ wg
#define MI355X_DPMQREC_XCC 3     // XCC id in bits 0..3, hsteps in bits 8..
#define MI355X_DPMQREC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPMQREC_FOLD 8    // 24 words: wave * 6 + {W1, W2, scales} * 2 + {xor, sum}
// LDS
#define MI355X_DPMQ_LDS_W1_BYTES 32768             // a slab of W1: two k-halves of 16 KiB
#define MI355X_DPMQ_LDS_W2_BYTES 8192              // a slab of W2, and the Q tile

// explicit kernel arguments of both kernels (72 bytes; they use no hidden args)
struct mi355x_datapath_mxquant_args {
  uint32_t* records;  // host-visible, grid * MI355X_DPMQ_REC_WORDS
  uint32_t* tiles;    // host-visible, grid * MI355X_DPMQ_WG_WORDS: Y, word = row * 128 + column
  uint32_t* image;    // host-visible, grid * MI355X_DPMQ_IMG_WORDS(hsteps): the quantised image
  uint16_t* x;        // device, grid * 128 * 128 bf16: X_wg at wg * 16384, [token][k]
  uint16_t* w1;       // device, 128 hsteps * 128 bf16, [hidden][k]
  uint8_t* w2;        // device, 128 * 64 hsteps bytes, [column][hidden / 2]
  uint8_t* sb;        // device, 128 * 4 hsteps bytes, [column][block]
  uint32_t nonce;
  uint32_t grid;      // workgroups; a workgroup beyond it reads and writes nothing
  uint32_t hsteps;    // hidden / 128
  uint32_t pad;
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it).
  // Runtime arguments, the siblings' six fields:
  //   H      before the quantisation, GEMM-1 accumulator word `index` (slab * 64 +
  //          block of the slab * 16 + register) of lane `lane` of wave `wave` of
  //          workgroup `wg` is xor-ed with `mask`
  //   Q      after the barrier behind the quantisation of slab `wave` (the field
  //          carries the slab), dword `index` (0..2047) of the Q tile of
  //          workgroup `wg` is xor-ed with `mask`
  //   SCALE  before sub-step (index >> 2) & 1 of slab index >> 3, gathered scale
  //          VGPR index & 3 (the activations' row blocks 0 and 1, then W2's
  //          column blocks) of lane `lane` of wave `wave` of workgroup `wg` is
  //          xor-ed with `mask`; it stays so to the end of the slab, where the
  //          VGPRs are folded
  //   MFMA   after the loop, Y accumulator word `index` (32x32 block * 16 +
  //          register) of that lane is xor-ed with `mask`
  uint32_t inject_kind;   // MI355X_DPMQ_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;
  uint32_t inject_lane;
  uint32_t inject_index;
  uint32_t inject_mask;
#endif
};

#define MI355X_DPMQ_INJECT_NONE 0
#define MI355X_DPMQ_INJECT_H 1
#define MI355X_DPMQ_INJECT_Q 2
#define MI355X_DPMQ_INJECT_SCALE 3
#define MI355X_DPMQ_INJECT_MFMA 4

// index spaces of dpbf_hash, after the MXFP4 GEMM check's
#define MI355X_DPMQ_SPACE_SHAPE 0x70u  // idx = pair, seed = the nonce: bit 0 is the pair's shape
#define MI355X_DPMQ_SPACE_A 0x71u      // idx = token * 64 + pair, seed = the workgroup's
#define MI355X_DPMQ_SPACE_ROW 0x72u    // idx = token, seed = the workgroup's: the row's class and g_i
#define MI355X_DPMQ_SPACE_WX 0x73u     // idx = hidden * 64 + pair, seed = the nonce
#define MI355X_DPMQ_SPACE_LIVE 0x74u   // idx = hidden, seed = the nonce: the live pairs and t0, t1
#define MI355X_DPMQ_SPACE_BLK 0x75u    // idx = block, seed = the nonce: the block's class; idx 0xFFFF: r of f_b
#define MI355X_DPMQ_SPACE_W2 0x76u     // idx = column * (16 hsteps) + hidden / 8, seed = the nonce
#define MI355X_DPMQ_SPACE_SB 0x77u     // idx = column: SB_j
#define MI355X_DPMQ_SPACE_DB 0x78u     // idx = column * 64 + block: d'
#define MI355X_DPMQ_SPACE_C 0x79u      // idx = row * 128 + column, seed = the workgroup's
#define MI355X_DPMQ_SPACE_XV 0x7Au     // idx = column: the verdict's second projection vector

MI355X_DPMX_HD bool dpmq_sizes_ok(uint32_t grid, uint32_t hsteps) {
  return grid != 0u && grid <= 1024u && hsteps != 0u && hsteps <= MI355X_DPMQ_HSTEPS_MAX;
}

MI355X_DPMX_HD uint32_t dpmq_wg_seed(uint32_t nonce, uint32_t wg) { return dpbf_wave_nonce(nonce, wg, 0u); }
MI355X_DPMX_HD uint32_t dpmq_shape(uint32_t nonce, uint32_t pair) { return dpbf_hash(nonce, MI355X_DPMQ_SPACE_SHAPE, pair) & 1u; }

// the row's hash: bit 0 = high row, g_i = dpmq_g(h)
MI355X_DPMX_HD uint32_t dpmq_row(uint32_t seed, uint32_t token) { return dpbf_hash(seed, MI355X_DPMQ_SPACE_ROW, token); }
MI355X_DPMX_HD int32_t dpmq_g(uint32_t row_hash) { return static_cast<int32_t>((row_hash >> 8) % 49u) - 24; }

// a of (token, pair): +-1 in a low row; in a high row +-{1,3} for pair < 32, +-{1,2,3} for the others
MI355X_DPMX_HD int32_t dpmq_a(uint32_t seed, uint32_t row_hash, uint32_t token, uint32_t pair) {
  const uint32_t h = dpbf_hash(seed, MI355X_DPMQ_SPACE_A, token * 64u + pair);
  int32_t mag = 1;
  if (row_hash & 1u) mag = pair < 32u ? 1 + 2 * static_cast<int32_t>(h & 1u) : 1 + static_cast<int32_t>((h & 0xFFFFu) % 3u);
  return (h >> 31) ? -mag : mag;
}

// x = +-{6..10} of (hidden, pair): |x| > |t|, so no element of W1 is zero
MI355X_DPMX_HD int32_t dpmq_x(uint32_t nonce, uint32_t hidden, uint32_t pair) {
  const uint32_t h = dpbf_hash(nonce, MI355X_DPMQ_SPACE_WX, hidden * 64u + pair);
  const int32_t mag = 6 + static_cast<int32_t>((h & 0xFFFFu) % 5u);
  return (h >> 31) ? -mag : mag;
}

MI355X_DPMX_HD uint32_t dpmq_block_class(uint32_t nonce, uint32_t block) { return dpbf_hash(nonce, MI355X_DPMQ_SPACE_BLK, block) % 3u; }
MI355X_DPMX_HD uint32_t dpmq_f(uint32_t nonce, uint32_t block) { return (block ^ dpbf_hash(nonce, MI355X_DPMQ_SPACE_BLK, 0xFFFFu)) & 1u; }

// the live pairs of a hidden column (p0 < 32 <= p1) and t0 (odd), t1 (even)
MI355X_DPMX_HD void dpmq_live(uint32_t nonce, uint32_t hidden, uint32_t pair[2], int32_t t[2]) {
  const uint32_t h = dpbf_hash(nonce, MI355X_DPMQ_SPACE_LIVE, hidden), cls = dpmq_block_class(nonce, hidden >> 5);
  pair[0] = h & 31u;
  pair[1] = 32u + ((h >> 5) & 31u);
  const int32_t m0 = 1 + 2 * static_cast<int32_t>(((h >> 10) & 0xFFu) % (cls + 1u));
  const int32_t m1 = 2 * (1 + static_cast<int32_t>(cls == 2u ? (h >> 18) & 1u : 0u));
  t[0] = ((h >> 20) & 1u) ? -m0 : m0;
  t[1] = ((h >> 21) & 1u) ? -m1 : m1;
}

// the bf16 of n * 2^x, n a non-zero integer of magnitude below 256
MI355X_DPMX_HD uint32_t dpmq_bf16(int32_t n, int32_t x) { return (dpat_bf16_int(n) + (static_cast<uint32_t>(x) << 7)) & 0xFFFFu; }

// the dword holding elements 2 * pair and 2 * pair + 1 of a row of X
MI355X_DPMX_HD uint32_t dpmq_x_dword(uint32_t nonce, uint32_t seed, uint32_t token, uint32_t pair) {
  const uint32_t rh = dpmq_row(seed, token);
  const int32_t a = dpmq_a(seed, rh, token, pair), g = dpmq_g(rh);
  return dpmq_bf16(a, g) | (dpmq_bf16(dpmq_shape(nonce, pair) ? 2 * a : a, g) << 16);
}

// likewise of a row of W1
MI355X_DPMX_HD uint32_t dpmq_w1_dword(uint32_t nonce, uint32_t hidden, uint32_t pair) {
  const int32_t x = dpmq_x(nonce, hidden, pair), f = static_cast<int32_t>(dpmq_f(nonce, hidden >> 5));
  uint32_t live[2];
  int32_t t[2];
  dpmq_live(nonce, hidden, live, t);
  int32_t first = dpmq_shape(nonce, pair) ? 2 * x : x;
  for (uint32_t i = 0; i < 2; ++i)
    if (live[i] == pair) first += t[i];
  return dpmq_bf16(first, f) | (dpmq_bf16(-x, f) << 16);
}

// dword kd (hidden 8 kd .. 8 kd + 7) of column `col` of W2: eight free codes
MI355X_DPMX_HD uint32_t dpmq_w2_dword(uint32_t nonce, uint32_t hsteps, uint32_t col, uint32_t kd) {
  return dpmx_codes(dpbf_hash(nonce, MI355X_DPMQ_SPACE_W2, col * (hsteps * 16u) + kd));
}

MI355X_DPMX_HD uint32_t dpmq_sb_base(uint32_t nonce, uint32_t col) {
  return MI355X_DPMX_SBASE_LO + dpbf_hash(nonce, MI355X_DPMQ_SPACE_SB, col) % MI355X_DPMX_SBASE_N;
}
MI355X_DPMX_HD uint32_t dpmq_sb_delta(uint32_t nonce, uint32_t col, uint32_t block) {
  return (dpbf_hash(nonce, MI355X_DPMQ_SPACE_DB, col * 64u + block) >> 13) & 1u;
}

MI355X_DPMX_HD int32_t dpmq_ga(uint32_t seed, uint32_t row, uint32_t col) {
  const uint32_t h = dpbf_hash(seed, MI355X_DPMQ_SPACE_C, row * 128u + col);
  const int32_t mag = static_cast<int32_t>((h & 0xFFFFFu) | 1u);  // odd, < 2^20
  return (h >> 31) ? -mag : mag;
}

// C of output (row, col): ga * q, q = 2^(g_i + SB_j - 132)
MI355X_DPMX_HD uint32_t dpmq_c_word(uint32_t seed, uint32_t nonce, uint32_t row, uint32_t col) {
  return dpbf_scaled_int(dpmq_ga(seed, row, col), dpmq_g(dpmq_row(seed, row)) + static_cast<int32_t>(dpmq_sb_base(nonce, col)) - 132);
}

// E8M0 byte of a block from the f32 word of its amax
MI355X_DPMX_HD uint32_t dpmq_e8m0(uint32_t amax_word) {
  const uint32_t ef = (amax_word >> 23) & 0xFFu;
  return (ef < 3u ? 3u : ef) - 2u;
}

// LDS byte offset of the 16-byte chunk (row, chunk 0..3) of a tile with 64-byte rows: the Q tile and the W2 tile
MI355X_DPMX_HD uint32_t dpmq_lds(uint32_t row, uint32_t c) { return row * 64u + ((c ^ ((row >> 2) & 3u)) << 4); }

// the scale VGPR lane group h feeds to a slab's MFMAs from the slab's four bytes: (h, 2+h, h, 2+h)
MI355X_DPMX_HD uint32_t dpmq_gather(uint32_t raw, uint32_t h) {
  const uint32_t two = ((raw >> (8u * h)) & 0xFFu) | (((raw >> (16u + 8u * h)) & 0xFFu) << 8);
  return two | (two << 16);
}

// where fold word `word` of feed stage `stage` sits in a record: stage 0 word = wave * 2 + {xor, sum} (W1), stage 1
// word = wave * 4 + {W2 xor, W2 sum, scale xor, scale sum}
MI355X_DPMX_HD uint32_t dpmq_fold_slot(uint32_t stage, uint32_t word) {
  return stage == 0u ? MI355X_DPMQREC_FOLD + (word >> 1) * 6u + (word & 1u) : MI355X_DPMQREC_FOLD + (word >> 2) * 6u + 2u + (word & 3u);
}
