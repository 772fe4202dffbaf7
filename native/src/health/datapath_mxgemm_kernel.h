// Shared between the gfx950 MXFP4 GEMM pipeline kernels (mi355x_mxgemm_fill,
// mi355x_mfma_datapath_mxgemm), the host verdict (datapath_mxgemm_verify.h) and
// native/tests/datapath_mxgemm_contract_cli.cpp.
//
// The fp6 / fp4 check (datapath_f6f4_kernel.h) drives the e2m1 decoder and the
// scale multiply with one instruction on operands made in registers. A tenant's
// MXFP4 GEMM streams packed 4-bit operands and a separate stream of E8M0 block
// scales out of HBM, the operands through LDS, the scales through registers,
// into long dependent chains of v_mfma_scale_f32_32x32x64_f8f6f4 whose scales
// change from block to block. This check is that pipeline, small and bit-exact.
// It has the shape of the bf16 GEMM check (datapath_gemm_kernel.h).
//
// Problem. `grid` workgroups of 256 lanes; workgroup wg computes the 128 x 128
// f32 tile
//   D_wg[i][j] = C_wg[i][j] + sum over k of A_wg[i][k] * B[j][k] * 2^(sa[i][k>>5]-127) * 2^(sb[j][k>>5]-127)
// A_wg is the workgroup's own panel, 128 x K e2m1, two elements a byte (element
// k in bits 4*(k&1).. of byte k/2), row-major, K/2 bytes a row; it streams from
// HBM. B is one panel, 128 x K e2m1, K-major ([column][k], as quantised weights
// are stored), read by every workgroup through L2. The scales are plain
// row-major E8M0 bytes, sa_wg[128][K/32] and sb[128][K/32], not pre-shuffled.
// K = ksteps * 256 with 1 <= ksteps <= MI355X_DPMX_KSTEPS_MAX.
// mi355x_mxgemm_fill writes operands and scales into device memory from the
// hash, with 16-byte vector stores, in a dispatch of its own on the same queue;
// D and the records go to host memory.
//
// Operands (stage 7 of the fp6 / fp4 check, stretched to a long K).
//   elements  e2m1 free codes: any code but +-0. A code is u units of the
//             quantum 2^-1, |u| one of 1, 2, 3, 4, 6, 8, 12. A dword of eight
//             codes is one hash word in which a nibble with no magnitude bit
//             gets magnitude 1.
//   scales    row i of A_wg has a base SA_i, column j of B a base SB_j, both in
//             112..142; the scale of (row i, scale block g) is SA_i + d, d in
//             0..3, of (column j, block g) SB_j + d', d' in 0..1, from the hash:
//             the scale changes from block to block inside a row.
//   C         C[i][j] = ga * q, ga odd, |ga| < 2^20, q = U / 2,
//             U = 2^-2 * 2^(SA_i+SB_j-254).
//
// Why every word is exact in any order. A product is ua * ub * 2^(d+d') * U, an
// even integer multiple of q; C is an odd one, so no output word is zero. The
// magnitudes of all K products and of C sum, in quanta q, to at most
//   2 * K * 12 * 12 * 2^4 + 2^20 = 10 485 760   at K = 2048 (ksteps 8)
// below 2^24 = 16 777 216 (K = 4096 would give 19 922 944: ksteps 8 is the
// largest whole power of two, hence MI355X_DPMX_KSTEPS_MAX). So every partial
// sum, in every order, tree shape and chain split, is an integer multiple of q
// below 2^24 q and fits an f32 significand; between two MFMAs of a chain it
// sits in an f32 register and is exact. q = 2^(SA_i+SB_j-257) lies in
// 2^-33..2^27 and the largest scale byte is 145: every output is a normal f32.
//
// Kernel design (datapath_mxgemm_kernel.hip).
//   waves    4, as 2 x 2: wave v owns rows 64*(v>>1).., columns 64*(v&1).. of the
//            tile, four 32x32 accumulators of v_mfma_scale_f32_32x32x64_f8f6f4
//            (cbsz = blgp = 4: e2m1), each a dependent chain of 4 * ksteps MFMAs.
//   LDS      two buffers of 32 KiB: a 128-row x 128-byte tile of A and one of B
//            (16 KiB each) per k-step of 256 elements.
//   loads    global_load_lds_dwordx4: 16 bytes a lane, a wave's 64 lanes land
//            in 1 KiB of consecutive LDS (8 rows), 8 wave-loads a wave a step.
//            The loads of step s+1 are issued before the MFMAs of step s; one
//            barrier a step.
//   swizzle  made on the global-address side, in units of 16-byte chunks, the
//            same for both tiles: the chunk at LDS position p of row r holds
//            k-chunk p ^ ((r >> 1) & 7). Bank arithmetic for the read below:
//            a ds_read_b128 is served a quarter-wave at a time, 16 lanes that
//            read rows r0..r0+15 (r0 a multiple of 16) at one k-chunk c. Row r
//            starts at byte 128 r, so within the 256 bytes the 64 banks span
//            the lane's chunk sits at 128 * (r & 1) + 16 * (c ^ ((r >> 1) & 7)):
//            r & 1 picks the half, and (r >> 1) & 7 takes all eight values
//            over the 16 rows, so the 16 lanes fall on 16 different 16-byte
//            bank groups: no conflict. Without the swizzle they would fall on
//            two. (From the arithmetic; the conflict counters were not read.)
//   reads    ds_read_b128 for both operands, none transposed. The 4-bit
//            fragment map measured for the fp6 / fp4 check: element e of lane
//            group h is k = 32*h + e, so for sub-step kk (64 k) lane l reads
//            the 16 bytes of row / column (l & 31) of its 32-row block at
//            k-chunk 2*kk + (l >> 5): one lane's fragment is one scale block.
//            The builtin's upper four dwords are zero.
//   scales   not through LDS. Per k-step a lane loads the 8 scale bytes of each
//            of its two rows and two columns (global_load_dwordx2), one step
//            ahead of use. v_perm_b32 gathers bytes h, 2+h, 4+h, 6+h into one
//            VGPR for lane group h = l >> 5 (selector 0x06040200 or 0x07050301
//            over {high dword, low dword}); sub-step kk's MFMA selects byte kk
//            (op_sel) for both A and B, so a step uses every op_sel value on
//            both operands.
//
// Record (32 words a workgroup): magic, workgroup, nonce ^ wg, XCC id with
// ksteps in bits 8.., HW_ID of the four waves, and per wave six fold words: an
// xor and a sum modulo 2^32 over the dwords of the A fragments, of the B
// fragments, and of the gathered scale VGPRs (A's two and B's two, once a step)
// the wave fed to its MFMAs. The host knows what a wave reads (all K of rows
// 64*(v>>1).. of A and of sa, of columns 64*(v&1).. of B and of sb) and
// compares: stage 0 = A feed, 1 = B feed, 2 = scale feed, 3 = D words.
#pragma once

#include <stdint.h>

#include "datapath_bf16_kernel.h"

#define MI355X_DPMX_THREADS 256
#define MI355X_DPMX_TILE 128                       // rows = columns of a workgroup's tile
#define MI355X_DPMX_KSTEP 256                      // k of one step of the loop: 128 bytes a row
#define MI355X_DPMX_KSTEPS 8                       // production: K = 2048
#define MI355X_DPMX_KSTEPS_MAX 8                   // the bound above
#define MI355X_DPMX_WG_WORDS (MI355X_DPMX_TILE * MI355X_DPMX_TILE)
#define MI355X_DPMX_REC_WORDS 32
#define MI355X_DPMX_MAGIC 0x44504D58u /* "DPMX" */
#define MI355X_DPMX_STAGES 4                       // 0 = A feed, 1 = B feed, 2 = scale feed, 3 = D words
// record words (one record per workgroup)
#define MI355X_DPMXREC_MAGIC 0
#define MI355X_DPMXREC_WG 1
#define MI355X_DPMXREC_NONCE 2   // nonce ^ wg
#define MI355X_DPMXREC_XCC 3     // XCC id in bits 0..3, ksteps in bits 8..
#define MI355X_DPMXREC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPMXREC_FOLD 8    // 24 words: wave * 6 + feed stage * 2 + {xor, sum}
// LDS: two buffers, each the A tile, then the B tile
#define MI355X_DPMX_LDS_TILE_BYTES 16384
#define MI355X_DPMX_LDS_BYTES (4 * MI355X_DPMX_LDS_TILE_BYTES)

// explicit kernel arguments of both kernels (64 bytes; they use no hidden args)
struct mi355x_datapath_mxgemm_args {
  uint32_t* records;  // host-visible, grid * MI355X_DPMX_REC_WORDS
  uint32_t* tiles;    // host-visible, grid * MI355X_DPMX_WG_WORDS: D, word = row * 128 + column
  uint8_t* a;         // device, grid * 128 * K/2 bytes: A_wg at wg * 64 * K, row-major
  uint8_t* b;         // device, 128 * K/2 bytes, [column][k]
  uint8_t* sa;        // device, grid * 128 * K/32 bytes: sa_wg at wg * 4 * K, [row][block]
  uint8_t* sb;        // device, 128 * K/32 bytes, [column][block]
  uint32_t nonce;
  uint32_t grid;      // workgroups; a workgroup beyond it reads and writes nothing
  uint32_t ksteps;    // K / 256
  uint32_t pad;
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it).
  // Runtime arguments, the siblings' six fields:
  //   MFMA   after the loop, accumulator word `index` (32x32 block * 16 + register)
  //          of lane `lane` of wave `wave` of workgroup `wg` is xor-ed with `mask`
  //   LDS    after the loads of step `wave` (the field carries the step) have landed
  //          and before they are read, dword `index` (0..8191: the A tile, then
  //          the B tile) of that step's LDS buffer of workgroup `wg` is xor-ed
  //          with `mask`
  //   HBM    mi355x_mxgemm_fill xors the low 8 bits of `mask` into byte `index`
  //          (row * K/2 + k/2) of A of workgroup `wg`
  //   SCALE  before sub-step (index >> 2) & 3 of step index >> 4, gathered scale
  //          VGPR index & 3 (A's row blocks 0 and 1, then B's column blocks) of
  //          lane `lane` of wave `wave` of workgroup `wg` is xor-ed with `mask`;
  //          it stays so to the end of the step, where the VGPRs are folded
  uint32_t inject_kind;   // MI355X_DPMX_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;
  uint32_t inject_lane;
  uint32_t inject_index;
  uint32_t inject_mask;
#endif
};

#define MI355X_DPMX_INJECT_NONE 0
#define MI355X_DPMX_INJECT_MFMA 1
#define MI355X_DPMX_INJECT_LDS 2
#define MI355X_DPMX_INJECT_HBM 3
#define MI355X_DPMX_INJECT_SCALE 4

#if defined(__HIPCC__)
#define MI355X_DPMX_HD __host__ __device__ inline
#else
#define MI355X_DPMX_HD static inline
#endif

// index spaces of dpmx_hash (the `stage` of dpbf_hash), after the attention check's
#define MI355X_DPMX_SPACE_A 0x60u   // idx = row * (K/8) + k/8, seed = the workgroup's: a dword of eight codes
#define MI355X_DPMX_SPACE_B 0x61u   // idx = col * (K/8) + k/8, seed = the nonce
#define MI355X_DPMX_SPACE_C 0x62u   // idx = row * 128 + col, seed = the workgroup's
#define MI355X_DPMX_SPACE_SA 0x63u  // idx = row: SA_i
#define MI355X_DPMX_SPACE_SB 0x64u  // idx = col: SB_j
#define MI355X_DPMX_SPACE_DA 0x65u  // idx = row * 64 + block: d
#define MI355X_DPMX_SPACE_DB 0x66u  // idx = col * 64 + block: d'
#define MI355X_DPMX_SPACE_X 0x67u   // idx = col: the verdict's second projection vector

#define MI355X_DPMX_SBASE_LO 112u   // SA_i, SB_j: 112..142
#define MI355X_DPMX_SBASE_N 31u

MI355X_DPMX_HD bool dpmx_sizes_ok(uint32_t grid, uint32_t ksteps) {
  return grid != 0u && grid <= 1024u && ksteps != 0u && ksteps <= MI355X_DPMX_KSTEPS_MAX;
}

MI355X_DPMX_HD uint32_t dpmx_wg_seed(uint32_t nonce, uint32_t wg) { return dpbf_wave_nonce(nonce, wg, 0u); }

// eight free codes: the hash word, a nibble without a magnitude bit gets magnitude 1
MI355X_DPMX_HD uint32_t dpmx_codes(uint32_t h) {
  const uint32_t m = h & 0x77777777u;
  return h | (~(m | (m >> 1) | (m >> 2)) & 0x11111111u);
}

// dword kd (elements 8 kd .. 8 kd + 7) of row `row` of A_wg, of column `col` of B
MI355X_DPMX_HD uint32_t dpmx_a_dword(uint32_t seed, uint32_t ksteps, uint32_t row, uint32_t kd) {
  return dpmx_codes(dpbf_hash(seed, MI355X_DPMX_SPACE_A, row * (ksteps * 32u) + kd));
}
MI355X_DPMX_HD uint32_t dpmx_b_dword(uint32_t nonce, uint32_t ksteps, uint32_t col, uint32_t kd) {
  return dpmx_codes(dpbf_hash(nonce, MI355X_DPMX_SPACE_B, col * (ksteps * 32u) + kd));
}

// SA_i (which = 0, seed = the workgroup's) or SB_j (which = 1, seed = the nonce)
MI355X_DPMX_HD uint32_t dpmx_scale_base(uint32_t seed, uint32_t which, uint32_t rc) {
  return MI355X_DPMX_SBASE_LO + dpbf_hash(seed, which ? MI355X_DPMX_SPACE_SB : MI355X_DPMX_SPACE_SA, rc) % MI355X_DPMX_SBASE_N;
}
// d of (row, scale block) or d' of (column, scale block)
MI355X_DPMX_HD uint32_t dpmx_delta(uint32_t seed, uint32_t which, uint32_t rc, uint32_t block) {
  return (dpbf_hash(seed, which ? MI355X_DPMX_SPACE_DB : MI355X_DPMX_SPACE_DA, rc * 64u + block) >> 13) & (which ? 1u : 3u);
}
MI355X_DPMX_HD uint32_t dpmx_scale_byte(uint32_t seed, uint32_t which, uint32_t rc, uint32_t block) {
  return dpmx_scale_base(seed, which, rc) + dpmx_delta(seed, which, rc, block);
}

MI355X_DPMX_HD int32_t dpmx_ga(uint32_t seed, uint32_t row, uint32_t col) {
  const uint32_t h = dpbf_hash(seed, MI355X_DPMX_SPACE_C, row * 128u + col);
  const int32_t mag = static_cast<int32_t>((h & 0xFFFFFu) | 1u);  // odd, < 2^20
  return (h >> 31) ? -mag : mag;
}

// log2 of the quantum q of output (row, col)
MI355X_DPMX_HD int32_t dpmx_qx(uint32_t seed, uint32_t nonce, uint32_t row, uint32_t col) {
  return static_cast<int32_t>(dpmx_scale_base(seed, 0u, row) + dpmx_scale_base(nonce, 1u, col)) - 257;
}

MI355X_DPMX_HD uint32_t dpmx_c_word(uint32_t seed, uint32_t nonce, uint32_t row, uint32_t col) {
  return dpbf_scaled_int(dpmx_ga(seed, row, col), dpmx_qx(seed, nonce, row, col));
}

// LDS byte offset within a tile of the 16-byte chunk (row / column, k-chunk 0..7)
MI355X_DPMX_HD uint32_t dpmx_lds(uint32_t row, uint32_t kc) { return row * 128u + ((kc ^ ((row >> 1) & 7u)) << 4); }

// the scale VGPR lane group h feeds to a step's MFMAs: bytes h, 2+h, 4+h, 6+h of the step's eight (lo: 0..3, hi: 4..7)
MI355X_DPMX_HD uint32_t dpmx_gather(uint32_t lo, uint32_t hi, uint32_t h) {
  const uint32_t s = 8u * h;
  return ((lo >> s) & 0xFFu) | (((lo >> (16u + s)) & 0xFFu) << 8) | (((hi >> s) & 0xFFu) << 16) |
         (((hi >> (16u + s)) & 0xFFu) << 24);
}

// where word `word` (wave * 2 + {0 xor, 1 sum}) of feed stage `stage` (0 = A, 1 = B, 2 = scales) sits in a record
MI355X_DPMX_HD uint32_t dpmx_fold_slot(uint32_t stage, uint32_t word) {
  return MI355X_DPMXREC_FOLD + (word >> 1) * 6u + stage * 2u + (word & 1u);
}
