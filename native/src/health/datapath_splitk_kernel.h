// Shared between the gfx950 split-K GEMM kernels (mi355x_splitk_fill,
// mi355x_mfma_datapath_splitk, mi355x_splitk_drain), the host verdict
// (datapath_splitk_verify.h) and native/tests/datapath_splitk_contract_cli.cpp.
//
// In the nine checks before this one a workgroup writes only words that no
// other workgroup touches. A tenant's split-K or stream-K GEMM, MoE combine or
// embedding gradient ends with many workgroups, on different XCDs, adding into
// the same device-memory words with global_atomic_add_f32 and its integer kin,
// executed by the L2 / memory-side atomic units. This check is that tail, small
// and bit-exact: a unit that drops, doubles or mis-adds one update, or a
// coherence path that loses one, changes a word the host knows exactly.
//
// Problem. `tiles` output tiles of 128 x 128 f32; tile t is
//   D_t = C_t + A_t (128 x K, bf16, row-major) . B (K x 128, bf16, row-major)
// with the operands of the GEMM pipeline check (datapath_gemm_kernel.h, dpgm_*):
// panel seed dpgm_wg_seed(nonce, t), K = splits * ksteps * 64, that is
// ksteps_total = splits * ksteps <= MI355X_DPGM_KSTEPS_MAX. K is split `splits`
// ways: the grid is tiles * splits workgroups of 256 lanes, workgroup wg serves
// tile wg / splits and k in [(wg % splits) * ksteps * 64, + ksteps * 64).
// Neighbouring workgroups are dealt to different XCDs, so one tile's
// contributors normally sit on different dies; that placement is reported (XCC
// id, HW_ID), never required or arranged: no residency wait, no flag, no loop
// that waits for another workgroup.
//
// Why any arrival order is exact. Every product and C are integer multiples of
// the output's quantum q, and all their magnitudes sum to at most 8 882 175 q
// < 2^24 q at K = 2048 (the bound of datapath_gemm_kernel.h). A split's partial
// is a sub-sum of those terms and D at any moment is C plus some of the
// partials, so every addend, every intermediate D and the final D are integers
// below 2^24 in quanta: exact f32, whatever order the atomic unit sees. The
// final word is odd (an even count of odd products plus the odd C), never zero.
//
// Three dispatches on one queue, each with the barrier bit.
//   mi355x_splitk_fill  writes A and B (the bytes mi355x_gemm_fill writes for
//            grid = tiles, ksteps = splits * ksteps), D = C and a zeroed ledger
//            of 8 words a tile into device memory, 16 bytes a store.
//   mi355x_mfma_datapath_splitk  each workgroup computes its partial from a
//            zero accumulator and adds it into D_t; see below.
//   mi355x_splitk_drain  one workgroup a tile copies D_t (64 KiB) and the ledger
//            to the host-visible buffers with 16-byte loads and stores.
//
// Kernel design (datapath_splitk_kernel.hip).
//   waves    4, as 2 x 2: wave v owns rows 64*(v>>1).., columns 64*(v&1).. as
//            sixteen 16x16 accumulators of v_mfma_f32_16x16x32_bf16 (64
//            registers), each a dependent chain of 2 * ksteps MFMAs.
//   LDS      two buffers (two variables, as in the GEMM check) of 32 KiB: a
//            128 x 64 tile of A (128 B a row) and a 64 x 128 tile of B (256 B a
//            row) per k-step, filled by global_load_lds_dwordx4; the loads of
//            step s+1 are issued before the MFMAs of step s; one barrier a step.
//   A reads  ds_read_b128: lane l reads row l&15 of its 16-row block, k-chunk
//            4*kk + (l>>4) of the step's two 32-wide sub-steps kk.
//   B reads  ds_read_b64_tr_b16, two a fragment, with the lane map measured for
//            the GEMM check: in a block of 16 lanes source lane t points at row
//            (k) t>>2, column group t&3, and result lane L holds column L,
//            k = 0..3. The 16 lanes l>>4 = g are exactly k-group g (k 8g..8g+7)
//            of this shape: read h covers k 8g + 4h .. + 3.
//   swizzle  on the global-address side, in 16-byte chunks, worked out again for
//            these patterns by bank arithmetic (64 banks of 4 bytes = 16 chunk
//            slots of 256 bytes; the conflict counters were not read).
//            A: 16 lanes of a ds_read_b128 read rows r0..r0+15 at one k-chunk c.
//            A row is 8 chunks, so row r starts at slot 8*(r&1): the 8 rows of
//            one parity must land on 8 different positions. Position
//            p = c ^ ((r >> 1) & 7) does that -- the GEMM check's function holds
//            for 16 rows as for 32 (dpgm_lds_a is reused).
//            B: the 32 lanes of one pass of a transposed read are two k-groups:
//            8 rows (k & 3 = 0..3, (k >> 3) & 1 = 0, 1) of 32 bytes (16
//            columns) each at one column offset. A row is a whole 256 bytes, so
//            unswizzled they collide 8 ways, and the GEMM check's function
//            (xor of (k & 3) << 2, made for 4 rows of 64 bytes) would leave 2
//            ways. Position p = c ^ (((k & 3) << 1) | (((k >> 3) & 1) << 3))
//            moves the 8 rows onto the 8 different 32-byte pairs of slots.
//   tail     every accumulator word is added to its D word with a relaxed,
//            agent-scope, no-return f32 atomic add (global_atomic_add_f32); six
//            lanes update the tile's ledger with integer atomics. Cache-policy
//            bits are the compiler's for agent scope. Vector stores and vector
//            atomics only.
//
// Ledger (8 words a tile, device memory, zeroed by the fill):
//   0  += 1                          arrivals: `splits` when all came
//   1  ^= nonce ^ wg                 which workgroups came
//   2  += sum, 3 ^= xor              of the 16-bit elements of the workgroup's
//                                    128 x (ksteps*64) part of A_t, as it read
//                                    them out of LDS (waves 0 and 2)
//   4  += sum, 5 ^= xor              likewise of its (ksteps*64) x 128 part of B
//                                    (waves 0 and 1)
//   6, 7 stay zero
// Over a tile's contributors words 2..5 are the folds of the whole A_t and B.
//
// Record (32 words a workgroup, straight to host memory): magic, workgroup,
// nonce ^ wg, XCC id, HW_ID of the four waves, tiles, splits, ksteps, and per
// wave the fold (xor, and sum modulo 2^32, over 16-bit elements) of the A and
// of the B fragments it read. Stages: 0 = A feed, 1 = B feed, 2 = D words
// (word = tile * 16384 + row * 128 + column), 3 = ledger (word = tile * 8 +
// ledger word); for the feeds word = wg * 8 + wave * 2 + {0 xor, 1 sum}.
#pragma once

#include <stdint.h>

#include "datapath_gemm_kernel.h"

#define MI355X_DPSK_THREADS 256
#define MI355X_DPSK_SPLITS 8                       // production: eight contributors a word
#define MI355X_DPSK_KSTEPS 4                       // production: K = 8 * 4 * 64 = 2048
#define MI355X_DPSK_CUS_PER_TILE 8                 // production: tiles = cu_count / 8
#define MI355X_DPSK_TILE_WORDS (MI355X_DPGM_TILE * MI355X_DPGM_TILE)
#define MI355X_DPSK_LEDGER_WORDS 8
#define MI355X_DPSK_REC_WORDS 32
#define MI355X_DPSK_MAGIC 0x4450534Bu /* "DPSK" */
#define MI355X_DPSK_STAGES 4                       // 0 = A feed, 1 = B feed, 2 = D words, 3 = ledger
// record words (one record per workgroup); 11..15 are written as zero
#define MI355X_DPSKREC_MAGIC 0
#define MI355X_DPSKREC_WG 1
#define MI355X_DPSKREC_NONCE 2   // nonce ^ wg
#define MI355X_DPSKREC_XCC 3
#define MI355X_DPSKREC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPSKREC_TILES 8
#define MI355X_DPSKREC_SPLITS 9
#define MI355X_DPSKREC_KSTEPS 10
#define MI355X_DPSKREC_FOLD 16   // 16 words: wave * 4 + {A xor, A sum, B xor, B sum}
// ledger words
#define MI355X_DPSKLED_ARRIVALS 0
#define MI355X_DPSKLED_WHO 1
#define MI355X_DPSKLED_A_SUM 2
#define MI355X_DPSKLED_A_XOR 3
#define MI355X_DPSKLED_B_SUM 4
#define MI355X_DPSKLED_B_XOR 5

// explicit kernel arguments of the three kernels (72 bytes; they use no hidden args)
struct mi355x_datapath_splitk_args {
  uint32_t* records;     // host-visible, tiles * splits * MI355X_DPSK_REC_WORDS
  uint32_t* out_d;       // host-visible, tiles * MI355X_DPSK_TILE_WORDS: the drain's copy of D
  uint32_t* out_ledger;  // host-visible, tiles * MI355X_DPSK_LEDGER_WORDS: the drain's copy of the ledger
  uint16_t* a;           // device, tiles * 128 * K bf16: A_t at t * 128 * K, row-major
  uint16_t* b;           // device, K * 128 bf16, row-major
  float* d;              // device, tiles * 128 * 128: word = row * 128 + column of tile t at t * 16384
  uint32_t* ledger;      // device, tiles * MI355X_DPSK_LEDGER_WORDS
  uint32_t nonce;
  uint32_t tiles;
  uint32_t splits;
  uint32_t ksteps;       // k-steps of 64 a workgroup; splits * ksteps in 1..MI355X_DPGM_KSTEPS_MAX
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it).
  // Runtime arguments, the siblings' six fields: the atomic add of accumulator
  // word `index` ((row block * 4 + column block) * 4 + register, 0..63) of lane
  // `lane` of wave `wave` of workgroup `wg`
  //   ATOMIC  has its operand xor-ed with `mask`
  //   DROP    is skipped
  uint32_t inject_kind;   // MI355X_DPSK_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;
  uint32_t inject_lane;
  uint32_t inject_index;
  uint32_t inject_mask;
#endif
};

#define MI355X_DPSK_INJECT_NONE 0
#define MI355X_DPSK_INJECT_ATOMIC 1
#define MI355X_DPSK_INJECT_DROP 2

// what the kernels refuse: nothing is read or written
MI355X_DPGM_HD bool dpsk_sizes_ok(uint32_t tiles, uint32_t splits, uint32_t ksteps) {
  return tiles != 0u && splits != 0u && ksteps != 0u && splits <= MI355X_DPGM_KSTEPS_MAX &&
         ksteps <= MI355X_DPGM_KSTEPS_MAX && splits * ksteps <= MI355X_DPGM_KSTEPS_MAX;
}

// LDS byte offset within the B tile of the 16-byte chunk (k of the step, column chunk 0..15); A uses dpgm_lds_a
MI355X_DPGM_HD uint32_t dpsk_b_swz(uint32_t k) { return ((k & 3u) << 1) | (((k >> 3) & 1u) << 3); }
MI355X_DPGM_HD uint32_t dpsk_lds_b(uint32_t k, uint32_t nc) { return k * 256u + ((nc ^ dpsk_b_swz(k)) << 4); }

// row and column within the wave's 64 x 64 of accumulator word `index` of lane `lane`
MI355X_DPGM_HD uint32_t dpsk_acc_row(uint32_t index, uint32_t lane) { return 16u * (index >> 4) + 4u * (lane >> 4) + (index & 3u); }
MI355X_DPGM_HD uint32_t dpsk_acc_col(uint32_t index, uint32_t lane) { return 16u * ((index >> 2) & 3u) + (lane & 15u); }

// where word `word` (wave * 2 + {0 xor, 1 sum}) of feed stage `stage` (0 = A, 1 = B) sits in a record
MI355X_DPGM_HD uint32_t dpsk_fold_slot(uint32_t stage, uint32_t word) {
  return MI355X_DPSKREC_FOLD + (word >> 1) * 4u + stage * 2u + (word & 1u);
}
