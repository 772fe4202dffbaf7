// Shared between the gfx950 bf16 GEMM pipeline kernels (mi355x_gemm_fill,
// mi355x_mfma_datapath_gemm), the host verdict (datapath_gemm_verify.h) and
// native/tests/datapath_gemm_contract_cli.cpp.
//
// The eight MFMA datapath checks build operands in registers and issue one MFMA
// per stage. A tenant's GEMM moves its operands out of HBM through L2 into LDS
// by the direct-to-LDS loads, out of LDS by 128-bit and by transposed reads,
// and into a K loop in which every MFMA takes the previous one's accumulator as
// its C while the next tile's loads are in flight. This check is that pipeline,
// small and bit-exact.
//
// Problem. `grid` workgroups of 256 lanes; workgroup wg computes the 128 x 128
// f32 tile
//   D_wg = C_wg + A_wg (128 x K, bf16, row-major) . B (K x 128, bf16, row-major)
// A_wg is the workgroup's own panel (it streams from HBM), B is one panel all
// workgroups read (through L2, from every XCD), K = ksteps * 64 with
// 1 <= ksteps <= MI355X_DPGM_KSTEPS_MAX. mi355x_gemm_fill writes both operands
// into device memory from the hash, with 16-byte vector stores, in a dispatch of
// its own on the same queue; D goes to host memory, whole.
//
// Operands (the bf16 check's stage-2 recipe, stretched to a long K). Row i of
// A_wg has an exponent field Ea_i, column j of B has Eb_j, both in 101..158.
//   full element    +-(128+m) * 2^(E-134), m odd in 1..127
//   narrow element  +-(8+m')  * 2^(E-134), m' odd in 1..7: a bf16 with exponent
//                   field E-4 whose four low mantissa bits are zero
// In the even 32-wide k-blocks A is full and B narrow, in the odd ones A is
// narrow and B full. C[i][j] = ga * q, ga odd, |ga| < 2^20, q = 2^(Ea_i+Eb_j-268).
//
// Why every word is exact in any order. Every product is an odd integer of at
// most 255 * 15 = 3825 times q. The magnitudes of all K products and of C sum
// to at most
//   K = 1024 (ksteps 16):  3 916 800 + 1 048 575 = 4 965 375
//   K = 2048 (ksteps 32):  7 833 600 + 1 048 575 = 8 882 175
// quanta, below 2^24 = 16 777 216. So every partial sum, in every order, tree
// shape and chain split, is an integer multiple of q below 2^24 q and fits an
// f32 significand; between two MFMAs of a chain it sits in an f32 register and
// is exact. K is even, so an even count of odd products plus the odd ga is odd:
// no output word is zero. q lies in 2^-66..2^48.
//
// Kernel design (datapath_gemm_kernel.hip).
//   waves    4, as 2 x 2: wave v owns rows 64*(v>>1).., columns 64*(v&1).. of the
//            tile, four 32x32 accumulators of v_mfma_f32_32x32x16_bf16, each a
//            dependent chain of 4 * ksteps MFMAs.
//   LDS      two buffers of 32 KiB: a 128 x 64 tile of A (16 KiB, 128 B a row)
//            and a 64 x 128 tile of B (16 KiB, 256 B a row) per k-step.
//   loads    global_load_lds_dwordx4: 16 bytes a lane, a wave's 64 lanes land
//            in 1 KiB of consecutive LDS, 8 wave-loads a wave a step. The loads
//            of step s+1 are issued before the MFMAs of step s; one barrier a
//            step.
//   swizzle  made on the global-address side, in units of 16-byte chunks. The
//            chunk at LDS position p of row r of the A tile holds k-chunk
//            p ^ ((r >> 1) & 7): the 16 rows a ds_read_b128 quarter-wave reads
//            at one k-chunk fall on 16 different 16-byte bank groups. The chunk
//            at LDS position p of row k of the B tile holds column chunk
//            p ^ ((k & 3) << 2): the four rows of 64 bytes that 32 lanes of a
//            transposed read touch tile 256 bytes of banks. (Designed from the
//            bank arithmetic; the conflict counters were not read.)
//   A reads  ds_read_b128: lane l reads the 8 consecutive k of row l&31 of its
//            32-row block, k-chunk 2*kk + (l>>5) of the step's four 16-wide
//            sub-steps kk.
//   B reads  ds_read_b64_tr_b16, two a fragment. Lane map, measured on an MI355X
//            (docs/health.md): within each block of 16 lanes, lane t supplies the
//            address of four consecutive 16-bit elements, and lane L receives, as
//            element e, element L&3 of the four that lane 4*e + (L>>2) addressed.
//            So source lane t points at row (k) t>>2, column group t&3, and
//            result lane L holds column L, k = 0..3.
//
// Record (32 words a workgroup): magic, workgroup, nonce ^ wg, XCC id, HW_ID of
// the four waves, ksteps, and per wave an order-independent fold -- xor, and
// sum modulo 2^32, over the 16-bit elements -- of the A fragments and of the B
// fragments the wave read out of LDS. The host knows which rows and columns a
// wave reads (all K of rows 64*(v>>1).. of A, of columns 64*(v&1).. of B) and
// compares: stage 0 = A feed, stage 1 = B feed, stage 2 = D words.
#pragma once

#include <stdint.h>

#include "datapath_bf16_kernel.h"

#define MI355X_DPGM_THREADS 256
#define MI355X_DPGM_TILE 128                       // rows = columns of a workgroup's tile
#define MI355X_DPGM_KSTEP 64                       // k of one step of the loop
#define MI355X_DPGM_KSTEPS 16                      // production: K = 1024
#define MI355X_DPGM_KSTEPS_MAX 32                  // K = 2048: the bound above still holds
#define MI355X_DPGM_WG_WORDS (MI355X_DPGM_TILE * MI355X_DPGM_TILE)
#define MI355X_DPGM_REC_WORDS 32
#define MI355X_DPGM_MAGIC 0x4450474Du /* "DPGM" */
#define MI355X_DPGM_STAGES 3                       // 0 = A feed, 1 = B feed, 2 = D words
// record words (one record per workgroup); 9..15 are written as zero
#define MI355X_DPGMREC_MAGIC 0
#define MI355X_DPGMREC_WG 1
#define MI355X_DPGMREC_NONCE 2   // nonce ^ wg
#define MI355X_DPGMREC_XCC 3
#define MI355X_DPGMREC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPGMREC_KSTEPS 8
#define MI355X_DPGMREC_FOLD 16   // 16 words: wave * 4 + {A xor, A sum, B xor, B sum}
// LDS: two buffers, each the A tile, then the B tile
#define MI355X_DPGM_LDS_TILE_BYTES 16384
#define MI355X_DPGM_LDS_BYTES (4 * MI355X_DPGM_LDS_TILE_BYTES)

// explicit kernel arguments of both kernels (40 bytes; they use no hidden args)
struct mi355x_datapath_gemm_args {
  uint32_t* records;  // host-visible, grid * MI355X_DPGM_REC_WORDS
  uint32_t* tiles;    // host-visible, grid * MI355X_DPGM_WG_WORDS: D, word = row * 128 + column
  uint16_t* a;        // device, grid * 128 * K bf16: A_wg at wg * 128 * K, row-major
  uint16_t* b;        // device, K * 128 bf16, row-major
  uint32_t nonce;
  uint32_t grid;      // workgroups; a workgroup beyond it reads and writes nothing
  uint32_t ksteps;    // K / 64
  uint32_t pad;
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it).
  // Runtime arguments, the siblings' six fields:
  //   MFMA  after the loop, accumulator word `index` (32x32 block * 16 + register)
  //         of lane `lane` of wave `wave` of workgroup `wg` is xor-ed with `mask`
  //   LDS   after the loads of step `wave` (the field carries the step) have landed
  //         and before they are read, dword `index` (0..8191: the A tile, then
  //         the B tile) of that step's LDS buffer of workgroup `wg` is xor-ed
  //         with `mask`
  //   HBM   mi355x_gemm_fill xors the low 16 bits of `mask` into element `index`
  //         (row * K + k) of A of workgroup `wg`
  uint32_t inject_kind;   // MI355X_DPGM_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;
  uint32_t inject_lane;
  uint32_t inject_index;
  uint32_t inject_mask;
#endif
};

#define MI355X_DPGM_INJECT_NONE 0
#define MI355X_DPGM_INJECT_MFMA 1
#define MI355X_DPGM_INJECT_LDS 2
#define MI355X_DPGM_INJECT_HBM 3

#if defined(__HIPCC__)
#define MI355X_DPGM_HD __host__ __device__ inline
#else
#define MI355X_DPGM_HD static inline
#endif

// index spaces of dpgm_hash (the `stage` of dpbf_hash)
#define MI355X_DPGM_SPACE_A 0x40u   // idx = row * (K/2) + k/2, seed = the workgroup's
#define MI355X_DPGM_SPACE_B 0x41u   // idx = k * 64 + col/2, seed = the nonce
#define MI355X_DPGM_SPACE_C 0x42u   // idx = row * 128 + col, seed = the workgroup's
#define MI355X_DPGM_SPACE_EA 0x43u  // idx = row
#define MI355X_DPGM_SPACE_EB 0x44u  // idx = col
#define MI355X_DPGM_SPACE_X 0x45u   // idx = col: the verdict's second projection vector

#define MI355X_DPGM_E_LO 101u       // exponent fields 101..158: a narrow element's field stays >= 97
#define MI355X_DPGM_E_N 58u

MI355X_DPGM_HD uint32_t dpgm_wg_seed(uint32_t nonce, uint32_t wg) { return dpbf_wave_nonce(nonce, wg, 0u); }

MI355X_DPGM_HD uint32_t dpgm_exp_field(uint32_t seed, uint32_t space, uint32_t rc) {
  return MI355X_DPGM_E_LO + dpbf_hash(seed, space, rc) % MI355X_DPGM_E_N;
}

// two elements of one operand dword: full (7 mantissa bits, the lowest set) or
// narrow (exponent field e - 4, mantissa m' << 4 with m' odd)
MI355X_DPGM_HD uint32_t dpgm_pair(uint32_t h, uint32_t e, bool full) {
  if (full) return (h & 0x807F807Fu) | 0x00010001u | (e << 7) | (e << 23);
  return (h & 0x80708070u) | 0x00100010u | ((e - 4u) << 7) | ((e - 4u) << 23);
}

// the dword holding elements (row, k) and (row, k + 1) of A_wg, k even
MI355X_DPGM_HD uint32_t dpgm_a_dword(uint32_t seed, uint32_t ksteps, uint32_t row, uint32_t k) {
  const uint32_t h = dpbf_hash(seed, MI355X_DPGM_SPACE_A, row * (ksteps * 32u) + (k >> 1));
  return dpgm_pair(h, dpgm_exp_field(seed, MI355X_DPGM_SPACE_EA, row), ((k >> 5) & 1u) == 0u);
}

// element (k, col) of B: the halves of one hash word serve columns col and col ^ 1
MI355X_DPGM_HD uint32_t dpgm_b_elem(uint32_t nonce, uint32_t k, uint32_t col) {
  const uint32_t h = dpbf_hash(nonce, MI355X_DPGM_SPACE_B, k * 64u + (col >> 1));
  const uint32_t w = dpgm_pair(h, dpgm_exp_field(nonce, MI355X_DPGM_SPACE_EB, col), ((k >> 5) & 1u) == 1u);
  return (col & 1u) ? (w >> 16) : (w & 0xFFFFu);
}

MI355X_DPGM_HD int32_t dpgm_ga(uint32_t seed, uint32_t row, uint32_t col) {
  const uint32_t h = dpbf_hash(seed, MI355X_DPGM_SPACE_C, row * 128u + col);
  const int32_t mag = static_cast<int32_t>((h & 0xFFFFFu) | 1u);  // odd, < 2^20
  return (h >> 31) ? -mag : mag;
}

// log2 of the quantum of output (row, col)
MI355X_DPGM_HD int32_t dpgm_qx(uint32_t seed, uint32_t nonce, uint32_t row, uint32_t col) {
  return static_cast<int32_t>(dpgm_exp_field(seed, MI355X_DPGM_SPACE_EA, row) +
                              dpgm_exp_field(nonce, MI355X_DPGM_SPACE_EB, col)) - 268;
}

MI355X_DPGM_HD uint32_t dpgm_c_word(uint32_t seed, uint32_t nonce, uint32_t row, uint32_t col) {
  return dpbf_scaled_int(dpgm_ga(seed, row, col), dpgm_qx(seed, nonce, row, col));
}

// a bf16 element of the recipe in quanta of 2^(E-134), E its row's / column's field: +-(128+m) or +-(8+m')
MI355X_DPGM_HD int32_t dpgm_units(uint32_t elem, uint32_t e) {
  const int32_t mag = static_cast<int32_t>(128u + (elem & 0x7Fu)) >> (e - ((elem >> 7) & 0xFFu));
  return (elem & 0x8000u) ? -mag : mag;
}

// LDS byte offsets within a tile of the 16-byte chunk (A: row, k-chunk 0..7; B: k, column chunk 0..15)
MI355X_DPGM_HD uint32_t dpgm_lds_a(uint32_t row, uint32_t kc) { return row * 128u + ((kc ^ ((row >> 1) & 7u)) << 4); }
MI355X_DPGM_HD uint32_t dpgm_lds_b(uint32_t k, uint32_t nc) { return k * 256u + ((nc ^ ((k & 3u) << 2)) << 4); }

// where word `word` of feed stage `stage` (0 = A, 1 = B) sits in a record: word = wave * 2 + {0 xor, 1 sum}
MI355X_DPGM_HD uint32_t dpgm_fold_slot(uint32_t stage, uint32_t word) {
  return MI355X_DPGMREC_FOLD + (word >> 1) * 4u + stage * 2u + (word & 1u);
}
