// Shared between the gfx950 fused attention kernels (mi355x_attn_fill,
// mi355x_mfma_datapath_attn), the host verdict (datapath_attn_verify.h) and
// native/tests/datapath_attn_contract_cli.cpp.
//
// The ten checks before this one cover what a tenant's GEMM does. A
// flash-attention kernel does four more things: it takes an MFMA accumulator as
// the next MFMA's operand (packed to bf16 by v_cvt_pk_bf16_f32 and moved across
// the two halves of the wave by v_permlane32_swap, both new on gfx950), it
// reduces across lanes inside the loop, it uses the transcendental unit
// (v_exp_f32) between two matrix instructions, and it rescales live accumulators
// between MFMAs (online softmax). This check is that loop, small and bit-exact.
//
// Problem. `heads` heads, each with N = kblocks * 64 keys and values and
// qblocks * 128 queries of head dimension d = 64, all bf16, row-major, in device
// memory: Q [head][query][64], K and V [head][key][64]. The grid is
// heads * qblocks workgroups of 256 lanes; workgroup wg serves head wg / qblocks
// and queries 128 * (wg % qblocks) onwards; the qblocks workgroups of a head read
// the same K and V through L2. For every query i the kernel writes the base-2
// softmax state before normalisation, what a split-KV kernel hands to its combine
// step:
//   S_ij = sum_d Q_id K_jd      m_i = max_j S_ij
//   l_i  = sum_j 2^(S_ij - m_i)
//   O_id = sum_j 2^(S_ij - m_i) V_jd
// No division, no mask, no scale. o (f32 [wg][128][64]), ml (f32 [wg][128][2]:
// m, l) and the records go straight to host-visible memory.
//
// Operands, and why every word is exact in any order.
//   Q, K   d is 32 pairs (2p, 2p+1). A hash bit per pair, seeded by the nonce and
//          shared by Q and K, picks the pair's shape: shape 0 has the Q pair
//          (a, a) and the K pair (x, -x); shape 1 has (a, 2a) and (2x, -x), with
//          a = +-{1,2} hashed per (query, pair) and x = +-{2..6} per (key, pair).
//          Every pair's contribution cancels to 0 exactly. Each key has three
//          distinct live pairs; there the first K element is increased by
//          t = +-1, which contributes a * t.
//   S      all elements are non-zero integers of magnitude <= 13, exact in bf16;
//          every product and partial sum inside the S MFMAs is a small integer,
//          and S_ij, the sum of three a * t, is an integer in -6..6 (dpat_score
//          gives it in O(1)). So S_ij - m is in -12..0 for the running max at any
//          time.
//   V      V_jd = +-{1,2,3} * 2^(Ev_d - 127), Ev_d a per-column exponent field in
//          101..158.
//   P      2^n with n in -12..0 is an exact bf16.
//   bound  relative to the running max every term of l is a multiple of 2^-12 and
//          every term of O_.d a multiple of q_d = 2^(Ev_d - 139). A rescale by
//          2^(m_old - m_new) keeps both multiples of the same quantum, because
//          the range bound is over the whole row: min_j S_ij - m_new >= -12
//          always. At N = 512 the magnitudes of l sum below 2^9 * 2^12 = 2^21
//          quanta and those of O below 3 * 2^9 * 2^12 < 2^23 quanta, both below
//          2^24: every partial sum is exact in f32 for any MFMA tree shape, block
//          order, chain split and lane-combine order.
//
// Two rules for the kernel that the exactness depends on.
//   1. P comes from v_exp_f32 on the exact integer S - m. The ISA documents it to
//      1 ulp, not as exact, and the check does not depend on it: P is rounded to
//      bf16 by v_cvt_pk_bf16_f32, and round-to-nearest-even of 2^n +- 1 ulp(f32)
//      is 2^n. l is summed from the bf16-rounded P widened back to f32, never
//      from the f32 exponentials. The f32 results that were not exact powers of
//      two are counted into the record word exp_inexact: reported, never judged.
//   2. The rescale of O and l is an exact power-of-two operation: v_ldexp_f32 by
//      the integer m_old - m_new, never a multiply by a v_exp_f32 result. m
//      starts at the finite sentinel -1024.0f and O and l at 0, so the first
//      block's rescale is exact as well.
//
// Kernel design (datapath_attn_kernel.hip), transposed so that one lane owns one
// query from start to finish and nothing is ever broadcast.
//   waves    4; wave w owns queries 32w..32w+31 of the workgroup's 128. All MFMAs
//            are v_mfma_f32_32x32x16_bf16 (lane maps: datapath_gemm_kernel.h).
//   Q        loaded once from global into 16 VGPRs a lane, 16 bytes a load, as
//            the four B fragments: lane l holds query l&31, d = 16c + 8*(l>>5)..
//            Q never enters LDS.
//   K, V     blocks of 64 keys: two tiles of 64 rows x 128 B (8 KiB each) in each
//            of two LDS buffers (two variables, 32 KiB in all, an even / odd
//            written-out loop as in the GEMM kernels), filled by
//            global_load_lds_dwordx4; the loads of block s+1 are issued before
//            the MFMAs of block s; one barrier a block.
//   K reads  ds_read_b128: lane l reads row l&31 of a 32-key sub-block, d-chunk
//            2c + (l>>5). The tile has the GEMM A tile's geometry (128-byte
//            rows, 16 lanes reading 16 consecutive rows at one chunk), so its
//            swizzle p = c ^ ((r >> 1) & 7) holds: row r starts at slot 8*(r&1) of
//            the 16 chunk slots, and the 8 rows of one parity land on 8 different
//            positions (dpgm_lds_a is reused).
//   V reads  V^T fragments by ds_read_b64_tr_b16, two a fragment, with the lane
//            map measured for the GEMM check: lane l addresses key
//            16kc + 8*(l>>5) + 4h + ((l&15)>>2), d = 32dh + 16*((l>>4)&1) +
//            4*(l&3).., and receives d = 32dh + (l&31), four consecutive keys.
//   swizzle  of V, on the global-address side, by bank arithmetic (64 banks of 4
//            bytes = 256 bytes; the conflict counters were not read). 32 lanes of
//            a transposed read touch 4 consecutive rows of 64 bytes (32 d) each.
//            The GEMM B tile's rows are 256 bytes, so its four rows start on the
//            same bank and its swizzle moves each by a different 64 bytes. Here
//            a row is 128 bytes: rows k and k+1 already differ by 128 bytes, rows
//            k and k+2 by 256, that is by nothing. So chunk position
//            p = c ^ (((k >> 1) & 1) << 2) moves rows 2 and 3 of every four to the
//            other 64-byte half, and the four rows tile the 256 bytes. (That a
//            transposed read is served 32 lanes a pass is assumed, as there.)
//   S^T      = K . Q^T: per block 2 key sub-blocks x 4 d-chunks = 8 MFMAs into 32
//            accumulator registers; register r of sub-block sb of lane l is key
//            32sb + (r&3) + 8*(r>>2) + 4*(l>>5) for query l&31. A lane holds 16
//            of a sub-block's 32 keys for its query, lane l^32 the other 16.
//   max      in-lane v_max3_f32 over the 32 registers, one exchange with lane
//            l^32 by v_permlane32_swap, a final max.
//   exp      k = int(m_old - m_new); O and l rescaled by rule 2;
//            P = v_exp_f32(S - m_new), packed in pairs by v_cvt_pk_bf16_f32; l is
//            a per-lane partial, the two half-waves are added once after the loop.
//   P^T      as B of the second MFMA: for each 16 keys the fragment of a lane
//            < 32 is keys 0..7 (it owns 0..3 and needs 4..7 from lane + 32), of a
//            lane >= 32 keys 8..15 (it owns 12..15 and needs 8..11 from lane -
//            32). With X the packed registers 0..3 and Y the packed registers
//            4..7, one v_permlane32_swap of (X, Y) per dword does exactly that:
//            8 swaps a block a wave. (The swap exchanges lanes 32..63 of its
//            first operand with lanes 0..31 of its second; docs/health.md.)
//   O^T      = V^T . P^T: per block 2 d-halves x 4 key-chunks = 8 MFMAs into 32
//            accumulator registers; registers 4g..4g+3 of half dh of lane l are
//            d = 32dh + 8g + 4*(l>>5).. of query l&31, so O goes out row-major
//            with 16-byte stores; m and l are written by the lanes < 32.
// No inter-workgroup synchronisation, no waiting loop, vector loads and stores
// only, no scratch.
//
// Record (32 words a workgroup): magic, workgroup, nonce ^ wg, XCC id, HW_ID of
// the four waves, heads, qblocks, kblocks, exp_inexact, and per wave the fold
// (xor, and sum modulo 2^32, over 16-bit elements) of the K and of the V
// fragments it read out of LDS: every wave reads the head's whole K and V.
// Stages: 0 = K feed, 1 = V feed (word = wg * 8 + wave * 2 + {0 xor, 1 sum}),
// 2 = m / l words (word = wg * 256 + query * 2 + {0 m, 1 l}), 3 = O words
// (word = wg * 8192 + query * 64 + d).
#pragma once

#include <stdint.h>

#include "datapath_gemm_kernel.h"

#define MI355X_DPAT_THREADS 256
#define MI355X_DPAT_D 64                           // head dimension
#define MI355X_DPAT_QBLOCK 128                     // queries of a workgroup
#define MI355X_DPAT_KBLOCK 64                      // keys of one step of the loop
#define MI355X_DPAT_QBLOCKS 4                      // production
#define MI355X_DPAT_KBLOCKS 4                      // production: N = 256
#define MI355X_DPAT_KBLOCKS_MAX 8                  // N = 512: the bound above still holds
#define MI355X_DPAT_CUS_PER_HEAD 4                 // production: heads = cu_count / 4
#define MI355X_DPAT_GRID_MAX 65536u                // heads * qblocks: word numbers stay below 2^31
#define MI355X_DPAT_ML_WORDS (MI355X_DPAT_QBLOCK * 2)
#define MI355X_DPAT_O_WORDS (MI355X_DPAT_QBLOCK * MI355X_DPAT_D)
#define MI355X_DPAT_REC_WORDS 32
#define MI355X_DPAT_MAGIC 0x44504154u /* "DPAT" */
#define MI355X_DPAT_STAGES 4                       // 0 = K feed, 1 = V feed, 2 = m / l words, 3 = O words
#define MI355X_DPAT_M_START (-1024.0f)             // the running max before the first block
// record words (one record per workgroup); 12..15 are written as zero
#define MI355X_DPATREC_MAGIC 0
#define MI355X_DPATREC_WG 1
#define MI355X_DPATREC_NONCE 2   // nonce ^ wg
#define MI355X_DPATREC_XCC 3
#define MI355X_DPATREC_HWID 4    // 4 words: HW_ID of waves 0..3
#define MI355X_DPATREC_HEADS 8
#define MI355X_DPATREC_QBLOCKS 9
#define MI355X_DPATREC_KBLOCKS 10
#define MI355X_DPATREC_EXP_INEXACT 11  // v_exp_f32 results that were not exact powers of two: reported, not judged
#define MI355X_DPATREC_FOLD 16   // 16 words: wave * 4 + {K xor, K sum, V xor, V sum}
// LDS: two buffers, each the K tile, then the V tile
#define MI355X_DPAT_LDS_TILE_BYTES 8192

// explicit kernel arguments of both kernels (64 bytes; they use no hidden args)
struct mi355x_datapath_attn_args {
  uint32_t* records;  // host-visible, heads * qblocks * MI355X_DPAT_REC_WORDS
  uint32_t* ml;       // host-visible, heads * qblocks * MI355X_DPAT_ML_WORDS: word = query * 2 + {m, l}
  uint32_t* o;        // host-visible, heads * qblocks * MI355X_DPAT_O_WORDS: word = query * 64 + d
  uint16_t* q;        // device, heads * qblocks * 128 * 64 bf16
  uint16_t* k;        // device, heads * kblocks * 64 * 64 bf16
  uint16_t* v;        // device, heads * kblocks * 64 * 64 bf16
  uint32_t nonce;
  uint32_t heads;
  uint32_t qblocks;
  uint32_t kblocks;
#if defined(MI355X_TEST_INJECT)
  // Test-only build (liveness_gfx950_inject.hsaco; no shipped binary loads it).
  // Runtime arguments, the siblings' six fields, naming lane `lane` of wave
  // `wave` of workgroup `wg`:
  //   S  xors `mask` into S accumulator word `index` (block * 32 + sub-block * 16
  //      + register) before the max
  //   O  xors `mask` into O accumulator word `index` (d-half * 16 + register)
  //      after the loop
  uint32_t inject_kind;   // MI355X_DPAT_INJECT_*
  uint32_t inject_wg;
  uint32_t inject_wave;
  uint32_t inject_lane;
  uint32_t inject_index;
  uint32_t inject_mask;
#endif
};

#define MI355X_DPAT_INJECT_NONE 0
#define MI355X_DPAT_INJECT_S 1
#define MI355X_DPAT_INJECT_O 2

// index spaces of dpbf_hash (after the GEMM check's)
#define MI355X_DPAT_SPACE_SHAPE 0x50u  // idx = pair, seed = the nonce: bit 0 is the pair's shape
#define MI355X_DPAT_SPACE_Q 0x51u      // idx = query * 32 + pair, seed = the head's
#define MI355X_DPAT_SPACE_K 0x52u      // idx = key * 32 + pair, seed = the head's
#define MI355X_DPAT_SPACE_LIVE 0x53u   // idx = key, seed = the head's: the three live pairs and their t
#define MI355X_DPAT_SPACE_V 0x54u      // idx = key * 32 + d / 2, seed = the head's
#define MI355X_DPAT_SPACE_EV 0x55u     // idx = d, seed = the head's
#define MI355X_DPAT_SPACE_X 0x56u      // idx = d, seed = the nonce: the verdict's second projection vector

// what the kernels refuse: nothing is read or written
MI355X_DPGM_HD bool dpat_sizes_ok(uint32_t heads, uint32_t qblocks, uint32_t kblocks) {
  return heads != 0u && qblocks != 0u && kblocks != 0u && kblocks <= MI355X_DPAT_KBLOCKS_MAX &&
         heads <= MI355X_DPAT_GRID_MAX && qblocks <= MI355X_DPAT_GRID_MAX && heads * qblocks <= MI355X_DPAT_GRID_MAX;
}

MI355X_DPGM_HD uint32_t dpat_head_seed(uint32_t nonce, uint32_t head) { return dpgm_wg_seed(nonce, head); }

// the bf16 of a non-zero integer of magnitude below 256
MI355X_DPGM_HD uint32_t dpat_bf16_int(int32_t n) {
  const uint32_t mag = static_cast<uint32_t>(n < 0 ? -n : n);
  const uint32_t top = 31u - static_cast<uint32_t>(__builtin_clz(mag));
  return (n < 0 ? 0x8000u : 0u) | ((127u + top) << 7) | ((mag << (7u - top)) & 0x7Fu);
}

MI355X_DPGM_HD uint32_t dpat_shape(uint32_t nonce, uint32_t pair) { return dpbf_hash(nonce, MI355X_DPAT_SPACE_SHAPE, pair) & 1u; }

// a = +-{1,2} of (query, pair)
MI355X_DPGM_HD int32_t dpat_a(uint32_t seed, uint32_t query, uint32_t pair) {
  const uint32_t h = dpbf_hash(seed, MI355X_DPAT_SPACE_Q, query * 32u + pair);
  const int32_t mag = 1 + static_cast<int32_t>(h & 1u);
  return (h >> 31) ? -mag : mag;
}

// x = +-{2..6} of (key, pair)
MI355X_DPGM_HD int32_t dpat_x(uint32_t seed, uint32_t key, uint32_t pair) {
  const uint32_t h = dpbf_hash(seed, MI355X_DPAT_SPACE_K, key * 32u + pair);
  const int32_t mag = 2 + static_cast<int32_t>((h & 0xFFFFu) % 5u);
  return (h >> 31) ? -mag : mag;
}

// the three distinct live pairs of a key and their t = +-1
MI355X_DPGM_HD void dpat_live(uint32_t seed, uint32_t key, uint32_t pair[3], int32_t t[3]) {
  const uint32_t h = dpbf_hash(seed, MI355X_DPAT_SPACE_LIVE, key);
  pair[0] = h & 31u;
  pair[1] = (pair[0] + 1u + ((h >> 5) & 15u)) & 31u;   // 1..16 further
  pair[2] = (pair[1] + 1u + ((h >> 9) & 7u)) & 31u;    // 1..8 further: 2..24 from the first
  for (uint32_t i = 0; i < 3; ++i) t[i] = ((h >> (12u + i)) & 1u) ? -1 : 1;
}

// S of (query, key) from the three live terms
MI355X_DPGM_HD int32_t dpat_score(uint32_t seed, uint32_t query, uint32_t key) {
  uint32_t pair[3];
  int32_t t[3];
  dpat_live(seed, key, pair, t);
  return dpat_a(seed, query, pair[0]) * t[0] + dpat_a(seed, query, pair[1]) * t[1] + dpat_a(seed, query, pair[2]) * t[2];
}

// the dword holding elements 2 * pair and 2 * pair + 1 of a row of Q
MI355X_DPGM_HD uint32_t dpat_q_dword(uint32_t nonce, uint32_t seed, uint32_t query, uint32_t pair) {
  const int32_t a = dpat_a(seed, query, pair);
  return dpat_bf16_int(a) | (dpat_bf16_int(dpat_shape(nonce, pair) ? 2 * a : a) << 16);
}

// likewise of a row of K
MI355X_DPGM_HD uint32_t dpat_k_dword(uint32_t nonce, uint32_t seed, uint32_t key, uint32_t pair) {
  const int32_t x = dpat_x(seed, key, pair);
  uint32_t live[3];
  int32_t t[3];
  dpat_live(seed, key, live, t);
  int32_t first = dpat_shape(nonce, pair) ? 2 * x : x;
  for (uint32_t i = 0; i < 3; ++i)
    if (live[i] == pair) first += t[i];
  return dpat_bf16_int(first) | (dpat_bf16_int(-x) << 16);
}

MI355X_DPGM_HD uint32_t dpat_ev(uint32_t seed, uint32_t d) { return dpgm_exp_field(seed, MI355X_DPAT_SPACE_EV, d); }

// V's integer +-{1,2,3} of (key, d): the halves of one hash word serve d and d ^ 1
MI355X_DPGM_HD int32_t dpat_v_int(uint32_t seed, uint32_t key, uint32_t d) {
  const uint32_t h = dpbf_hash(seed, MI355X_DPAT_SPACE_V, key * 32u + (d >> 1));
  const uint32_t h16 = (d & 1u) ? (h >> 16) : (h & 0xFFFFu);
  const int32_t mag = 1 + static_cast<int32_t>((h16 & 0x7FFFu) % 3u);
  return (h16 >> 15) ? -mag : mag;
}

// element (key, d) of V: +-{1,2,3} * 2^(Ev_d - 127)
MI355X_DPGM_HD uint32_t dpat_v_elem(uint32_t seed, uint32_t key, uint32_t d) {
  return dpat_bf16_int(dpat_v_int(seed, key, d)) + ((dpat_ev(seed, d) - 127u) << 7);
}

// LDS byte offset within the V tile of the 16-byte chunk (key of the block, d-chunk 0..7); K uses dpgm_lds_a
MI355X_DPGM_HD uint32_t dpat_v_swz(uint32_t key) { return ((key >> 1) & 1u) << 2; }
MI355X_DPGM_HD uint32_t dpat_lds_v(uint32_t key, uint32_t dc) { return key * 128u + ((dc ^ dpat_v_swz(key)) << 4); }

// the f32 word of n * 2^x, |n| < 2^24; zero is +0
MI355X_DPGM_HD uint32_t dpat_word(int32_t n, int32_t x) { return n == 0 ? 0u : dpbf_scaled_int(n, x); }

// where word `word` (wave * 2 + {0 xor, 1 sum}) of feed stage `stage` (0 = K, 1 = V) sits in a record
MI355X_DPGM_HD uint32_t dpat_fold_slot(uint32_t stage, uint32_t word) {
  return MI355X_DPATREC_FOLD + (word >> 1) * 4u + stage * 2u + (word & 1u);
}
