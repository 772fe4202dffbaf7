// gfx950 (CDNA4) f64 MFMA datapath kernel: see datapath_f64_kernel.h for the
// operand recipe and why every stage is exact.
//
// Launch: `grid` workgroups x 256 lanes (4 waves). Straight-line, like
// mi355x_mfma_datapath_f16: no inter-workgroup synchronisation and no waiting
// loop; where the workgroups land is reported (XCC id, HW_ID per wave), not
// arranged. Each wave runs nine v_mfma_f64_16x16x4_f64 (stages 0..4, three of
// them with a neg bit) and three v_mfma_f64_4x4x4_4b_f64 (stages 5, 6) on
// operands generated in registers as bit patterns, and compares its accumulator
// registers, as 32-bit words, with a k-ordered VALU v_fma_f64 chain over the
// regenerated operands (exact for these operands); stage 2 also with the
// integer product of the two significands. No instruction converts an integer
// or a float to a double. Wave 0's tiles also go to the host, which checks
// them word for word in integer arithmetic (datapath_f64_verify.h).
//
// Lane maps, as measured on an MI355X from the one-hot tiles of stages 0 and 5
// (distinct band doubles: a wrong map shows as a readable permutation). Both
// forms keep k in the lane's upper two bits on the way in and the output row
// there on the way out:
// 16x16x4: lane l holds A[l&15][k = l>>4] and B[k = l>>4][l&15]; accumulator
// double r of lane l is D[4*r + (l>>4)][l&15] (not the f32 16x16 forms'
// D[4*(l>>4) + r][l&15], which the first run assumed and which came back with
// one word in four equal).
// 4x4x4_4b (4 blocks b, one double of A, B and D per lane): lane l holds
// A[b][i][k] and B[b][k][j] with i or j = l&3, b = (l>>2)&3, k = l>>4, and
// D[b][i][j] with j = l&3, b = (l>>2)&3, i = l>>4 (dpd_4x4_rc, dpd_4x4_k,
// dpd_4x4_d in the header; the first run assumed k = (l>>2)&3, b = l>>4).
#include <hip/hip_runtime.h>

#include "datapath_f64_kernel.h"

typedef double dpd_f64x4 __attribute__((ext_vector_type(4)));

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPD_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPD_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))

__device__ inline double dpd_as_double(uint64_t v) { return __builtin_bit_cast(double, v); }
__device__ inline uint64_t dpd_as_bits(double d) { return __builtin_bit_cast(uint64_t, d); }

// the non-MFMA value of output (row, col) of tile `t` of `stage`: C, then one
// fma per k in k order, with B's column `b` at hand
__device__ inline uint64_t dpd_want(uint32_t stage, uint32_t t, uint32_t row, uint32_t col, uint32_t nw,
                                    const uint64_t (&b)[4]) {
  double s = dpd_as_double(dpd_c_bits(stage, row, col, nw) ^ dpd_neg_c(stage, t));
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k)
    s = __builtin_fma(dpd_as_double(dpd_a_bits(stage, t, row, k, nw) ^ dpd_neg_ab(stage, t)), dpd_as_double(b[k]), s);
  return dpd_as_bits(s);
}

// the wrong words (0..2) of accumulator double `got` of output (row, col) of
// tile `t`; wave 0 stores the double at word `at` of its tile
__device__ inline uint32_t dpd_compare(uint32_t stage, uint32_t t, uint32_t row, uint32_t col, uint32_t nw,
                                       const uint64_t (&b)[4], uint64_t got, uint32_t* tile, uint32_t at,
                                       uint32_t wave) {
  const uint64_t want = dpd_want(stage, t, row, col, nw, b);
  uint64_t diff = got ^ want;
  if (stage == 2u)
    diff |= got ^ dpd_wide_product(dpd_a_bits(2u, 0u, row, dpd_onehot_pos(nw, 2u, col), nw), dpd_hot(nw, 2u, col));
  if (wave == 0) {
    tile[at] = static_cast<uint32_t>(got);
    tile[at + 1] = static_cast<uint32_t>(got >> 32);
  }
  return (static_cast<uint32_t>(diff) != 0u) + (static_cast<uint32_t>(diff >> 32) != 0u);
}

template <int kBlgp>
__device__ inline dpd_f64x4 dpd_mfma16(uint64_t a, uint64_t b, dpd_f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(dpd_as_double(a), dpd_as_double(b), c, 0, 0, kBlgp);
}

// one v_mfma_f64_16x16x4_f64 stage of one wave: kTiles MFMAs (the passes of
// stages 0 and 1; with kNeg the three neg forms of stage 4). Returns the lane's
// count of wrong accumulator words.
template <uint32_t kTiles, bool kNeg>
__device__ inline uint32_t dpd_stage16(uint32_t stage, uint32_t wg, uint32_t wave, uint32_t lane,
                                       const mi355x_datapath_f64_args& args) {
  const uint32_t nw = dpd_wave_nonce(args.nonce, wg, wave);
  uint32_t* tile = args.tiles + static_cast<size_t>(wg) * MI355X_DPD_WG_WORDS + dpd_tile_offset(stage);
  const uint32_t col = lane & 15;
  const uint32_t blk = lane >> 4;
  dpd_f64x4 c;
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) c[r] = dpd_as_double(dpd_c_bits(stage, 4 * r + blk, col, nw));
  dpd_f64x4 acc[kTiles];
  if constexpr (kNeg) {
    static_assert(kTiles == 3, "neg:[1,0,0], [0,1,0], [0,0,1]");
    const uint64_t a = dpd_a_bits(stage, 0u, col, blk, nw), b = dpd_b_bits(stage, 0u, col, blk, nw);
    acc[0] = dpd_mfma16<1>(a, b, c);
    acc[1] = dpd_mfma16<2>(a, b, c);
    acc[2] = dpd_mfma16<4>(a, b, c);
  } else {
#pragma unroll
    for (uint32_t t = 0; t < kTiles; ++t)
      acc[t] = dpd_mfma16<0>(dpd_a_bits(stage, t, col, blk, nw), dpd_b_bits(stage, t, col, blk, nw), c);
  }
  uint32_t got[kTiles * 8];
#pragma unroll
  for (uint32_t w = 0; w < kTiles * 8; ++w) {
    const uint64_t d = dpd_as_bits(acc[w >> 3][(w >> 1) & 3]);
    got[w] = static_cast<uint32_t>((w & 1) ? d >> 32 : d);
  }
#if defined(MI355X_TEST_INJECT)
  const bool hit = args.inject_kind == MI355X_DPD_INJECT_MFMA && wg == args.inject_wg &&
                   wave == args.inject_wave && lane == args.inject_lane;
#pragma unroll
  for (uint32_t w = 0; w < kTiles * 8; ++w)
    if (hit && stage * 32 + w == args.inject_index) got[w] ^= args.inject_mask;
#endif
  uint32_t bad = 0;
#pragma unroll
  for (uint32_t t = 0; t < kTiles; ++t) {
    uint64_t bcol[4];  // column `col` of B in this tile
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) bcol[k] = dpd_b_bits(stage, t, col, k, nw);
    // one row per trip, the register picked by a select chain: unrolled, the
    // compiler keeps the operand hashes of all four rows live at once
#pragma unroll 1
    for (uint32_t r = 0; r < 4; ++r) {
      uint32_t lo = got[t * 8], hi = got[t * 8 + 1];
#pragma unroll
      for (uint32_t k = 1; k < 4; ++k) {
        lo = r == k ? got[t * 8 + 2 * k] : lo;
        hi = r == k ? got[t * 8 + 2 * k + 1] : hi;
      }
      const uint32_t row = 4 * r + blk;
      bad += dpd_compare(stage, t, row, col, nw, bcol, dpd_pack(hi, lo), tile, (t * 256 + row * 16 + col) * 2, wave);
    }
  }
  return bad;
}

// one v_mfma_f64_4x4x4_4b_f64 stage of one wave: kTiles MFMAs, one accumulator
// double a lane each
template <uint32_t kTiles>
__device__ inline uint32_t dpd_stage4(uint32_t stage, uint32_t wg, uint32_t wave, uint32_t lane,
                                      const mi355x_datapath_f64_args& args) {
  const uint32_t nw = dpd_wave_nonce(args.nonce, wg, wave);
  uint32_t* tile = args.tiles + static_cast<size_t>(wg) * MI355X_DPD_WG_WORDS + dpd_tile_offset(stage);
  const uint32_t rc = dpd_4x4_rc(lane), kk = dpd_4x4_k(lane), d = dpd_4x4_d(lane);
  const uint32_t row = dpd_row_of(stage, d), col = dpd_col_of(stage, d);
  const double c = dpd_as_double(dpd_c_bits(stage, row, col, nw));
  uint32_t got[kTiles * 2];
#pragma unroll
  for (uint32_t t = 0; t < kTiles; ++t) {
    const uint64_t acc = dpd_as_bits(__builtin_amdgcn_mfma_f64_4x4x4f64(
        dpd_as_double(dpd_a_bits(stage, t, rc, kk, nw)), dpd_as_double(dpd_b_bits(stage, t, rc, kk, nw)), c, 0, 0, 0));
    got[2 * t] = static_cast<uint32_t>(acc);
    got[2 * t + 1] = static_cast<uint32_t>(acc >> 32);
  }
#if defined(MI355X_TEST_INJECT)
  const bool hit = args.inject_kind == MI355X_DPD_INJECT_MFMA && wg == args.inject_wg &&
                   wave == args.inject_wave && lane == args.inject_lane;
#pragma unroll
  for (uint32_t w = 0; w < kTiles * 2; ++w)
    if (hit && stage * 32 + w == args.inject_index) got[w] ^= args.inject_mask;
#endif
  uint32_t bad = 0;
#pragma unroll
  for (uint32_t t = 0; t < kTiles; ++t) {
    uint64_t bcol[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) bcol[k] = dpd_b_bits(stage, t, col, k, nw);
    bad += dpd_compare(stage, t, row, col, nw, bcol, dpd_pack(got[2 * t + 1], got[2 * t]), tile, (t * 64 + d) * 2, wave);
  }
  return bad;
}

extern "C" __global__ __launch_bounds__(MI355X_DPD_THREADS) void mi355x_mfma_datapath_f64(
    mi355x_datapath_f64_args args) {
  __shared__ uint32_t ctr[12];  // 0..6 bad words per stage, 8..11 HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid >> 6;
  const uint32_t lane = tid & 63;
  const uint32_t wg = blockIdx.x;
  if (wg >= args.grid) return;
  if (tid < 12) ctr[tid] = 0;
  __syncthreads();

  // one copy of the two-pass stage's code and one of the one-tile stage's, `stage` at run time
#pragma unroll 1
  for (uint32_t stage = 0; stage < 2; ++stage) {
    const uint32_t bad = dpd_stage16<2, false>(stage, wg, wave, lane, args);
    if (bad) atomicAdd(&ctr[stage], bad);
  }
#pragma unroll 1
  for (uint32_t stage = 2; stage < 4; ++stage) {
    const uint32_t bad = dpd_stage16<1, false>(stage, wg, wave, lane, args);
    if (bad) atomicAdd(&ctr[stage], bad);
  }
  {
    const uint32_t bad = dpd_stage16<3, true>(4u, wg, wave, lane, args);
    if (bad) atomicAdd(&ctr[4], bad);
  }
  {
    const uint32_t bad = dpd_stage4<2>(5u, wg, wave, lane, args);
    if (bad) atomicAdd(&ctr[5], bad);
  }
  {
    const uint32_t bad = dpd_stage4<1>(6u, wg, wave, lane, args);
    if (bad) atomicAdd(&ctr[6], bad);
  }
  if (lane == 0) ctr[8 + wave] = __builtin_amdgcn_s_getreg(MI355X_DPD_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DPD_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPDREC_MAGIC) v = MI355X_DPD_MAGIC;
    if (tid == MI355X_DPDREC_WG) v = wg;
    if (tid == MI355X_DPDREC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPDREC_XCC) v = __builtin_amdgcn_s_getreg(MI355X_DPD_HWREG_XCC_ID) & 0xF;
    if (tid >= MI355X_DPDREC_HWID && tid < MI355X_DPDREC_HWID + 4) v = ctr[8 + tid - MI355X_DPDREC_HWID];
    if (tid >= MI355X_DPDREC_BAD && tid < MI355X_DPDREC_BAD + MI355X_DPD_STAGES) v = ctr[tid - MI355X_DPDREC_BAD];
    args.records[static_cast<size_t>(wg) * MI355X_DPD_REC_WORDS + tid] = v;
  }
}
