// gfx950 (CDNA4) f16 MFMA datapath kernel: see datapath_f16_kernel.h for the
// operand recipe and why every stage is exact.
//
// Launch: `grid` workgroups x 256 lanes (4 waves). Straight-line, like
// mi355x_mfma_datapath_bf16: no inter-workgroup synchronisation and no waiting
// loop; where the workgroups land is reported (XCC id, HW_ID per wave), not
// arranged. Each wave runs four stages of one v_mfma_f32_32x32x16_f16 and one
// stage each of v_mfma_f32_16x16x32_f16, v_mfma_f32_32x32x8_f16 and
// v_mfma_f32_16x16x16_f16 on operands generated in registers, and compares its
// accumulator registers, as words, with a k-ordered VALU fmaf chain over the
// regenerated operands widened to f32 by integer arithmetic (exact for these
// operands; no v_cvt_f32_f16 and no v_dot2 form). Wave 0's tiles also go to
// the host, which checks them word for word (datapath_f16_verify.h).
//
// 32x32 forms: lane l holds fragment (row / column l&31, k = kw*(l>>5) + e),
// kw = 8 for 32x32x16 and 4 for 32x32x8; accumulator register r of lane l is
// D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
// 16x16 forms: lane l holds fragment (row / column l&15, k = kw*(l>>4) + e),
// kw = 8 for 16x16x32 and 4 for 16x16x16; accumulator register r of lane l is
// D[4*(l>>4) + r][l&15].
#include <hip/hip_runtime.h>

#include "datapath_f16_kernel.h"

typedef _Float16 dphf_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 dphf_f16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t dphf_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t dphf_u32x2 __attribute__((ext_vector_type(2)));
typedef float dphf_f32x4 __attribute__((ext_vector_type(4)));
typedef float dphf_f32x16 __attribute__((ext_vector_type(16)));

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPHF_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPHF_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))

// the non-MFMA value of D[row][col] of `stage`: C, then one fmaf per k in k
// order, with B's column `b` (kBlocks * kDwords words) at hand
template <uint32_t kBlocks, uint32_t kDwords>
__device__ inline uint32_t dphf_want(uint32_t stage, uint32_t row, uint32_t col, uint32_t nw,
                                     const uint32_t (&b)[kBlocks * kDwords]) {
  float s = __uint_as_float(dphf_c_word(stage, row, col, nw));
#pragma unroll
  for (uint32_t h = 0; h < kBlocks; ++h) {
    uint32_t a[kDwords];
#pragma unroll
    for (uint32_t d = 0; d < kDwords; ++d) a[d] = dphf_a_word(stage, row, h, d, nw);
#pragma unroll
    for (uint32_t e = 0; e < 2 * kDwords; ++e)
      s = __builtin_fmaf(__uint_as_float(dphf_widen(a[e >> 1], e & 1)),
                         __uint_as_float(dphf_widen(b[h * kDwords + (e >> 1)], e & 1)), s);
  }
  return __float_as_uint(s);
}

// one 32x32 stage of one wave: kDwords = 4 is v_mfma_f32_32x32x16_f16, 2 is
// v_mfma_f32_32x32x8_f16. Returns the lane's count of wrong accumulator words.
template <uint32_t kDwords>
__device__ inline uint32_t dphf_stage32(uint32_t stage, uint32_t wg, uint32_t wave, uint32_t lane,
                                        const mi355x_datapath_f16_args& args) {
  const uint32_t nw = dphf_wave_nonce(args.nonce, wg, wave);
  uint32_t* tile = args.tiles + static_cast<size_t>(wg) * MI355X_DPHF_WG_WORDS + dphf_tile_offset(stage);
  const uint32_t col = lane & 31;
  const uint32_t blk = lane >> 5;
  uint32_t a[kDwords], b[kDwords];
#pragma unroll
  for (uint32_t d = 0; d < kDwords; ++d) {
    a[d] = dphf_a_word(stage, col, blk, d, nw);
    b[d] = dphf_b_word(stage, col, blk, d, nw);
  }
  dphf_f32x16 acc;
#pragma unroll
  for (uint32_t r = 0; r < 16; ++r)
    acc[r] = __uint_as_float(dphf_c_word(stage, (r & 3) + 8 * (r >> 2) + 4 * blk, col, nw));
  if constexpr (kDwords == 4) {
    const dphf_u32x4 av = {a[0], a[1], a[2], a[3]}, bv = {b[0], b[1], b[2], b[3]};
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(dphf_f16x8, av),
                                                 __builtin_bit_cast(dphf_f16x8, bv), acc, 0, 0, 0);
  } else {
    const dphf_u32x2 av = {a[0], a[1]}, bv = {b[0], b[1]};
    acc = __builtin_amdgcn_mfma_f32_32x32x8f16(__builtin_bit_cast(dphf_f16x4, av),
                                               __builtin_bit_cast(dphf_f16x4, bv), acc, 0, 0, 0);
  }
  uint32_t got[16];
#pragma unroll
  for (uint32_t r = 0; r < 16; ++r) got[r] = __float_as_uint(acc[r]);
#if defined(MI355X_TEST_INJECT)
  const bool hit = args.inject_kind == MI355X_DPHF_INJECT_MFMA && wg == args.inject_wg &&
                   wave == args.inject_wave && lane == args.inject_lane;
#pragma unroll
  for (uint32_t r = 0; r < 16; ++r)
    if (hit && stage * 16 + r == args.inject_index) got[r] ^= args.inject_mask;
#endif
  uint32_t bcol[2 * kDwords];  // column `col` of B, both blocks
#pragma unroll
  for (uint32_t w = 0; w < 2 * kDwords; ++w) bcol[w] = dphf_b_word(stage, col, w / kDwords, w % kDwords, nw);
  uint32_t bad = 0;
  // one row per trip, the register picked by a select chain: unrolled, the
  // compiler keeps the operand hashes of all 16 rows live at once and spills
#pragma unroll 1
  for (uint32_t r = 0; r < 16; ++r) {
    uint32_t g = got[0];
#pragma unroll
    for (uint32_t k = 1; k < 16; ++k) g = r == k ? got[k] : g;
    const uint32_t i = (r & 3) + 8 * (r >> 2) + 4 * blk;
    bad += g != dphf_want<2, kDwords>(stage, i, col, nw, bcol);
    if (wave == 0) tile[i * 32 + col] = g;
  }
  return bad;
}

// one 16x16 stage of one wave: kDwords = 4 is v_mfma_f32_16x16x32_f16, 2 is
// v_mfma_f32_16x16x16_f16
template <uint32_t kDwords>
__device__ inline uint32_t dphf_stage16(uint32_t stage, uint32_t wg, uint32_t wave, uint32_t lane,
                                        const mi355x_datapath_f16_args& args) {
  const uint32_t nw = dphf_wave_nonce(args.nonce, wg, wave);
  uint32_t* tile = args.tiles + static_cast<size_t>(wg) * MI355X_DPHF_WG_WORDS + dphf_tile_offset(stage);
  const uint32_t col = lane & 15;
  const uint32_t blk = lane >> 4;
  uint32_t a[kDwords], b[kDwords];
#pragma unroll
  for (uint32_t d = 0; d < kDwords; ++d) {
    a[d] = dphf_a_word(stage, col, blk, d, nw);
    b[d] = dphf_b_word(stage, col, blk, d, nw);
  }
  dphf_f32x4 acc;
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) acc[r] = __uint_as_float(dphf_c_word(stage, 4 * blk + r, col, nw));
  if constexpr (kDwords == 4) {
    const dphf_u32x4 av = {a[0], a[1], a[2], a[3]}, bv = {b[0], b[1], b[2], b[3]};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(dphf_f16x8, av),
                                                 __builtin_bit_cast(dphf_f16x8, bv), acc, 0, 0, 0);
  } else {
    const dphf_u32x2 av = {a[0], a[1]}, bv = {b[0], b[1]};
    acc = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(dphf_f16x4, av),
                                                __builtin_bit_cast(dphf_f16x4, bv), acc, 0, 0, 0);
  }
  uint32_t got[4];
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) got[r] = __float_as_uint(acc[r]);
#if defined(MI355X_TEST_INJECT)
  const bool hit = args.inject_kind == MI355X_DPHF_INJECT_MFMA && wg == args.inject_wg &&
                   wave == args.inject_wave && lane == args.inject_lane;
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r)
    if (hit && stage * 16 + r == args.inject_index) got[r] ^= args.inject_mask;
#endif
  uint32_t bcol[4 * kDwords];  // column `col` of B, all four blocks
#pragma unroll
  for (uint32_t w = 0; w < 4 * kDwords; ++w) bcol[w] = dphf_b_word(stage, col, w / kDwords, w % kDwords, nw);
  uint32_t bad = 0;
#pragma unroll 1
  for (uint32_t r = 0; r < 4; ++r) {
    uint32_t g = got[0];
#pragma unroll
    for (uint32_t k = 1; k < 4; ++k) g = r == k ? got[k] : g;
    const uint32_t i = 4 * blk + r;
    bad += g != dphf_want<4, kDwords>(stage, i, col, nw, bcol);
    if (wave == 0) tile[i * 16 + col] = g;
  }
  return bad;
}

extern "C" __global__ __launch_bounds__(MI355X_DPHF_THREADS) void mi355x_mfma_datapath_f16(
    mi355x_datapath_f16_args args) {
  __shared__ uint32_t ctr[12];  // 0..6 bad elements per stage, 8..11 HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid >> 6;
  const uint32_t lane = tid & 63;
  const uint32_t wg = blockIdx.x;
  if (wg >= args.grid) return;
  if (tid < 12) ctr[tid] = 0;
  __syncthreads();

  // one copy of the 32x32x16 stage's code, `stage` at run time
#pragma unroll 1
  for (uint32_t stage = 0; stage < MI355X_DPHF_WIDE_STAGES; ++stage) {
    const uint32_t bad = dphf_stage32<4>(stage, wg, wave, lane, args);
    if (bad) atomicAdd(&ctr[stage], bad);
  }
  {
    const uint32_t bad = dphf_stage16<4>(4u, wg, wave, lane, args);
    if (bad) atomicAdd(&ctr[4], bad);
  }
  {
    const uint32_t bad = dphf_stage32<2>(5u, wg, wave, lane, args);
    if (bad) atomicAdd(&ctr[5], bad);
  }
  {
    const uint32_t bad = dphf_stage16<2>(6u, wg, wave, lane, args);
    if (bad) atomicAdd(&ctr[6], bad);
  }
  if (lane == 0) ctr[8 + wave] = __builtin_amdgcn_s_getreg(MI355X_DPHF_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DPHF_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPHFREC_MAGIC) v = MI355X_DPHF_MAGIC;
    if (tid == MI355X_DPHFREC_WG) v = wg;
    if (tid == MI355X_DPHFREC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPHFREC_XCC) v = __builtin_amdgcn_s_getreg(MI355X_DPHF_HWREG_XCC_ID) & 0xF;
    if (tid >= MI355X_DPHFREC_HWID && tid < MI355X_DPHFREC_HWID + 4) v = ctr[8 + tid - MI355X_DPHFREC_HWID];
    if (tid >= MI355X_DPHFREC_BAD && tid < MI355X_DPHFREC_BAD + MI355X_DPHF_STAGES) v = ctr[tid - MI355X_DPHFREC_BAD];
    args.records[static_cast<size_t>(wg) * MI355X_DPHF_REC_WORDS + tid] = v;
  }
}
