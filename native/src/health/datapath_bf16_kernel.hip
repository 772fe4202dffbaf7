// gfx950 (CDNA4) bf16 MFMA datapath kernel: see datapath_bf16_kernel.h for the
// operand recipe and why every stage is exact.
//
// Launch: `grid` workgroups x 256 lanes (4 waves). Straight-line, like
// mi355x_mfma_datapath_i8: no inter-workgroup synchronisation and no waiting
// loop; where the workgroups land is reported (XCC id, HW_ID per wave), not
// arranged. Each wave runs four stages of one v_mfma_f32_32x32x16_bf16 and one
// of v_mfma_f32_16x16x32_bf16 on 128-bit operands generated in registers, and
// compares its accumulator registers, as words, with a k-ordered VALU fmaf
// chain over the regenerated operands widened to f32 (exact for these
// operands; no v_dot2 form, whose numerics are as undocumented as the
// MFMA's). Wave 0's tiles also go to the host, which checks them word for
// word (datapath_bf16_verify.h).
//
// 32x32x16: lane l holds fragment (row / column l&31, k = 8*(l>>5) + e);
// accumulator register r of lane l is D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
// 16x16x32: lane l holds fragment (row / column l&15, k = 8*(l>>4) + e);
// accumulator register r of lane l is D[4*(l>>4) + r][l&15].
#include <hip/hip_runtime.h>

#include "datapath_bf16_kernel.h"

typedef __bf16 dpbf_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t dpbf_u32x4 __attribute__((ext_vector_type(4)));
typedef float dpbf_f32x4 __attribute__((ext_vector_type(4)));
typedef float dpbf_f32x16 __attribute__((ext_vector_type(16)));

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPBF_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPBF_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))

// the non-MFMA value of D[row][col] of `stage`: C, then one fmaf per k in k
// order, with B's column `b` (blocks * 4 words) at hand
template <uint32_t kBlocks>
__device__ inline uint32_t dpbf_want(uint32_t stage, uint32_t row, uint32_t col, uint32_t nw,
                                     const uint32_t (&b)[kBlocks * 4]) {
  float s = __uint_as_float(dpbf_c_word(stage, row, col, nw));
#pragma unroll
  for (uint32_t h = 0; h < kBlocks; ++h) {
    uint32_t a[4];
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) a[d] = dpbf_a_word(stage, row, h, d, nw);
#pragma unroll
    for (uint32_t e = 0; e < 8; ++e)
      s = __builtin_fmaf(__uint_as_float(dpbf_widen(a[e >> 1], e & 1)),
                         __uint_as_float(dpbf_widen(b[h * 4 + (e >> 1)], e & 1)), s);
  }
  return __float_as_uint(s);
}

extern "C" __global__ __launch_bounds__(MI355X_DPBF_THREADS) void mi355x_mfma_datapath_bf16(
    mi355x_datapath_bf16_args args) {
  __shared__ uint32_t ctr[12];  // 0..4 bad elements per stage, 8..11 HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid >> 6;
  const uint32_t lane = tid & 63;
  const uint32_t wg = blockIdx.x;
  if (wg >= args.grid) return;
  if (tid < 12) ctr[tid] = 0;
  __syncthreads();

  const uint32_t nw = dpbf_wave_nonce(args.nonce, wg, wave);
  uint32_t* tiles = args.tiles + static_cast<size_t>(wg) * MI355X_DPBF_WG_WORDS;
#if defined(MI355X_TEST_INJECT)
  const bool hit = args.inject_kind == MI355X_DPBF_INJECT_MFMA && wg == args.inject_wg &&
                   wave == args.inject_wave && lane == args.inject_lane;
#endif
  {
    const uint32_t col = lane & 31;
    const uint32_t blk = lane >> 5;
    // one copy of the stage's code, `stage` at run time
#pragma unroll 1
    for (uint32_t stage = 0; stage < MI355X_DPBF_WIDE_STAGES; ++stage) {
      dpbf_u32x4 a, b;
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) {
        a[d] = dpbf_a_word(stage, col, blk, d, nw);
        b[d] = dpbf_b_word(stage, col, blk, d, nw);
      }
      dpbf_f32x16 acc;
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r)
        acc[r] = __uint_as_float(dpbf_c_word(stage, (r & 3) + 8 * (r >> 2) + 4 * blk, col, nw));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(dpbf_bf16x8, a),
                                                    __builtin_bit_cast(dpbf_bf16x8, b), acc, 0, 0, 0);
      uint32_t got[16];
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r) got[r] = __float_as_uint(acc[r]);
#if defined(MI355X_TEST_INJECT)
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r)
        if (hit && stage * 16 + r == args.inject_index) got[r] ^= args.inject_mask;
#endif
      uint32_t bcol[8];  // column `col` of B, both blocks
#pragma unroll
      for (uint32_t w = 0; w < 8; ++w) bcol[w] = dpbf_b_word(stage, col, w >> 2, w & 3, nw);
      uint32_t bad = 0;
      // one row per trip, the register picked by a select chain: unrolled, the
      // compiler keeps the operand hashes of all 16 rows live at once and spills
#pragma unroll 1
      for (uint32_t r = 0; r < 16; ++r) {
        uint32_t g = got[0];
#pragma unroll
        for (uint32_t k = 1; k < 16; ++k) g = r == k ? got[k] : g;
        const uint32_t i = (r & 3) + 8 * (r >> 2) + 4 * blk;
        bad += g != dpbf_want<2>(stage, i, col, nw, bcol);
        if (wave == 0) tiles[dpbf_tile_offset(stage) + i * 32 + col] = g;
      }
      if (bad) atomicAdd(&ctr[stage], bad);
    }
  }
  {
    const uint32_t stage = 4;
    const uint32_t col = lane & 15;
    const uint32_t blk = lane >> 4;
    dpbf_u32x4 a, b;
    dpbf_f32x4 acc;
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
      a[d] = dpbf_a_word(stage, col, blk, d, nw);
      b[d] = dpbf_b_word(stage, col, blk, d, nw);
      acc[d] = __uint_as_float(dpbf_c_word(stage, 4 * blk + d, col, nw));
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dpbf_bf16x8, a),
                                                  __builtin_bit_cast(dpbf_bf16x8, b), acc, 0, 0, 0);
    uint32_t got[4];
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) got[r] = __float_as_uint(acc[r]);
#if defined(MI355X_TEST_INJECT)
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
      if (hit && stage * 16 + r == args.inject_index) got[r] ^= args.inject_mask;
#endif
    uint32_t bcol[16];  // column `col` of B, all four blocks
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) bcol[w] = dpbf_b_word(stage, col, w >> 2, w & 3, nw);
    uint32_t bad = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t i = 4 * blk + r;
      bad += got[r] != dpbf_want<4>(stage, i, col, nw, bcol);
      if (wave == 0) tiles[dpbf_tile_offset(stage) + i * 16 + col] = got[r];
    }
    if (bad) atomicAdd(&ctr[stage], bad);
  }
  if (lane == 0) ctr[8 + wave] = __builtin_amdgcn_s_getreg(MI355X_DPBF_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DPBF_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPBFREC_MAGIC) v = MI355X_DPBF_MAGIC;
    if (tid == MI355X_DPBFREC_WG) v = wg;
    if (tid == MI355X_DPBFREC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPBFREC_XCC) v = __builtin_amdgcn_s_getreg(MI355X_DPBF_HWREG_XCC_ID) & 0xF;
    if (tid >= MI355X_DPBFREC_HWID && tid < MI355X_DPBFREC_HWID + 4) v = ctr[8 + tid - MI355X_DPBFREC_HWID];
    if (tid >= MI355X_DPBFREC_BAD && tid < MI355X_DPBFREC_BAD + MI355X_DPBF_STAGES) v = ctr[tid - MI355X_DPBFREC_BAD];
    args.records[static_cast<size_t>(wg) * MI355X_DPBF_REC_WORDS + tid] = v;
  }
}
