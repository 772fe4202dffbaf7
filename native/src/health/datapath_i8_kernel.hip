// gfx950 (CDNA4) int8 MFMA datapath kernel: see datapath_i8_kernel.h for the
// operand recipe and why no stage can overflow.
//
// Launch: `grid` workgroups x 256 lanes (4 waves). Straight-line, like
// mi355x_mfma_datapath: no inter-workgroup synchronisation and no waiting
// loop; where the workgroups land is reported (XCC id, HW_ID per wave), not
// arranged. Each wave runs four stages of one v_mfma_i32_32x32x32_i8 and one
// of v_mfma_i32_16x16x64_i8 on 128-bit operands generated in registers, and
// compares its accumulator registers, as words, with a v_dot4 recomputation
// from regenerated operands. Wave 0's tiles also go to the host, which checks
// them word for word (datapath_i8_verify.h).
//
// 32x32x32: lane l holds fragment (row / column l&31, block l>>5); accumulator
// register r of lane l is D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
// 16x16x64: lane l holds fragment (row / column l&15, block l>>4); accumulator
// register r of lane l is D[4*(l>>4) + r][l&15].
#include <hip/hip_runtime.h>

#include "datapath_i8_kernel.h"

typedef int dpi8_i32x4 __attribute__((ext_vector_type(4)));
typedef int dpi8_i32x16 __attribute__((ext_vector_type(16)));

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPI8_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPI8_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))

// the non-MFMA value of D[row][col] of `stage`: C plus the dot product over
// every block and dword, with B's fragment `b` (blocks * 4 words) at hand
template <uint32_t kBlocks>
__device__ inline uint32_t dpi8_want(uint32_t stage, uint32_t row, uint32_t col, uint32_t nw,
                                     const uint32_t (&b)[kBlocks * 4]) {
  int32_t s = static_cast<int32_t>(dpi8_c_word(stage, row, col, nw));
#pragma unroll
  for (uint32_t h = 0; h < kBlocks; ++h)
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d)
      s = __builtin_amdgcn_sdot4(static_cast<int32_t>(dpi8_a_word(stage, row, h, d, nw)),
                                 static_cast<int32_t>(b[h * 4 + d]), s, false);
  return static_cast<uint32_t>(s);
}

extern "C" __global__ __launch_bounds__(MI355X_DPI8_THREADS) void mi355x_mfma_datapath_i8(
    mi355x_datapath_i8_args args) {
  __shared__ uint32_t ctr[12];  // 0..4 bad elements per stage, 8..11 HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid >> 6;
  const uint32_t lane = tid & 63;
  const uint32_t wg = blockIdx.x;
  if (wg >= args.grid) return;
  if (tid < 12) ctr[tid] = 0;
  __syncthreads();

  const uint32_t nw = dpi8_wave_nonce(args.nonce, wg, wave);
  uint32_t* tiles = args.tiles + static_cast<size_t>(wg) * MI355X_DPI8_WG_WORDS;
#if defined(MI355X_TEST_INJECT)
  const bool hit = args.inject_kind == MI355X_DPI8_INJECT_MFMA && wg == args.inject_wg &&
                   wave == args.inject_wave && lane == args.inject_lane;
#endif
  {
    const uint32_t col = lane & 31;
    const uint32_t blk = lane >> 5;
#pragma unroll
    for (uint32_t stage = 0; stage < MI355X_DPI8_WIDE_STAGES; ++stage) {
      dpi8_i32x4 a, b;
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) {
        a[d] = static_cast<int>(dpi8_a_word(stage, col, blk, d, nw));
        b[d] = static_cast<int>(dpi8_b_word(stage, col, blk, d, nw));
      }
      dpi8_i32x16 acc;
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r)
        acc[r] = static_cast<int>(dpi8_c_word(stage, (r & 3) + 8 * (r >> 2) + 4 * blk, col, nw));
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
#if defined(MI355X_TEST_INJECT)
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r)
        if (hit && stage * 16 + r == args.inject_index) acc[r] ^= static_cast<int>(args.inject_mask);
#endif
      uint32_t bcol[8];  // column `col` of B, both blocks
#pragma unroll
      for (uint32_t w = 0; w < 8; ++w) bcol[w] = dpi8_b_word(stage, col, w >> 2, w & 3, nw);
      uint32_t bad = 0;
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r) {
        const uint32_t i = (r & 3) + 8 * (r >> 2) + 4 * blk;
        const uint32_t got = static_cast<uint32_t>(acc[r]);
        bad += got != dpi8_want<2>(stage, i, col, nw, bcol);
        if (wave == 0) tiles[dpi8_tile_offset(stage) + i * 32 + col] = got;
      }
      if (bad) atomicAdd(&ctr[stage], bad);
    }
  }
  {
    const uint32_t stage = 4;
    const uint32_t col = lane & 15;
    const uint32_t blk = lane >> 4;
    dpi8_i32x4 a, b, acc;
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
      a[d] = static_cast<int>(dpi8_a_word(stage, col, blk, d, nw));
      b[d] = static_cast<int>(dpi8_b_word(stage, col, blk, d, nw));
      acc[d] = static_cast<int>(dpi8_c_word(stage, 4 * blk + d, col, nw));
    }
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
#if defined(MI355X_TEST_INJECT)
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
      if (hit && stage * 16 + r == args.inject_index) acc[r] ^= static_cast<int>(args.inject_mask);
#endif
    uint32_t bcol[16];  // column `col` of B, all four blocks
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) bcol[w] = dpi8_b_word(stage, col, w >> 2, w & 3, nw);
    uint32_t bad = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t i = 4 * blk + r;
      const uint32_t got = static_cast<uint32_t>(acc[r]);
      bad += got != dpi8_want<4>(stage, i, col, nw, bcol);
      if (wave == 0) tiles[dpi8_tile_offset(stage) + i * 16 + col] = got;
    }
    if (bad) atomicAdd(&ctr[stage], bad);
  }
  if (lane == 0) ctr[8 + wave] = __builtin_amdgcn_s_getreg(MI355X_DPI8_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DPI8_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPI8REC_MAGIC) v = MI355X_DPI8_MAGIC;
    if (tid == MI355X_DPI8REC_WG) v = wg;
    if (tid == MI355X_DPI8REC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPI8REC_XCC) v = __builtin_amdgcn_s_getreg(MI355X_DPI8_HWREG_XCC_ID) & 0xF;
    if (tid >= MI355X_DPI8REC_HWID && tid < MI355X_DPI8REC_HWID + 4) v = ctr[8 + tid - MI355X_DPI8REC_HWID];
    if (tid >= MI355X_DPI8REC_BAD && tid < MI355X_DPI8REC_BAD + MI355X_DPI8_STAGES) v = ctr[tid - MI355X_DPI8REC_BAD];
    args.records[static_cast<size_t>(wg) * MI355X_DPI8_REC_WORDS + tid] = v;
  }
}
