// gfx950 (CDNA4) fp8 / MX-scaled MFMA datapath kernel: see datapath_fp8_kernel.h
// for the operand recipe and why every stage is exact.
//
// Launch: `grid` workgroups x 256 lanes (4 waves). Straight-line, like
// mi355x_mfma_datapath_bf16: no inter-workgroup synchronisation and no waiting
// loop; where the workgroups land is reported (XCC id, HW_ID per wave), not
// arranged. Each wave runs eight stages of one MFMA each -- three
// v_mfma_f32_32x32x16_{fp8,bf8}_{fp8,bf8}, one v_mfma_f32_16x16x32_bf8_fp8,
// three v_mfma_scale_f32_32x32x64_f8f6f4 and one
// v_mfma_scale_f32_16x16x128_f8f6f4 -- on operands generated in registers, and
// compares its accumulator registers, as words, with a k-ordered VALU fmaf
// chain over the regenerated operands, decoded to f32 by integer arithmetic
// and scaled by exact powers of two (exact for these operands; no v_cvt of
// fp8, which would be a second copy of the decoder under test). Wave 0's tiles
// also go to the host, which checks them word for word (datapath_fp8_verify.h).
//
// 32x32: lane l holds fragment (row / column l&31, K-block l>>5) and, in the
// scaled form, the scale of scale block l>>5 (dpf8_scale_block: not its own
// fragment) in the selected byte of its scale VGPR;
// accumulator register r of lane l is D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
// 16x16: lane l holds fragment (row / column l&15, K-block l>>4);
// accumulator register r of lane l is D[4*(l>>4) + r][l&15].
#include <hip/hip_runtime.h>

#include "datapath_fp8_kernel.h"

typedef int dpf8_i32x8 __attribute__((ext_vector_type(8)));

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPF8_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPF8_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))

// the non-MFMA value of D[row][col] of stage S: C, then one fmaf per k in k
// order, with B's column `b` (blocks * dwords words) and its scale blocks' scales at hand
template <uint32_t S, uint32_t kWords, uint32_t kBlocks>
__device__ inline uint32_t dpf8_want(uint32_t row, uint32_t col, uint32_t nw, const uint32_t (&b)[kWords],
                                     const float (&sb)[kBlocks]) {
  constexpr uint32_t kDwords = kWords / kBlocks;
  float s = __uint_as_float(dpf8_c_word(S, row, col, nw));
  float sa[kBlocks];  // the row's scales, per scale block
#pragma unroll
  for (uint32_t g = 0; g < kBlocks; ++g)
    sa[g] = S >= 4 ? __uint_as_float(dpf8_scale_f32(dpf8_scale_byte(nw, S, 0, row, g))) : 1.0f;
#pragma unroll
  for (uint32_t h = 0; h < kBlocks; ++h) {
#pragma unroll
    for (uint32_t d = 0; d < kDwords; ++d) {
      const uint32_t g = dpf8_scale_block(S, h, d);
      const uint32_t aw = dpf8_a_word(S, row, h, d, nw);
      const uint32_t bw = b[h * kDwords + d];
#pragma unroll
      for (uint32_t e = 0; e < 4; ++e) {
        float x = __uint_as_float(dpf8_decode((aw >> (8 * e)) & 0xFFu, dpf8_fmt_a(S)));
        float y = __uint_as_float(dpf8_decode((bw >> (8 * e)) & 0xFFu, dpf8_fmt_b(S)));
        if constexpr (S >= 4) {
          x *= sa[g];
          y *= sb[g];
        }
        s = __builtin_fmaf(x, y, s);
      }
    }
  }
  return __float_as_uint(s);
}

// one stage of one wave: operands, the MFMA, the comparison, wave 0's tile
template <uint32_t S>
__device__ inline void dpf8_stage(const mi355x_datapath_fp8_args& args, uint32_t wg, uint32_t nw, uint32_t lane,
                                  uint32_t wave, uint32_t* tiles, uint32_t* ctr) {
  constexpr uint32_t kDim = (S == 3 || S == 7) ? 16 : 32;
  constexpr uint32_t kBlocks = kDim == 16 ? 4 : 2;
  constexpr uint32_t kDwords = S >= 4 ? 8 : 2;
  constexpr uint32_t kRegs = kDim == 16 ? 4 : 16;
  typedef float acc_t __attribute__((ext_vector_type(kRegs)));
  const uint32_t col = lane & (kDim - 1);
  const uint32_t blk = lane / kDim;
  const auto row_of = [blk](uint32_t r) { return kDim == 16 ? 4 * blk + r : (r & 3) + 8 * (r >> 2) + 4 * blk; };

  uint32_t a[kDwords], b[kDwords];
#pragma unroll
  for (uint32_t d = 0; d < kDwords; ++d) {
    a[d] = dpf8_a_word(S, col, blk, d, nw);
    b[d] = dpf8_b_word(S, col, blk, d, nw);
  }
  acc_t acc;
#pragma unroll
  for (uint32_t r = 0; r < kRegs; ++r) acc[r] = __uint_as_float(dpf8_c_word(S, row_of(r), col, nw));

  if constexpr (S < 4) {
    const long a64 = static_cast<long>((static_cast<uint64_t>(a[1]) << 32) | a[0]);
    const long b64 = static_cast<long>((static_cast<uint64_t>(b[1]) << 32) | b[0]);
    if constexpr (S == 0) acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a64, b64, acc, 0, 0, 0);
    if constexpr (S == 1) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf8_bf8(a64, b64, acc, 0, 0, 0);
    if constexpr (S == 2) acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_bf8(a64, b64, acc, 0, 0, 0);
    if constexpr (S == 3) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf8_fp8(a64, b64, acc, 0, 0, 0);
  } else {
    dpf8_i32x8 a8, b8;
#pragma unroll
    for (uint32_t d = 0; d < 8; ++d) {
      a8[d] = static_cast<int>(a[d]);
      b8[d] = static_cast<int>(b[d]);
    }
    // cbsz / blgp: 0 = e4m3, 1 = e5m2; the scale VGPRs' selected bytes: S-4 for A, 7-S for B
    const int sa = static_cast<int>(dpf8_scale_word(nw, S, 0, col, blk));
    const int sb = static_cast<int>(dpf8_scale_word(nw, S, 1, col, blk));
    if constexpr (S == 4) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 0, 1, 0, sa, 3, sb);
    if constexpr (S == 5) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 1, 0, 1, sa, 2, sb);
    if constexpr (S == 6) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 0, 0, 2, sa, 1, sb);
    if constexpr (S == 7) acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, acc, 1, 1, 3, sa, 0, sb);
  }
  uint32_t got[kRegs];
#pragma unroll
  for (uint32_t r = 0; r < kRegs; ++r) got[r] = __float_as_uint(acc[r]);
#if defined(MI355X_TEST_INJECT)
  const bool hit = args.inject_kind == MI355X_DPF8_INJECT_MFMA && wg == args.inject_wg &&
                   wave == args.inject_wave && lane == args.inject_lane;
#pragma unroll
  for (uint32_t r = 0; r < kRegs; ++r)
    if (hit && S * 16 + r == args.inject_index) got[r] ^= args.inject_mask;
#endif
  uint32_t bcol[kBlocks * kDwords];  // column `col` of B, every block
  float sbcol[kBlocks];              // and the blocks' scales (1 in the non-scaled stages)
#pragma unroll
  for (uint32_t h = 0; h < kBlocks; ++h) {
    sbcol[h] = S >= 4 ? __uint_as_float(dpf8_scale_f32(dpf8_scale_byte(nw, S, 1, col, h))) : 1.0f;
#pragma unroll
    for (uint32_t d = 0; d < kDwords; ++d) bcol[h * kDwords + d] = dpf8_b_word(S, col, h, d, nw);
  }
  uint32_t bad = 0;
  // one row per trip, the register picked by a select chain: unrolled, the
  // compiler keeps the operand hashes of all rows live at once and spills
#pragma unroll 1
  for (uint32_t r = 0; r < kRegs; ++r) {
    uint32_t g = got[0];
#pragma unroll
    for (uint32_t k = 1; k < kRegs; ++k) g = r == k ? got[k] : g;
    const uint32_t i = row_of(r);
    bad += g != dpf8_want<S>(i, col, nw, bcol, sbcol);
    if (wave == 0) tiles[dpf8_tile_offset(S) + i * kDim + col] = g;
  }
  if (bad) atomicAdd(&ctr[S], bad);
}

#define MI355X_DPF8_STAGE(S) dpf8_stage<S>(args, wg, nw, lane, wave, tiles, ctr)

extern "C" __global__ __launch_bounds__(MI355X_DPF8_THREADS) void mi355x_mfma_datapath_fp8(
    mi355x_datapath_fp8_args args) {
  __shared__ uint32_t ctr[12];  // 0..7 bad elements per stage, 8..11 HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid >> 6;
  const uint32_t lane = tid & 63;
  const uint32_t wg = blockIdx.x;
  if (wg >= args.grid) return;
  if (tid < 12) ctr[tid] = 0;
  __syncthreads();

  const uint32_t nw = dpf8_wave_nonce(args.nonce, wg, wave);
  uint32_t* tiles = args.tiles + static_cast<size_t>(wg) * MI355X_DPF8_WG_WORDS;
  MI355X_DPF8_STAGE(0);
  MI355X_DPF8_STAGE(1);
  MI355X_DPF8_STAGE(2);
  MI355X_DPF8_STAGE(3);
  MI355X_DPF8_STAGE(4);
  MI355X_DPF8_STAGE(5);
  MI355X_DPF8_STAGE(6);
  MI355X_DPF8_STAGE(7);
  if (lane == 0) ctr[8 + wave] = __builtin_amdgcn_s_getreg(MI355X_DPF8_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DPF8_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPF8REC_MAGIC) v = MI355X_DPF8_MAGIC;
    if (tid == MI355X_DPF8REC_WG) v = wg;
    if (tid == MI355X_DPF8REC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPF8REC_XCC) v = __builtin_amdgcn_s_getreg(MI355X_DPF8_HWREG_XCC_ID) & 0xF;
    if (tid >= MI355X_DPF8REC_HWID && tid < MI355X_DPF8REC_HWID + 4) v = ctr[8 + tid - MI355X_DPF8REC_HWID];
    if (tid >= MI355X_DPF8REC_BAD && tid < MI355X_DPF8REC_BAD + MI355X_DPF8_STAGES) v = ctr[tid - MI355X_DPF8REC_BAD];
    args.records[static_cast<size_t>(wg) * MI355X_DPF8_REC_WORDS + tid] = v;
  }
}
