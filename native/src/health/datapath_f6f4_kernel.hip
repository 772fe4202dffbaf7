// gfx950 (CDNA4) fp6 / fp4 MX-scaled MFMA datapath kernel: see
// datapath_f6f4_kernel.h for the operand recipe and why every stage is exact.
//
// Launch: `grid` workgroups x 256 lanes (4 waves). Straight-line, like
// mi355x_mfma_datapath_fp8: no inter-workgroup synchronisation and no waiting
// loop; where the workgroups land is reported (XCC id, HW_ID per wave), not
// arranged. Each wave runs eight stages of one MFMA each -- six
// v_mfma_scale_f32_32x32x64_f8f6f4 and two v_mfma_scale_f32_16x16x128_f8f6f4
// with e2m3, e3m2, e2m1 and (stage 6's A) e4m3 operands of 6, 4 and 8 dwords
// -- on operands generated and packed in registers, and compares its
// accumulator registers, as words, with a k-ordered VALU fmaf chain over the
// regenerated operands, decoded to f32 by integer arithmetic and scaled by
// exact powers of two (exact for these operands; no v_cvt of fp6 or fp4, which
// would be a second copy of the decoder under test). Wave 0's tiles also go to
// the host, which checks them word for word (datapath_f6f4_verify.h).
//
// 32x32: lane l holds fragment (row / column l&31, lane group l>>5; dpf6_k
// says which k its elements are) and the scale of scale block l>>5 in the
// selected byte of its scale VGPR;
// accumulator register r of lane l is D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
// 16x16: lane l holds fragment (row / column l&15, lane group l>>4);
// accumulator register r of lane l is D[4*(l>>4) + r][l&15].
#include <hip/hip_runtime.h>

#include "datapath_f6f4_kernel.h"

typedef int dpf6_i32x8 __attribute__((ext_vector_type(8)));

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPF6_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPF6_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))

// v[g] of a register array by a select chain (a dynamic index would go through scratch)
template <uint32_t N>
__device__ inline float dpf6_pick(const float (&v)[N], uint32_t g) {
  float x = v[0];
#pragma unroll
  for (uint32_t k = 1; k < N; ++k) x = g == k ? v[k] : x;
  return x;
}

// the non-MFMA value of D[row][col] of stage S: C, then one fmaf per k in k
// order over the regenerated codes of A's row and B's column, four k (one hash
// draw a side, one scale block) per trip; `sb`: the scales of the column's
// scale blocks. Rolled, so that the kernel stays in registers
template <uint32_t S, uint32_t kGroups>
__device__ inline uint32_t dpf6_want(uint32_t row, uint32_t col, uint32_t nw, const float (&sb)[kGroups]) {
  constexpr uint32_t kFa = dpf6_fmt(S, 0), kFb = dpf6_fmt(S, 1);
  float s = __uint_as_float(dpf6_c_word(S, row, col, nw));
  float sa[kGroups];  // the row's scales, per scale block
#pragma unroll
  for (uint32_t g = 0; g < kGroups; ++g) sa[g] = __uint_as_float(dpf6_scale_f32(dpf6_scale_byte(nw, S, 0, row, g)));
#pragma unroll 1
  for (uint32_t k0 = 0; k0 < kGroups * 32; k0 += 4) {
    const float xs = dpf6_pick(sa, k0 >> 5), ys = dpf6_pick(sb, k0 >> 5);
    const uint32_t ha = dpf6_group_of(S, kFa, k0), ea = dpf6_elem_of(S, kFa, k0);  // four k: one group, elements in a row
    const uint32_t hb = dpf6_group_of(S, kFb, k0), eb = dpf6_elem_of(S, kFb, k0);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const float x = __uint_as_float(dpf6_decode(dpf6_elem(S, 0, row, ha, ea + i, nw), kFa)) * xs;
      const float y = __uint_as_float(dpf6_decode(dpf6_elem(S, 1, col, hb, eb + i, nw), kFb)) * ys;
      s = __builtin_fmaf(x, y, s);
    }
  }
  return __float_as_uint(s);
}

// one stage of one wave: operands, the MFMA, the comparison, wave 0's tile
template <uint32_t S>
__device__ inline void dpf6_stage(const mi355x_datapath_f6f4_args& args, uint32_t wg, uint32_t nw, uint32_t lane,
                                  uint32_t wave, uint32_t* tiles, uint32_t* ctr) {
  constexpr uint32_t kDim = (S & 3) == 3 ? 16 : 32;
  constexpr uint32_t kGroups = kDim == 16 ? 4 : 2;
  constexpr uint32_t kRegs = kDim == 16 ? 4 : 16;
  typedef float acc_t __attribute__((ext_vector_type(kRegs)));
  const uint32_t col = lane & (kDim - 1);
  const uint32_t grp = lane / kDim;
  const auto row_of = [grp](uint32_t r) { return kDim == 16 ? 4 * grp + r : (r & 3) + 8 * (r >> 2) + 4 * grp; };

  dpf6_i32x8 a8, b8;  // the dwords beyond the format's own are zero (dpf6_word) and are not read
#pragma unroll
  for (uint32_t d = 0; d < 8; ++d) {
    a8[d] = static_cast<int>(dpf6_word(S, 0, col, grp, d, nw));
    b8[d] = static_cast<int>(dpf6_word(S, 1, col, grp, d, nw));
  }
  acc_t acc;
#pragma unroll
  for (uint32_t r = 0; r < kRegs; ++r) acc[r] = __uint_as_float(dpf6_c_word(S, row_of(r), col, nw));

  // cbsz / blgp: 2 = e2m3, 3 = e3m2, 4 = e2m1, 0 = e4m3; the scale VGPRs' selected bytes: S&3 for A, 3-(S&3) for B
  const int sa = static_cast<int>(dpf6_scale_word(nw, S, 0, col, grp));
  const int sb = static_cast<int>(dpf6_scale_word(nw, S, 1, col, grp));
  if constexpr (S == 0) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 2, 4, 0, sa, 3, sb);
  if constexpr (S == 1) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 3, 4, 1, sa, 2, sb);
  if constexpr (S == 2) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 4, 2, 2, sa, 1, sb);
  if constexpr (S == 3) acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, acc, 4, 3, 3, sa, 0, sb);
  if constexpr (S == 4) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 2, 2, 0, sa, 3, sb);
  if constexpr (S == 5) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 3, 4, 1, sa, 2, sb);
  if constexpr (S == 6) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 0, 4, 2, sa, 1, sb);
  if constexpr (S == 7) acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, acc, 4, 4, 3, sa, 0, sb);

  uint32_t got[kRegs];
#pragma unroll
  for (uint32_t r = 0; r < kRegs; ++r) got[r] = __float_as_uint(acc[r]);
#if defined(MI355X_TEST_INJECT)
  const bool hit = args.inject_kind == MI355X_DPF6_INJECT_MFMA && wg == args.inject_wg &&
                   wave == args.inject_wave && lane == args.inject_lane;
#pragma unroll
  for (uint32_t r = 0; r < kRegs; ++r)
    if (hit && S * 16 + r == args.inject_index) got[r] ^= args.inject_mask;
#endif
  float sbcol[kGroups];  // the scales of the scale blocks of column `col` of B
#pragma unroll
  for (uint32_t h = 0; h < kGroups; ++h) sbcol[h] = __uint_as_float(dpf6_scale_f32(dpf6_scale_byte(nw, S, 1, col, h)));
  uint32_t bad = 0;
  // one row per trip, the register picked by a select chain
#pragma unroll 1
  for (uint32_t r = 0; r < kRegs; ++r) {
    uint32_t g = got[0];
#pragma unroll
    for (uint32_t k = 1; k < kRegs; ++k) g = r == k ? got[k] : g;
    const uint32_t i = row_of(r);
    bad += g != dpf6_want<S>(i, col, nw, sbcol);
    if (wave == 0) tiles[dpf6_tile_offset(S) + i * kDim + col] = g;
  }
  if (bad) atomicAdd(&ctr[S], bad);
}

#define MI355X_DPF6_STAGE(S) dpf6_stage<S>(args, wg, nw, lane, wave, tiles, ctr)

extern "C" __global__ __launch_bounds__(MI355X_DPF6_THREADS) void mi355x_mfma_datapath_f6f4(
    mi355x_datapath_f6f4_args args) {
  __shared__ uint32_t ctr[12];  // 0..7 bad elements per stage, 8..11 HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid >> 6;
  const uint32_t lane = tid & 63;
  const uint32_t wg = blockIdx.x;
  if (wg >= args.grid) return;
  if (tid < 12) ctr[tid] = 0;
  __syncthreads();

  const uint32_t nw = dpf6_wave_nonce(args.nonce, wg, wave);
  uint32_t* tiles = args.tiles + static_cast<size_t>(wg) * MI355X_DPF6_WG_WORDS;
  MI355X_DPF6_STAGE(0);
  MI355X_DPF6_STAGE(1);
  MI355X_DPF6_STAGE(2);
  MI355X_DPF6_STAGE(3);
  MI355X_DPF6_STAGE(4);
  MI355X_DPF6_STAGE(5);
  MI355X_DPF6_STAGE(6);
  MI355X_DPF6_STAGE(7);
  if (lane == 0) ctr[8 + wave] = __builtin_amdgcn_s_getreg(MI355X_DPF6_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DPF6_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPF6REC_MAGIC) v = MI355X_DPF6_MAGIC;
    if (tid == MI355X_DPF6REC_WG) v = wg;
    if (tid == MI355X_DPF6REC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPF6REC_XCC) v = __builtin_amdgcn_s_getreg(MI355X_DPF6_HWREG_XCC_ID) & 0xF;
    if (tid >= MI355X_DPF6REC_HWID && tid < MI355X_DPF6REC_HWID + 4) v = ctr[8 + tid - MI355X_DPF6REC_HWID];
    if (tid >= MI355X_DPF6REC_BAD && tid < MI355X_DPF6REC_BAD + MI355X_DPF6_STAGES) v = ctr[tid - MI355X_DPF6REC_BAD];
    args.records[static_cast<size_t>(wg) * MI355X_DPF6_REC_WORDS + tid] = v;
  }
}
