// gfx950 (CDNA4) MFMA datapath kernel: see datapath_kernel.h for the operand
// recipe and why every stage is exact.
//
// Launch: `grid` workgroups x 256 lanes (4 waves). Straight-line: no
// inter-workgroup synchronisation and no waiting loop, so the grid drains
// behind whatever else runs on the GPU; where the workgroups land is reported
// (XCC id, HW_ID per wave), not arranged. Each wave runs four stages of one
// v_mfma_f32_32x32x2_f32 on operands generated in registers and compares its
// 16 accumulator registers, as bit patterns, with a VALU fmaf chain in k
// order (the instruction's documented numerics). Wave 0's tiles also go to
// the host, which checks them bit for bit (datapath_verify.h).
//
// Lane l holds A[l&31][l>>5] and B[l>>5][l&31]; accumulator register r of
// lane l is D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
#include <hip/hip_runtime.h>

#include "datapath_kernel.h"

typedef float dp_f32x16 __attribute__((ext_vector_type(16)));

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DP_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DP_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))

extern "C" __global__ __launch_bounds__(MI355X_DP_THREADS) void mi355x_mfma_datapath(mi355x_datapath_args args) {
  __shared__ uint32_t ctr[8];  // 0..3 bad elements per stage, 4..7 HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid >> 6;
  const uint32_t lane = tid & 63;
  const uint32_t wg = blockIdx.x;
  if (wg >= args.grid) return;
  if (tid < 8) ctr[tid] = 0;
  __syncthreads();

  const uint32_t nw = dp_wave_nonce(args.nonce, wg, wave);
  const uint32_t col = lane & 31;
  const uint32_t kk = lane >> 5;
  uint32_t* tiles = args.tiles + static_cast<size_t>(wg) * MI355X_DP_WG_WORDS;
#pragma unroll
  for (uint32_t stage = 0; stage < MI355X_DP_STAGES; ++stage) {
    const float a = dp_as_float(dp_a_word(stage, col, kk, nw));
    const float b = dp_as_float(dp_b_word(stage, kk, col, nw));
    const float b0 = dp_as_float(dp_b_word(stage, 0, col, nw));
    const float b1 = dp_as_float(dp_b_word(stage, 1, col, nw));
    dp_f32x16 acc;
#pragma unroll
    for (uint32_t r = 0; r < 16; ++r) acc[r] = dp_as_float(dp_c_word(stage, (r & 3) + 8 * (r >> 2) + 4 * kk, col, nw));
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
#if defined(MI355X_TEST_INJECT)
    {
      const bool hit = args.inject_kind == MI355X_DP_INJECT_MFMA && wg == args.inject_wg &&
                       wave == args.inject_wave && lane == args.inject_lane;
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r)
        if (hit && stage * 16 + r == args.inject_index) acc[r] = dp_as_float(dp_as_word(acc[r]) ^ args.inject_mask);
    }
#endif
    uint32_t bad = 0;
#pragma unroll
    for (uint32_t r = 0; r < 16; ++r) {
      const uint32_t i = (r & 3) + 8 * (r >> 2) + 4 * kk;
      const float c = dp_as_float(dp_c_word(stage, i, col, nw));
      const float want = __builtin_fmaf(dp_as_float(dp_a_word(stage, i, 1, nw)), b1,
                                        __builtin_fmaf(dp_as_float(dp_a_word(stage, i, 0, nw)), b0, c));
      const uint32_t got = dp_as_word(acc[r]);
      bad += got != dp_as_word(want);
      if (wave == 0) tiles[(stage * MI355X_DP_M + i) * MI355X_DP_N + col] = got;
    }
    if (bad) atomicAdd(&ctr[stage], bad);
  }
  if (lane == 0) ctr[4 + wave] = __builtin_amdgcn_s_getreg(MI355X_DP_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DP_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPREC_MAGIC) v = MI355X_DP_MAGIC;
    if (tid == MI355X_DPREC_WG) v = wg;
    if (tid == MI355X_DPREC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPREC_XCC) v = __builtin_amdgcn_s_getreg(MI355X_DP_HWREG_XCC_ID) & 0xF;
    if (tid >= MI355X_DPREC_HWID && tid < MI355X_DPREC_HWID + 4) v = ctr[4 + tid - MI355X_DPREC_HWID];
    if (tid >= MI355X_DPREC_BAD && tid < MI355X_DPREC_BAD + 4) v = ctr[tid - MI355X_DPREC_BAD];
    args.records[static_cast<size_t>(wg) * MI355X_DP_REC_WORDS + tid] = v;
  }
}
