// gfx950 (CDNA4) sparse (2:4) MFMA datapath kernel: see
// datapath_sparse_kernel.h for the operand recipe, the measured index / K /
// abid rules and why every stage is exact.
//
// Launch: `grid` workgroups x 256 lanes (4 waves). Straight-line, like
// mi355x_mfma_datapath_f16: no inter-workgroup synchronisation and no waiting
// loop; where the workgroups land is reported (XCC id, HW_ID per wave), not
// arranged. Each wave runs ten stages of one v_smfmac_* each -- f16, bf16, int8
// and fp8 x bf8 data, 32x32 and 16x16 tiles -- on a compressed A, an index
// register and a dense B generated in registers, and compares its accumulator
// registers, as words, with dpsp_expected: a VALU fmaf chain (integer
// arithmetic for int8) over the compressed elements of A's row, each times the
// element of B's column that the same index word names. Wave 0's tiles also go
// to the host, which checks them word for word (datapath_sparse_verify.h).
//
// 32x32: lane l holds the fragments of (row / column l&31, lane group l>>5);
// accumulator register r of lane l is D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
// 16x16: lane l holds (row / column l&15, lane group l>>4); accumulator
// register r of lane l is D[4*(l>>4) + r][l&15].
#include <hip/hip_runtime.h>

#include "datapath_sparse_kernel.h"

typedef int dpsp_i32x4 __attribute__((ext_vector_type(4)));
typedef int dpsp_i32x8 __attribute__((ext_vector_type(8)));
typedef _Float16 dpsp_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 dpsp_f16x16 __attribute__((ext_vector_type(16)));
typedef __bf16 dpsp_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 dpsp_bf16x16 __attribute__((ext_vector_type(16)));

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPSP_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPSP_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))

// one stage of one wave: operands and index, the sparse MFMA, the comparison, wave 0's tile
template <uint32_t S>
__device__ inline void dpsp_stage(const mi355x_datapath_sparse_args& args, uint32_t wg, uint32_t nw, uint32_t lane,
                                  uint32_t wave, uint32_t* tiles, uint32_t* ctr) {
  constexpr uint32_t kDim = (S == 4 || S == 6 || S == 8) ? 16 : 32;
  constexpr uint32_t kRegs = kDim == 16 ? 4 : 16;
  constexpr bool kInt = S == 7 || S == 8;
  typedef float facc_t __attribute__((ext_vector_type(kRegs)));
  typedef int iacc_t __attribute__((ext_vector_type(kRegs)));
  const uint32_t col = lane & (kDim - 1);
  const uint32_t grp = lane / kDim;
  const auto row_of = [grp](uint32_t r) { return kDim == 16 ? 4 * grp + r : (r & 3) + 8 * (r >> 2) + 4 * grp; };

  dpsp_i32x4 a4;
  dpsp_i32x8 b8;
#pragma unroll
  for (uint32_t d = 0; d < 4; ++d) a4[d] = static_cast<int>(dpsp_a_word(S, col, grp, d, nw));
#pragma unroll
  for (uint32_t d = 0; d < 8; ++d) b8[d] = static_cast<int>(dpsp_b_word(S, col, grp, d, nw));
  const int idx = static_cast<int>(dpsp_index_word(S, col, grp, nw));

  uint32_t got[kRegs];
  if constexpr (kInt) {
    iacc_t acc;
#pragma unroll
    for (uint32_t r = 0; r < kRegs; ++r) acc[r] = static_cast<int>(dpsp_c_word(S, row_of(r), col, nw));
    if constexpr (S == 7) acc = __builtin_amdgcn_smfmac_i32_32x32x64_i8(a4, b8, acc, idx, 0, 0);
    if constexpr (S == 8) acc = __builtin_amdgcn_smfmac_i32_16x16x128_i8(a4, b8, acc, idx, 0, 0);
#pragma unroll
    for (uint32_t r = 0; r < kRegs; ++r) got[r] = static_cast<uint32_t>(acc[r]);
  } else {
    facc_t acc;
#pragma unroll
    for (uint32_t r = 0; r < kRegs; ++r) acc[r] = __uint_as_float(dpsp_c_word(S, row_of(r), col, nw));
    const dpsp_f16x8 ah = __builtin_bit_cast(dpsp_f16x8, a4);
    const dpsp_f16x16 bh = __builtin_bit_cast(dpsp_f16x16, b8);
    const dpsp_bf16x8 ab = __builtin_bit_cast(dpsp_bf16x8, a4);
    const dpsp_bf16x16 bb = __builtin_bit_cast(dpsp_bf16x16, b8);
    // (A, B, C, index, cbsz, abid): cbsz stays 0; stage 2 reads idx[31:16]
    if constexpr (S == 0 || S == 1 || S == 3) acc = __builtin_amdgcn_smfmac_f32_32x32x32_f16(ah, bh, acc, idx, 0, 0);
    if constexpr (S == 2) acc = __builtin_amdgcn_smfmac_f32_32x32x32_f16(ah, bh, acc, idx, 0, 1);
    if constexpr (S == 4) acc = __builtin_amdgcn_smfmac_f32_16x16x64_f16(ah, bh, acc, idx, 0, 0);
    if constexpr (S == 5) acc = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(ab, bb, acc, idx, 0, 0);
    if constexpr (S == 6) acc = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(ab, bb, acc, idx, 0, 0);
    if constexpr (S == 9) acc = __builtin_amdgcn_smfmac_f32_32x32x64_fp8_bf8(a4, b8, acc, idx, 0, 0);
#pragma unroll
    for (uint32_t r = 0; r < kRegs; ++r) got[r] = __float_as_uint(acc[r]);
  }
#if defined(MI355X_TEST_INJECT)
  const bool hit = args.inject_kind == MI355X_DPSP_INJECT_MFMA && wg == args.inject_wg &&
                   wave == args.inject_wave && lane == args.inject_lane;
#pragma unroll
  for (uint32_t r = 0; r < kRegs; ++r)
    if (hit && S * 16 + r == args.inject_index) got[r] ^= args.inject_mask;
#endif
  uint32_t bad = 0;
  // one row per trip, the register picked by a select chain
#pragma unroll 1
  for (uint32_t r = 0; r < kRegs; ++r) {
    uint32_t g = got[0];
#pragma unroll
    for (uint32_t k = 1; k < kRegs; ++k) g = r == k ? got[k] : g;
    const uint32_t i = row_of(r);
    bad += g != dpsp_expected(S, i, col, nw);
    if (wave == 0) tiles[dpsp_tile_offset(S) + i * kDim + col] = g;
  }
  if (bad) atomicAdd(&ctr[S], bad);
}

#define MI355X_DPSP_STAGE(S) dpsp_stage<S>(args, wg, nw, lane, wave, tiles, ctr)

extern "C" __global__ __launch_bounds__(MI355X_DPSP_THREADS) void mi355x_mfma_datapath_sparse(
    mi355x_datapath_sparse_args args) {
  __shared__ uint32_t ctr[MI355X_DPSP_STAGES + 4];  // bad elements per stage, then HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = tid >> 6;
  const uint32_t lane = tid & 63;
  const uint32_t wg = blockIdx.x;
  if (wg >= args.grid) return;
  if (tid < MI355X_DPSP_STAGES + 4) ctr[tid] = 0;
  __syncthreads();

  const uint32_t nw = dpsp_wave_nonce(args.nonce, wg, wave);
  uint32_t* tiles = args.tiles + static_cast<size_t>(wg) * MI355X_DPSP_WG_WORDS;
  MI355X_DPSP_STAGE(0);
  MI355X_DPSP_STAGE(1);
  MI355X_DPSP_STAGE(2);
  MI355X_DPSP_STAGE(3);
  MI355X_DPSP_STAGE(4);
  MI355X_DPSP_STAGE(5);
  MI355X_DPSP_STAGE(6);
  MI355X_DPSP_STAGE(7);
  MI355X_DPSP_STAGE(8);
  MI355X_DPSP_STAGE(9);
  if (lane == 0) ctr[MI355X_DPSP_STAGES + wave] = __builtin_amdgcn_s_getreg(MI355X_DPSP_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DPSP_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPSPREC_MAGIC) v = MI355X_DPSP_MAGIC;
    if (tid == MI355X_DPSPREC_WG) v = wg;
    if (tid == MI355X_DPSPREC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPSPREC_XCC) v = __builtin_amdgcn_s_getreg(MI355X_DPSP_HWREG_XCC_ID) & 0xF;
    if (tid >= MI355X_DPSPREC_HWID && tid < MI355X_DPSPREC_HWID + 4)
      v = ctr[MI355X_DPSP_STAGES + tid - MI355X_DPSPREC_HWID];
    if (tid >= MI355X_DPSPREC_BAD && tid < MI355X_DPSPREC_BAD + MI355X_DPSP_STAGES) v = ctr[tid - MI355X_DPSPREC_BAD];
    args.records[static_cast<size_t>(wg) * MI355X_DPSP_REC_WORDS + tid] = v;
  }
}
