// gfx950 (CDNA4) MXFP4 GEMM pipeline kernels: see datapath_mxgemm_kernel.h for
// the problem, the operand recipe, the LDS layout and the lane maps.
//
// mi355x_mxgemm_fill: `grid` workgroups x 256 lanes write A and sa (grid panels
// each), B and sb into device memory, 16 bytes a store, grid-strided.
//
// mi355x_mfma_datapath_mxgemm: `grid` workgroups x 256 lanes (4 waves, 2 x 2).
// No inter-workgroup synchronisation and no waiting loop; where the workgroups
// land is reported (XCC id, HW_ID per wave), not arranged. Per k-step of 256:
//   wait for the step's direct-to-LDS loads, barrier, issue the next step's
//   loads into the other buffer and the next step's scale loads into registers,
//   gather this step's scales (v_perm_b32), then four 64-wide sub-steps of two
//   A and two B fragments (ds_read_b128 each) and four
//   v_mfma_scale_f32_32x32x64_f8f6f4, each on the accumulator the previous
//   sub-step left, with op_sel = the sub-step on both scale operands.
// Accumulator register r of lane l of a 32x32 block is
// D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
#include <hip/hip_runtime.h>

#include "datapath_mxgemm_kernel.h"

typedef float dpmx_f32x16 __attribute__((ext_vector_type(16)));
typedef int dpmx_i32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t dpmx_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t dpmx_u32x4 __attribute__((ext_vector_type(4)));

#define MI355X_DPMX_GLOBAL(p) ((const __attribute__((address_space(1))) void*)(p))
#define MI355X_DPMX_LDS(p) ((__attribute__((address_space(3))) void*)(p))

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPMX_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPMX_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))
// s_waitcnt vmcnt(0): expcnt and lgkmcnt left at their maxima
#define MI355X_DPMX_WAIT_VM0 0x0F70

extern "C" __global__ __launch_bounds__(MI355X_DPMX_THREADS) void mi355x_mxgemm_fill(mi355x_datapath_mxgemm_args args) {
  const uint32_t wg = blockIdx.x;
  if (wg >= args.grid || args.ksteps == 0 || args.ksteps > MI355X_DPMX_KSTEPS_MAX) return;
  const uint32_t blocks = args.ksteps * 8u;                 // scale blocks = 16-byte operand chunks of a row
  const uint32_t a_chunks = args.grid * MI355X_DPMX_TILE * blocks, b_chunks = MI355X_DPMX_TILE * blocks;
  const uint32_t sa_chunks = a_chunks / 16u, sb_chunks = b_chunks / 16u;  // 16 scale bytes a chunk
  for (uint32_t c = wg * MI355X_DPMX_THREADS + threadIdx.x; c < a_chunks + b_chunks + sa_chunks + sb_chunks;
       c += args.grid * MI355X_DPMX_THREADS) {
    dpmx_u32x4 v;
    if (c < a_chunks + b_chunks) {
      const bool is_b = c >= a_chunks;
      const uint32_t cc = is_b ? c - a_chunks : c;
      const uint32_t panel = cc / (MI355X_DPMX_TILE * blocks), in_panel = cc % (MI355X_DPMX_TILE * blocks);
      const uint32_t row = in_panel / blocks, g = in_panel % blocks;
      const uint32_t seed = dpmx_wg_seed(args.nonce, panel);
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d)
        v[d] = is_b ? dpmx_b_dword(args.nonce, args.ksteps, row, 4u * g + d) : dpmx_a_dword(seed, args.ksteps, row, 4u * g + d);
#if defined(MI355X_TEST_INJECT)
      if (args.inject_kind == MI355X_DPMX_INJECT_HBM && !is_b && panel == args.inject_wg && in_panel == args.inject_index / 16u) {
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d)
          if (d == (args.inject_index & 15u) >> 2) v[d] ^= (args.inject_mask & 0xFFu) << (8u * (args.inject_index & 3u));
      }
#endif
      reinterpret_cast<dpmx_u32x4*>(is_b ? args.b : args.a)[cc] = v;
    } else {
      const bool is_b = c >= a_chunks + b_chunks + sa_chunks;
      const uint32_t cc = c - a_chunks - b_chunks - (is_b ? sa_chunks : 0u);
      const uint32_t per_panel = MI355X_DPMX_TILE * blocks;  // scale bytes of a panel
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
          const uint32_t f = cc * 16u + d * 4u + i;            // byte of the whole scale array
          const uint32_t panel = f / per_panel, in_panel = f % per_panel;
          const uint32_t seed = is_b ? args.nonce : dpmx_wg_seed(args.nonce, panel);
          w |= dpmx_scale_byte(seed, is_b ? 1u : 0u, in_panel / blocks, in_panel % blocks) << (8u * i);
        }
        v[d] = w;
      }
      reinterpret_cast<dpmx_u32x4*>(is_b ? args.sb : args.sa)[cc] = v;
    }
  }
}

// xor and sum of dwords, folded lane by lane
__device__ inline void dpmx_fold(uint32_t w, uint32_t& fx, uint32_t& fs) {
  fx ^= w;
  fs += w;
}

extern "C" __global__ __launch_bounds__(MI355X_DPMX_THREADS) void mi355x_mfma_datapath_mxgemm(
    mi355x_datapath_mxgemm_args args) {
  // One variable per buffer, and the loop written out for an even and an odd step: see mi355x_mfma_datapath_gemm.
  __shared__ __attribute__((aligned(1024))) unsigned char lds0[MI355X_DPMX_LDS_BYTES / 2];
  __shared__ __attribute__((aligned(1024))) unsigned char lds1[MI355X_DPMX_LDS_BYTES / 2];
  __shared__ uint32_t ctr[24 + 4];  // the folds as in the record, then HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lane = tid & 63u;
  const uint32_t wg = blockIdx.x;
  const uint32_t ksteps = args.ksteps;
  if (wg >= args.grid || ksteps == 0 || ksteps > MI355X_DPMX_KSTEPS_MAX) return;  // the operands are sized by ksteps
  if (tid < 24 + 4) ctr[tid] = 0;  // the first step's barrier comes before any use

  const uint32_t row_bytes = ksteps * (MI355X_DPMX_KSTEP / 2u);  // K/2
  const unsigned char* ag = args.a + static_cast<size_t>(wg) * MI355X_DPMX_TILE * row_bytes;
  const unsigned char* bg = args.b;

  // Global byte offsets of this lane's 16 bytes in the wave's four wave-loads of a step of either tile. Wave-load w
  // fills LDS bytes [1024 w, 1024 w + 1024) of the tile, lane l the 16 at 16 l: rows 8w..8w+7. Which global chunk
  // lands there is the swizzle (dpmx_lds, inverted).
  uint32_t ld_off[4];
#pragma unroll
  for (uint32_t t = 0; t < 4; ++t) {
    const uint32_t row = 8u * (wave * 4u + t) + (lane >> 3), kc = (lane & 7u) ^ ((row >> 1) & 7u);
    ld_off[t] = row * row_bytes + kc * 16u;
  }
  const auto issue_loads = [&](unsigned char* lds, uint32_t s) {
    unsigned char* buf = lds + wave * 4096u;
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) {
      __builtin_amdgcn_global_load_lds(MI355X_DPMX_GLOBAL(ag + ld_off[t] + s * 128u), MI355X_DPMX_LDS(buf + t * 1024u), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(MI355X_DPMX_GLOBAL(bg + ld_off[t] + s * 128u),
                                       MI355X_DPMX_LDS(buf + MI355X_DPMX_LDS_TILE_BYTES + t * 1024u), 16, 0, 0);
    }
  };

  // the wave's sub-tile and this lane's place in its fragments
  const uint32_t row0 = 64u * (wave >> 1), col0 = 64u * (wave & 1u);
  const uint32_t hi = lane >> 5;                       // lane group: k 32*hi.. of a 64-wide sub-step
  const uint32_t a_row = row0 + (lane & 31u);          // + 32 * rb
  const uint32_t b_col = col0 + (lane & 31u);          // + 32 * cb
  const uint32_t a_swz = (a_row >> 1) & 7u, b_swz = (b_col >> 1) & 7u;  // the same for both blocks

  // this lane's scale bytes: 8 a step of each of its two rows and two columns
  const unsigned char* sag = args.sa + static_cast<size_t>(wg) * MI355X_DPMX_TILE * (ksteps * 8u);
  const dpmx_u32x2* sp[4];
#pragma unroll
  for (uint32_t t = 0; t < 2; ++t) {
    sp[t] = reinterpret_cast<const dpmx_u32x2*>(sag + (a_row + 32u * t) * (ksteps * 8u));
    sp[2 + t] = reinterpret_cast<const dpmx_u32x2*>(args.sb + (b_col + 32u * t) * (ksteps * 8u));
  }
  const uint32_t perm_sel = hi ? 0x07050301u : 0x06040200u;
  dpmx_u32x2 raw[4];
#pragma unroll
  for (uint32_t t = 0; t < 4; ++t) raw[t] = sp[t][0];

  const uint32_t seed = dpmx_wg_seed(args.nonce, wg);
  dpmx_f32x16 acc[2][2];
#pragma unroll
  for (uint32_t rb = 0; rb < 2; ++rb)
#pragma unroll
    for (uint32_t cb = 0; cb < 2; ++cb)
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r)
        acc[rb][cb][r] = __uint_as_float(dpmx_c_word(seed, args.nonce, row0 + 32u * rb + (r & 3u) + 8u * (r >> 2) + 4u * hi,
                                                     col0 + 32u * cb + (lane & 31u)));

  uint32_t fax = 0, fas = 0, fbx = 0, fbs = 0, fsx = 0, fss = 0;
  // one k-step: reads `cur`, which the loads of step s filled, while the loads of step s + 1 fill `nxt`
  const auto step = [&](unsigned char* cur, unsigned char* nxt, uint32_t s) {
    __builtin_amdgcn_s_waitcnt(MI355X_DPMX_WAIT_VM0);  // this wave's loads of step s have landed
    __syncthreads();                                   // and everyone's; everyone has read the other buffer
    uint32_t sc[4];                                    // the gathered scales: A's row blocks, then B's column blocks
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) sc[t] = __builtin_amdgcn_perm(raw[t][1], raw[t][0], perm_sel);
    if (s + 1u < ksteps) {
      issue_loads(nxt, s + 1u);
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t) raw[t] = sp[t][s + 1u];
    }
#if defined(MI355X_TEST_INJECT)
    if (args.inject_kind == MI355X_DPMX_INJECT_LDS && wg == args.inject_wg && s == args.inject_wave) {
      if (tid == 0) reinterpret_cast<uint32_t*>(cur)[args.inject_index & (MI355X_DPMX_LDS_BYTES / 8u - 1u)] ^= args.inject_mask;
      __syncthreads();
    }
#endif
    const unsigned char* at = cur;
    const unsigned char* bt = at + MI355X_DPMX_LDS_TILE_BYTES;
#pragma unroll
    for (uint32_t kk = 0; kk < 4; ++kk) {
#if defined(MI355X_TEST_INJECT)
      if (args.inject_kind == MI355X_DPMX_INJECT_SCALE && wg == args.inject_wg && wave == args.inject_wave &&
          lane == args.inject_lane && s * 16u + kk * 4u == (args.inject_index & ~3u)) {
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t)
          if (t == (args.inject_index & 3u)) sc[t] ^= args.inject_mask;
      }
#endif
      dpmx_i32x8 af[2], bf[2];
#pragma unroll
      for (uint32_t t = 0; t < 2; ++t) {
        const dpmx_u32x4 a4 =
            *reinterpret_cast<const dpmx_u32x4*>(at + (a_row + 32u * t) * 128u + (((2u * kk + hi) ^ a_swz) << 4));
        const dpmx_u32x4 b4 =
            *reinterpret_cast<const dpmx_u32x4*>(bt + (b_col + 32u * t) * 128u + (((2u * kk + hi) ^ b_swz) << 4));
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
          dpmx_fold(a4[d], fax, fas);
          dpmx_fold(b4[d], fbx, fbs);
          af[t][d] = static_cast<int>(a4[d]);
          bf[t][d] = static_cast<int>(b4[d]);
          af[t][4 + d] = 0;  // e2m1 fragments are four dwords: the instruction does not read these
          bf[t][4 + d] = 0;
        }
      }
#pragma unroll
      for (uint32_t rb = 0; rb < 2; ++rb)
#pragma unroll
        for (uint32_t cb = 0; cb < 2; ++cb) {
          const int sa = static_cast<int>(sc[rb]), sb = static_cast<int>(sc[2 + cb]);
          // cbsz = blgp = 4: e2m1; op_sel = kk: byte kk of both scale VGPRs
          if (kk == 0) acc[rb][cb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[rb], bf[cb], acc[rb][cb], 4, 4, 0, sa, 0, sb);
          if (kk == 1) acc[rb][cb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[rb], bf[cb], acc[rb][cb], 4, 4, 1, sa, 1, sb);
          if (kk == 2) acc[rb][cb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[rb], bf[cb], acc[rb][cb], 4, 4, 2, sa, 2, sb);
          if (kk == 3) acc[rb][cb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[rb], bf[cb], acc[rb][cb], 4, 4, 3, sa, 3, sb);
        }
    }
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) dpmx_fold(sc[t], fsx, fss);  // as fed
  };
  issue_loads(lds0, 0);
#pragma unroll 1
  for (uint32_t s = 0; s < ksteps; s += 2u) {
    step(lds0, lds1, s);
    if (s + 1u >= ksteps) break;
    step(lds1, lds0, s + 1u);
  }

  uint32_t* tile = args.tiles + static_cast<size_t>(wg) * MI355X_DPMX_WG_WORDS;
#pragma unroll
  for (uint32_t rb = 0; rb < 2; ++rb)
#pragma unroll
    for (uint32_t cb = 0; cb < 2; ++cb)
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r) {
        uint32_t word = __float_as_uint(acc[rb][cb][r]);
#if defined(MI355X_TEST_INJECT)
        if (args.inject_kind == MI355X_DPMX_INJECT_MFMA && wg == args.inject_wg && wave == args.inject_wave &&
            lane == args.inject_lane && (rb * 2u + cb) * 16u + r == args.inject_index)
          word ^= args.inject_mask;
#endif
        tile[(row0 + 32u * rb + (r & 3u) + 8u * (r >> 2) + 4u * hi) * MI355X_DPMX_TILE + col0 + 32u * cb + (lane & 31u)] = word;
      }

  atomicXor(&ctr[wave * 6u + 0u], fax);
  atomicAdd(&ctr[wave * 6u + 1u], fas);
  atomicXor(&ctr[wave * 6u + 2u], fbx);
  atomicAdd(&ctr[wave * 6u + 3u], fbs);
  atomicXor(&ctr[wave * 6u + 4u], fsx);
  atomicAdd(&ctr[wave * 6u + 5u], fss);
  if (lane == 0) ctr[24u + wave] = __builtin_amdgcn_s_getreg(MI355X_DPMX_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DPMX_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPMXREC_MAGIC) v = MI355X_DPMX_MAGIC;
    if (tid == MI355X_DPMXREC_WG) v = wg;
    if (tid == MI355X_DPMXREC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPMXREC_XCC) v = (__builtin_amdgcn_s_getreg(MI355X_DPMX_HWREG_XCC_ID) & 0xF) | (ksteps << 8);
    if (tid >= MI355X_DPMXREC_HWID && tid < MI355X_DPMXREC_HWID + 4) v = ctr[24u + tid - MI355X_DPMXREC_HWID];
    if (tid >= MI355X_DPMXREC_FOLD) v = ctr[tid - MI355X_DPMXREC_FOLD];
    args.records[static_cast<size_t>(wg) * MI355X_DPMX_REC_WORDS + tid] = v;
  }
}
