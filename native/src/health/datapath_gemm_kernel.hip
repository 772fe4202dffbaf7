// gfx950 (CDNA4) bf16 GEMM pipeline kernels: see datapath_gemm_kernel.h for the
// problem, the operand recipe, the LDS layout and the lane maps.
//
// mi355x_gemm_fill: `grid` workgroups x 256 lanes write A (grid panels) and B
// into device memory, 16 bytes a store, grid-strided.
//
// mi355x_mfma_datapath_gemm: `grid` workgroups x 256 lanes (4 waves, 2 x 2).
// No inter-workgroup synchronisation and no waiting loop; where the workgroups
// land is reported (XCC id, HW_ID per wave), not arranged. Per k-step of 64:
//   wait for the step's direct-to-LDS loads, barrier, issue the next step's
//   loads into the other buffer, then four 16-wide sub-steps of two A fragments
//   (ds_read_b128), two B fragments (two ds_read_b64_tr_b16 each) and four
//   v_mfma_f32_32x32x16_bf16, each on the accumulator the previous sub-step left.
// Accumulator register r of lane l of a 32x32 block is
// D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
#include <hip/hip_runtime.h>

#include "datapath_gemm_kernel.h"

typedef float dpgm_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 dpgm_bf16x8 __attribute__((ext_vector_type(8)));
typedef short dpgm_i16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t dpgm_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t dpgm_u32x4 __attribute__((ext_vector_type(4)));

#define MI355X_DPGM_GLOBAL(p) ((const __attribute__((address_space(1))) void*)(p))
#define MI355X_DPGM_LDS(p) ((__attribute__((address_space(3))) void*)(p))

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPGM_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPGM_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))
// s_waitcnt vmcnt(0): expcnt and lgkmcnt left at their maxima
#define MI355X_DPGM_WAIT_VM0 0x0F70

extern "C" __global__ __launch_bounds__(MI355X_DPGM_THREADS) void mi355x_gemm_fill(mi355x_datapath_gemm_args args) {
  const uint32_t wg = blockIdx.x;
  if (wg >= args.grid) return;
  const uint32_t K = args.ksteps * MI355X_DPGM_KSTEP;
  const uint32_t a_chunks = args.grid * MI355X_DPGM_TILE * (K / 8u);  // 16-byte chunks of 8 elements
  const uint32_t b_chunks = K * (MI355X_DPGM_TILE / 8u);
  for (uint32_t c = wg * MI355X_DPGM_THREADS + threadIdx.x; c < a_chunks + b_chunks;
       c += args.grid * MI355X_DPGM_THREADS) {
    dpgm_u32x4 v;
    if (c < a_chunks) {
      const uint32_t panel = c / (MI355X_DPGM_TILE * (K / 8u));
      const uint32_t in_panel = c - panel * (MI355X_DPGM_TILE * (K / 8u));
      const uint32_t row = in_panel / (K / 8u), k = (in_panel % (K / 8u)) * 8u;
      const uint32_t seed = dpgm_wg_seed(args.nonce, panel);
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) v[d] = dpgm_a_dword(seed, args.ksteps, row, k + 2u * d);
#if defined(MI355X_TEST_INJECT)
      if (args.inject_kind == MI355X_DPGM_INJECT_HBM && panel == args.inject_wg && in_panel == args.inject_index / 8u) {
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d)
          if (d == (args.inject_index & 7u) >> 1) v[d] ^= (args.inject_mask & 0xFFFFu) << (16u * (args.inject_index & 1u));
      }
#endif
      reinterpret_cast<dpgm_u32x4*>(args.a)[c] = v;
    } else {
      const uint32_t cb = c - a_chunks;
      const uint32_t k = cb / (MI355X_DPGM_TILE / 8u), col = (cb % (MI355X_DPGM_TILE / 8u)) * 8u;
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d)
        v[d] = dpgm_b_elem(args.nonce, k, col + 2u * d) | (dpgm_b_elem(args.nonce, k, col + 2u * d + 1u) << 16);
      reinterpret_cast<dpgm_u32x4*>(args.b)[cb] = v;
    }
  }
}

// xor and sum of the 16-bit elements of a fragment's dwords, folded lane by lane
__device__ inline void dpgm_fold(uint32_t w, uint32_t& fx, uint32_t& fs) {
  fx ^= w;
  fs += (w & 0xFFFFu) + (w >> 16);
}

extern "C" __global__ __launch_bounds__(MI355X_DPGM_THREADS) void mi355x_mfma_datapath_gemm(
    mi355x_datapath_gemm_args args) {
  // One variable per buffer: the compiler waits for a direct-to-LDS load before an LDS read only where the two may
  // alias, and it tells buffers apart as variables, not as halves of one. So the loop below is written out for an
  // even and an odd step, and the reads of one buffer do not wait for the loads in flight into the other.
  __shared__ __attribute__((aligned(1024))) unsigned char lds0[MI355X_DPGM_LDS_BYTES / 2];
  __shared__ __attribute__((aligned(1024))) unsigned char lds1[MI355X_DPGM_LDS_BYTES / 2];
  __shared__ uint32_t ctr[16 + 4];  // the folds as in the record, then HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lane = tid & 63u;
  const uint32_t wg = blockIdx.x;
  const uint32_t ksteps = args.ksteps;
  if (wg >= args.grid || ksteps == 0 || ksteps > MI355X_DPGM_KSTEPS_MAX) return;  // the operands are sized by ksteps
  if (tid < 16 + 4) ctr[tid] = 0;  // the first step's barrier comes before any use

  const uint32_t K = ksteps * MI355X_DPGM_KSTEP;
  const unsigned char* ag = reinterpret_cast<const unsigned char*>(args.a) +
                            static_cast<size_t>(wg) * MI355X_DPGM_TILE * K * sizeof(uint16_t);
  const unsigned char* bg = reinterpret_cast<const unsigned char*>(args.b);

  // Global byte offsets of this lane's 16 bytes in the wave's four A and four B
  // wave-loads of a step. Wave-load w fills LDS bytes [1024 w, 1024 w + 1024) of
  // the tile, lane l the 16 at 16 l: A rows 8w..8w+7, B rows 4w..4w+3. Which
  // global chunk lands there is the swizzle (dpgm_lds_a / dpgm_lds_b, inverted).
  uint32_t a_off[4], b_off[4];
#pragma unroll
  for (uint32_t t = 0; t < 4; ++t) {
    const uint32_t w = wave * 4u + t;
    const uint32_t row = 8u * w + (lane >> 3), kc = (lane & 7u) ^ ((row >> 1) & 7u);
    a_off[t] = row * K * 2u + kc * 16u;
    const uint32_t k = 4u * w + (lane >> 4), nc = (lane & 15u) ^ ((k & 3u) << 2);
    b_off[t] = k * 256u + nc * 16u;
  }
  const auto issue_loads = [&](unsigned char* lds, uint32_t s) {
    unsigned char* buf = lds + wave * 4096u;
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) {
      __builtin_amdgcn_global_load_lds(MI355X_DPGM_GLOBAL(ag + a_off[t] + s * 128u), MI355X_DPGM_LDS(buf + t * 1024u),
                                       16, 0, 0);
      __builtin_amdgcn_global_load_lds(MI355X_DPGM_GLOBAL(bg + b_off[t] + s * (MI355X_DPGM_KSTEP * 256u)),
                                       MI355X_DPGM_LDS(buf + MI355X_DPGM_LDS_TILE_BYTES + t * 1024u), 16, 0, 0);
    }
  };

  // the wave's sub-tile and this lane's place in its fragments
  const uint32_t row0 = 64u * (wave >> 1), col0 = 64u * (wave & 1u);
  const uint32_t hi = lane >> 5;                       // lane group: k 8*hi.. of a 16-wide sub-step
  const uint32_t a_row = row0 + (lane & 31u);          // + 32 * rb
  const uint32_t a_swz = (a_row >> 1) & 7u;            // the same for both row blocks
  // B, transposed read: this lane addresses row (k) 8*hi + 4*h + ((lane&15)>>2), columns 4*(lane&3).. of the
  // 16-column half (lane>>4)&1 of column block cb
  const uint32_t b_k = 8u * hi + ((lane & 15u) >> 2);  // + 16 * kk + 4 * h
  const uint32_t b_n = col0 + 16u * ((lane >> 4) & 1u) + 4u * (lane & 3u);  // + 32 * cb

  const uint32_t seed = dpgm_wg_seed(args.nonce, wg);
  dpgm_f32x16 acc[2][2];
#pragma unroll
  for (uint32_t rb = 0; rb < 2; ++rb)
#pragma unroll
    for (uint32_t cb = 0; cb < 2; ++cb)
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r)
        acc[rb][cb][r] = __uint_as_float(dpgm_c_word(seed, args.nonce, row0 + 32u * rb + (r & 3u) + 8u * (r >> 2) + 4u * hi,
                                                     col0 + 32u * cb + (lane & 31u)));

  uint32_t fax = 0, fas = 0, fbx = 0, fbs = 0;
  // one k-step: reads `cur`, which the loads of step s filled, while the loads of step s + 1 fill `nxt`
  const auto step = [&](unsigned char* cur, unsigned char* nxt, uint32_t s) {
    __builtin_amdgcn_s_waitcnt(MI355X_DPGM_WAIT_VM0);  // this wave's loads of step s have landed
    __syncthreads();                                   // and everyone's; everyone has read the other buffer
    if (s + 1u < ksteps) issue_loads(nxt, s + 1u);
#if defined(MI355X_TEST_INJECT)
    if (args.inject_kind == MI355X_DPGM_INJECT_LDS && wg == args.inject_wg && s == args.inject_wave) {
      if (tid == 0) reinterpret_cast<uint32_t*>(cur)[args.inject_index & (MI355X_DPGM_LDS_BYTES / 8u - 1u)] ^= args.inject_mask;
      __syncthreads();
    }
#endif
    const unsigned char* at = cur;
    const unsigned char* bt = at + MI355X_DPGM_LDS_TILE_BYTES;
    #pragma unroll
    for (uint32_t kk = 0; kk < 4; ++kk) {
      dpgm_u32x4 af[2], bf[2];
#pragma unroll
      for (uint32_t rb = 0; rb < 2; ++rb) {
        af[rb] = *reinterpret_cast<const dpgm_u32x4*>(at + (a_row + 32u * rb) * 128u + (((2u * kk + hi) ^ a_swz) << 4));
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) dpgm_fold(af[rb][d], fax, fas);
      }
#pragma unroll
      for (uint32_t cb = 0; cb < 2; ++cb) {
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
          const uint32_t k = 16u * kk + 4u * h + b_k, n = b_n + 32u * cb;
          const unsigned char* p = bt + k * 256u + (((n >> 3) ^ ((k & 3u) << 2)) << 4) + (n & 7u) * 2u;
          const dpgm_i16x4 q = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) dpgm_i16x4*)(p));
          const dpgm_u32x2 w = __builtin_bit_cast(dpgm_u32x2, q);
          bf[cb][2u * h] = w[0];
          bf[cb][2u * h + 1u] = w[1];
        }
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) dpgm_fold(bf[cb][d], fbx, fbs);
      }
#pragma unroll
      for (uint32_t rb = 0; rb < 2; ++rb)
#pragma unroll
        for (uint32_t cb = 0; cb < 2; ++cb)
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(dpgm_bf16x8, af[rb]),
                                                                __builtin_bit_cast(dpgm_bf16x8, bf[cb]), acc[rb][cb], 0, 0, 0);
    }
  };
  issue_loads(lds0, 0);
#pragma unroll 1
  for (uint32_t s = 0; s < ksteps; s += 2u) {
    step(lds0, lds1, s);
    if (s + 1u >= ksteps) break;
    step(lds1, lds0, s + 1u);
  }

  uint32_t* tile = args.tiles + static_cast<size_t>(wg) * MI355X_DPGM_WG_WORDS;
#pragma unroll
  for (uint32_t rb = 0; rb < 2; ++rb)
#pragma unroll
    for (uint32_t cb = 0; cb < 2; ++cb)
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r) {
        uint32_t word = __float_as_uint(acc[rb][cb][r]);
#if defined(MI355X_TEST_INJECT)
        if (args.inject_kind == MI355X_DPGM_INJECT_MFMA && wg == args.inject_wg && wave == args.inject_wave &&
            lane == args.inject_lane && (rb * 2u + cb) * 16u + r == args.inject_index)
          word ^= args.inject_mask;
#endif
        tile[(row0 + 32u * rb + (r & 3u) + 8u * (r >> 2) + 4u * hi) * MI355X_DPGM_TILE + col0 + 32u * cb + (lane & 31u)] = word;
      }

  atomicXor(&ctr[wave * 4u + 0u], (fax ^ (fax >> 16)) & 0xFFFFu);
  atomicAdd(&ctr[wave * 4u + 1u], fas);
  atomicXor(&ctr[wave * 4u + 2u], (fbx ^ (fbx >> 16)) & 0xFFFFu);
  atomicAdd(&ctr[wave * 4u + 3u], fbs);
  if (lane == 0) ctr[16u + wave] = __builtin_amdgcn_s_getreg(MI355X_DPGM_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DPGM_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPGMREC_MAGIC) v = MI355X_DPGM_MAGIC;
    if (tid == MI355X_DPGMREC_WG) v = wg;
    if (tid == MI355X_DPGMREC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPGMREC_XCC) v = __builtin_amdgcn_s_getreg(MI355X_DPGM_HWREG_XCC_ID) & 0xF;
    if (tid >= MI355X_DPGMREC_HWID && tid < MI355X_DPGMREC_HWID + 4) v = ctr[16u + tid - MI355X_DPGMREC_HWID];
    if (tid == MI355X_DPGMREC_KSTEPS) v = ksteps;
    if (tid >= MI355X_DPGMREC_FOLD && tid < MI355X_DPGMREC_FOLD + 16) v = ctr[tid - MI355X_DPGMREC_FOLD];
    args.records[static_cast<size_t>(wg) * MI355X_DPGM_REC_WORDS + tid] = v;
  }
}
