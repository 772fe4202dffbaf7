// gfx950 (CDNA4) MX quantise kernels: see datapath_mxquant_kernel.h for the
// problem, the operand recipe, the LDS layouts and the lane maps.
//
// mi355x_mxquant_fill: `grid` workgroups x 256 lanes write X (grid panels), W1,
// W2 and sb into device memory, 16 bytes a store, grid-strided.
//
// mi355x_mfma_datapath_mxquant: `grid` workgroups x 256 lanes (4 waves). No
// inter-workgroup synchronisation and no waiting loop; where the workgroups land
// is reported (XCC id, HW_ID per wave), not arranged. Per slab of 128 hidden
// columns:
//   wait for the slab's direct-to-LDS loads, barrier, issue the next slab's loads
//   into the other buffers and its W2 scale loads into registers; per block of 32
//   hidden columns 8 MFMAs H^T = W1 . X^T (ds_read_b128 for W1, X in registers),
//   amax (v_max3_f32, v_permlane32_swap), E, 8 v_cvt_scalef32_pk_fp4_f32, one
//   v_permlane32_swap, 2 v_perm_b32, one ds_write_b64 into the Q tile; the scale
//   dword; barrier; then the mxgemm check's sub-steps on the Q tile and the W2
//   tile: 2 x (2 + 2 ds_read_b128, 4 v_mfma_scale_f32_32x32x64_f8f6f4).
// Accumulator register r of lane l of a 32x32 block is
// D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
#include <hip/hip_runtime.h>

#include "datapath_mxquant_kernel.h"

typedef float dpmq_f32x16 __attribute__((ext_vector_type(16)));
typedef int dpmq_i32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 dpmq_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t dpmq_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t dpmq_u32x4 __attribute__((ext_vector_type(4)));

#define MI355X_DPMQ_GLOBAL(p) ((const __attribute__((address_space(1))) void*)(p))
#define MI355X_DPMQ_LDS(p) ((__attribute__((address_space(3))) void*)(p))

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPMQ_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPMQ_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))
// s_waitcnt vmcnt(0): expcnt and lgkmcnt left at their maxima
#define MI355X_DPMQ_WAIT_VM0 0x0F70

extern "C" __global__ __launch_bounds__(MI355X_DPMQ_THREADS) void mi355x_mxquant_fill(mi355x_datapath_mxquant_args args) {
  const uint32_t wg = blockIdx.x;
  if (wg >= args.grid || args.hsteps == 0 || args.hsteps > MI355X_DPMQ_HSTEPS_MAX) return;
  // 16-byte chunks: X and W1 rows have 16 (four pairs each), a W2 row 4 * hsteps, sb is 512 * hsteps bytes
  const uint32_t x_chunks = args.grid * MI355X_DPMQ_TILE * 16u, w1_chunks = args.hsteps * MI355X_DPMQ_TILE * 16u;
  const uint32_t w2_chunks = MI355X_DPMQ_TILE * 4u * args.hsteps, sb_chunks = 32u * args.hsteps;
  for (uint32_t c = wg * MI355X_DPMQ_THREADS + threadIdx.x; c < x_chunks + w1_chunks + w2_chunks + sb_chunks;
       c += args.grid * MI355X_DPMQ_THREADS) {
    dpmq_u32x4 v;
    if (c < x_chunks) {
      const uint32_t row = c / 16u, pair = (c % 16u) * 4u, panel = row / MI355X_DPMQ_TILE;
      const uint32_t seed = dpmq_wg_seed(args.nonce, panel);
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) v[d] = dpmq_x_dword(args.nonce, seed, row % MI355X_DPMQ_TILE, pair + d);
      reinterpret_cast<dpmq_u32x4*>(args.x)[c] = v;
    } else if (c < x_chunks + w1_chunks) {
      const uint32_t cc = c - x_chunks;
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) v[d] = dpmq_w1_dword(args.nonce, cc / 16u, (cc % 16u) * 4u + d);
      reinterpret_cast<dpmq_u32x4*>(args.w1)[cc] = v;
    } else if (c < x_chunks + w1_chunks + w2_chunks) {
      const uint32_t cc = c - x_chunks - w1_chunks;
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) v[d] = dpmq_w2_dword(args.nonce, args.hsteps, cc / (4u * args.hsteps), (cc % (4u * args.hsteps)) * 4u + d);
      reinterpret_cast<dpmq_u32x4*>(args.w2)[cc] = v;
    } else {
      const uint32_t cc = c - x_chunks - w1_chunks - w2_chunks;
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
          const uint32_t f = cc * 16u + d * 4u + i, col = f / (4u * args.hsteps), block = f % (4u * args.hsteps);
          w |= (dpmq_sb_base(args.nonce, col) + dpmq_sb_delta(args.nonce, col, block)) << (8u * i);
        }
        v[d] = w;
      }
      reinterpret_cast<dpmq_u32x4*>(args.sb)[cc] = v;
    }
  }
}

// xor and sum of dwords, folded lane by lane
__device__ inline void dpmq_fold(uint32_t w, uint32_t& fx, uint32_t& fs) {
  fx ^= w;
  fs += w;
}

// written as two maxima: the compiler makes one v_max3_f32 of them
__device__ inline float dpmq_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// v_permlane32_swap: lanes 32..63 of `x` change places with lanes 0..31 of `y`; [0] is the new x, [1] the new y
__device__ inline dpmq_u32x2 dpmq_swap(uint32_t x, uint32_t y) {
  return __builtin_bit_cast(dpmq_u32x2, __builtin_amdgcn_permlane32_swap(x, y, false, false));
}

extern "C" __global__ __launch_bounds__(MI355X_DPMQ_THREADS) void mi355x_mfma_datapath_mxquant(
    mi355x_datapath_mxquant_args args) {
  // One variable per buffer, and the loop written out for an even and an odd slab: see mi355x_mfma_datapath_gemm.
  __shared__ __attribute__((aligned(1024))) unsigned char w1_0[MI355X_DPMQ_LDS_W1_BYTES];
  __shared__ __attribute__((aligned(1024))) unsigned char w1_1[MI355X_DPMQ_LDS_W1_BYTES];
  __shared__ __attribute__((aligned(1024))) unsigned char w2_0[MI355X_DPMQ_LDS_W2_BYTES];
  __shared__ __attribute__((aligned(1024))) unsigned char w2_1[MI355X_DPMQ_LDS_W2_BYTES];
  __shared__ __attribute__((aligned(1024))) unsigned char qt[MI355X_DPMQ_LDS_W2_BYTES];  // the quantised slab
  __shared__ uint32_t qs[MI355X_DPMQ_TILE];                                              // and its four scale bytes a token
  __shared__ uint32_t ctr[24 + 4];  // the folds as in the record, then HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lane = tid & 63u;
  const uint32_t wg = blockIdx.x;
  const uint32_t hsteps = args.hsteps;
  if (wg >= args.grid || hsteps == 0 || hsteps > MI355X_DPMQ_HSTEPS_MAX) return;  // the operands are sized by hsteps
  if (tid < 24 + 4) ctr[tid] = 0;  // the first slab's barrier comes before any use

  const uint32_t hi = lane >> 5;                 // lane group: k 8*hi.. of a 16-wide MFMA k, 32*hi.. of a 64-wide one
  const uint32_t token = 32u * wave + (lane & 31u);  // the token this lane quantises
  const unsigned char* w1g = reinterpret_cast<const unsigned char*>(args.w1);
  const unsigned char* w2g = args.w2;

  // X: the eight B fragments of GEMM 1, straight from global memory
  dpmq_u32x4 xf[8];
  {
    const unsigned char* xg = reinterpret_cast<const unsigned char*>(args.x) +
                              (static_cast<size_t>(wg) * MI355X_DPMQ_TILE + token) * 256u + hi * 16u;
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c) xf[c] = *reinterpret_cast<const dpmq_u32x4*>(xg + c * 32u);
  }

  // Global byte offsets of this lane's 16 bytes in the wave's wave-loads of a slab. A wave-load fills 1 KiB of
  // consecutive LDS, lane l the 16 bytes at 16 l. W1: wave-load wave * 8 + t is rows 8 * ((wave & 1) * 8 + t).. of
  // k-half wave >> 1 (8 rows of 128 bytes); W2: wave-load wave * 2 + t is rows 16 * (wave * 2 + t).. (16 rows of 64
  // bytes). Which global chunk lands there is the swizzle (dpgm_lds_a / dpmq_lds, inverted).
  uint32_t w1_off[8], w2_off[2];
#pragma unroll
  for (uint32_t t = 0; t < 8; ++t) {
    const uint32_t row = 8u * ((wave & 1u) * 8u + t) + (lane >> 3), kc = (lane & 7u) ^ ((row >> 1) & 7u);
    w1_off[t] = row * 256u + (wave >> 1) * 128u + kc * 16u;
  }
#pragma unroll
  for (uint32_t t = 0; t < 2; ++t) {
    const uint32_t row = 16u * (wave * 2u + t) + (lane >> 2), c = (lane & 3u) ^ ((row >> 2) & 3u);
    w2_off[t] = row * (64u * hsteps) + c * 16u;
  }
  const auto issue_loads = [&](unsigned char* w1l, unsigned char* w2l, uint32_t s) {
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t)
      __builtin_amdgcn_global_load_lds(MI355X_DPMQ_GLOBAL(w1g + w1_off[t] + s * MI355X_DPMQ_LDS_W1_BYTES),
                                       MI355X_DPMQ_LDS(w1l + (wave * 8u + t) * 1024u), 16, 0, 0);
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t)
      __builtin_amdgcn_global_load_lds(MI355X_DPMQ_GLOBAL(w2g + w2_off[t] + s * 64u),
                                       MI355X_DPMQ_LDS(w2l + (wave * 2u + t) * 1024u), 16, 0, 0);
  };

  // GEMM 2: the wave's sub-tile and this lane's place in its fragments
  const uint32_t row0 = 64u * (wave >> 1), col0 = 64u * (wave & 1u);
  const uint32_t a_row = row0 + (lane & 31u);  // + 32 * rb
  const uint32_t b_col = col0 + (lane & 31u);  // + 32 * cb
  const uint32_t perm_sel = hi ? 0x03010301u : 0x02000200u;
  const uint32_t* sbp[2];  // this lane's W2 scale bytes: 4 a slab of each of its two columns
#pragma unroll
  for (uint32_t t = 0; t < 2; ++t) sbp[t] = reinterpret_cast<const uint32_t*>(args.sb + (b_col + 32u * t) * (4u * hsteps));
  uint32_t sbraw[2] = {sbp[0][0], sbp[1][0]};

  // where this lane writes its 8-byte half of a block: lanes with bit 4 set take the other half
  const uint32_t flip = (lane >> 4) & 1u, half = flip ^ hi;
  uint32_t* image = args.image + static_cast<size_t>(wg) * MI355X_DPMQ_IMG_WORDS(hsteps);

  const uint32_t seed = dpmq_wg_seed(args.nonce, wg);
  dpmq_f32x16 acc[2][2];
#pragma unroll
  for (uint32_t rb = 0; rb < 2; ++rb)
#pragma unroll
    for (uint32_t cb = 0; cb < 2; ++cb)
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r)
        acc[rb][cb][r] = __uint_as_float(dpmq_c_word(seed, args.nonce, row0 + 32u * rb + (r & 3u) + 8u * (r >> 2) + 4u * hi,
                                                     col0 + 32u * cb + (lane & 31u)));

  uint32_t fax = 0, fas = 0, fbx = 0, fbs = 0, fsx = 0, fss = 0;
  // one slab: reads the buffers the loads of slab s filled, while the loads of slab s + 1 fill the others
  const auto step = [&](unsigned char* w1c, unsigned char* w2c, unsigned char* w1n, unsigned char* w2n, uint32_t s,
                        uint32_t odd) {
    __builtin_amdgcn_s_waitcnt(MI355X_DPMQ_WAIT_VM0);  // this wave's loads of slab s have landed
    __syncthreads();                                   // and everyone's; everyone has read the other buffers and the Q tile
    const uint32_t sbcur[2] = {sbraw[0], sbraw[1]};
    if (s + 1u < hsteps) {
      issue_loads(w1n, w2n, s + 1u);
#pragma unroll
      for (uint32_t t = 0; t < 2; ++t) sbraw[t] = sbp[t][s + 1u];
    }

    // GEMM 1 and the quantisation, a block of 32 hidden columns at a time
    uint32_t escale = 0;
#pragma unroll
    for (uint32_t blk = 0; blk < 4; ++blk) {
      dpmq_f32x16 h;
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r) h[r] = 0.f;
#pragma unroll
      for (uint32_t c = 0; c < 8; ++c) {
        const dpmq_u32x4 wf = *reinterpret_cast<const dpmq_u32x4*>(w1c + (c >> 2) * 16384u +
                                                                   dpgm_lds_a(32u * blk + (lane & 31u), 2u * (c & 3u) + hi));
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) dpmq_fold(wf[d], fax, fas);
        h = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(dpmq_bf16x8, wf), __builtin_bit_cast(dpmq_bf16x8, xf[c]),
                                                    h, 0, 0, 0);
      }
#if defined(MI355X_TEST_INJECT)
      if (args.inject_kind == MI355X_DPMQ_INJECT_H && wg == args.inject_wg && wave == args.inject_wave &&
          lane == args.inject_lane && (args.inject_index >> 4) == s * 4u + blk) {
#pragma unroll
        for (uint32_t r = 0; r < 16; ++r)
          if (r == (args.inject_index & 15u)) h[r] = __uint_as_float(__float_as_uint(h[r]) ^ args.inject_mask);
      }
#endif
      // amax: 16 registers in the lane, the block's other 16 columns from lane ^ 32
      float mx = dpmq_max3(fabsf(h[0]), fabsf(h[1]), fabsf(h[2]));
#pragma unroll
      for (uint32_t r = 3; r < 15; r += 2) mx = dpmq_max3(mx, fabsf(h[r]), fabsf(h[r + 1u]));
      mx = fmaxf(mx, fabsf(h[15]));
      const dpmq_u32x2 both = dpmq_swap(__float_as_uint(mx), __float_as_uint(mx));
      const float amax = fmaxf(__uint_as_float(both[0]), __uint_as_float(both[1]));
      const uint32_t e = dpmq_e8m0(__float_as_uint(amax));
      escale |= e << (8u * blk);
      const float scale = __uint_as_float(e << 23);  // 2^(E-127), exact
      // byte k of a dword = registers (2k, 2k+1), the first in the low nibble
      uint32_t d0 = 0, d1 = 0;
      d0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(d0, h[0], h[1], scale, 0);
      d0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(d0, h[2], h[3], scale, 1);
      d0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(d0, h[4], h[5], scale, 2);
      d0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(d0, h[6], h[7], scale, 3);
      d1 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(d1, h[8], h[9], scale, 0);
      d1 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(d1, h[10], h[11], scale, 1);
      d1 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(d1, h[12], h[13], scale, 2);
      d1 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(d1, h[14], h[15], scale, 3);
      // d0 is the lane's 2-byte pieces of bytes 0..7 of the block, d1 of bytes 8..15; after the swap a lane holds
      // both lanes' dwords of one half ([0] from lane & 31, [1] from lane | 32), which interleave piece by piece
      const dpmq_u32x2 sw = dpmq_swap(flip ? d1 : d0, flip ? d0 : d1);
      const dpmq_u32x2 out = {__builtin_amdgcn_perm(sw[1], sw[0], 0x05040100u), __builtin_amdgcn_perm(sw[1], sw[0], 0x07060302u)};
      *reinterpret_cast<dpmq_u32x2*>(qt + dpmq_lds(token, blk) + 8u * half) = out;
    }
    if (hi == 0u) qs[token] = escale;
    __syncthreads();  // the Q tile is whole
#if defined(MI355X_TEST_INJECT)
    if (args.inject_kind == MI355X_DPMQ_INJECT_Q && wg == args.inject_wg && s == args.inject_wave) {
      if (tid == 0) reinterpret_cast<uint32_t*>(qt)[args.inject_index & (MI355X_DPMQ_LDS_W2_BYTES / 4u - 1u)] ^= args.inject_mask;
      __syncthreads();
    }
#endif

    // GEMM 2 on the slab: the gathered scales (the activations' row blocks, then W2's column blocks)
    uint32_t araw[2], sc[4];
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t) {
      araw[t] = qs[a_row + 32u * t];
      sc[t] = __builtin_amdgcn_perm(araw[t], araw[t], perm_sel);
      sc[2 + t] = __builtin_amdgcn_perm(sbcur[t], sbcur[t], perm_sel);
      if ((wave & 1u) == 0u && hi == 0u) image[2048u * hsteps + (a_row + 32u * t) * hsteps + s] = araw[t];
    }
#pragma unroll
    for (uint32_t kk = 0; kk < 2; ++kk) {
#if defined(MI355X_TEST_INJECT)
      if (args.inject_kind == MI355X_DPMQ_INJECT_SCALE && wg == args.inject_wg && wave == args.inject_wave &&
          lane == args.inject_lane && s * 8u + kk * 4u == (args.inject_index & ~3u)) {
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t)
          if (t == (args.inject_index & 3u)) sc[t] ^= args.inject_mask;
      }
#endif
      dpmq_i32x8 af[2], bf[2];
#pragma unroll
      for (uint32_t t = 0; t < 2; ++t) {
        const dpmq_u32x4 a4 = *reinterpret_cast<const dpmq_u32x4*>(qt + dpmq_lds(a_row + 32u * t, 2u * kk + hi));
        const dpmq_u32x4 b4 = *reinterpret_cast<const dpmq_u32x4*>(w2c + dpmq_lds(b_col + 32u * t, 2u * kk + hi));
        if ((wave & 1u) == 0u)  // the image as read: one of the two waves that read these rows stores it
          *reinterpret_cast<dpmq_u32x4*>(image + (a_row + 32u * t) * (16u * hsteps) + s * 16u + (2u * kk + hi) * 4u) = a4;
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
          dpmq_fold(b4[d], fbx, fbs);
          af[t][d] = static_cast<int>(a4[d]);
          bf[t][d] = static_cast<int>(b4[d]);
          af[t][4 + d] = 0;  // e2m1 fragments are four dwords: the instruction does not read these
          bf[t][4 + d] = 0;
        }
      }
      const uint32_t sel = 2u * odd + kk;  // op_sel: the byte of both scale VGPRs
#pragma unroll
      for (uint32_t rb = 0; rb < 2; ++rb)
#pragma unroll
        for (uint32_t cb = 0; cb < 2; ++cb) {
          const int sa = static_cast<int>(sc[rb]), sw2 = static_cast<int>(sc[2 + cb]);
          // cbsz = blgp = 4: e2m1
          if (sel == 0) acc[rb][cb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[rb], bf[cb], acc[rb][cb], 4, 4, 0, sa, 0, sw2);
          if (sel == 1) acc[rb][cb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[rb], bf[cb], acc[rb][cb], 4, 4, 1, sa, 1, sw2);
          if (sel == 2) acc[rb][cb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[rb], bf[cb], acc[rb][cb], 4, 4, 2, sa, 2, sw2);
          if (sel == 3) acc[rb][cb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[rb], bf[cb], acc[rb][cb], 4, 4, 3, sa, 3, sw2);
        }
    }
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) dpmq_fold(sc[t], fsx, fss);  // as fed
  };
  issue_loads(w1_0, w2_0, 0);
#pragma unroll 1
  for (uint32_t s = 0; s < hsteps; s += 2u) {
    step(w1_0, w2_0, w1_1, w2_1, s, 0u);
    if (s + 1u >= hsteps) break;
    step(w1_1, w2_1, w1_0, w2_0, s + 1u, 1u);
  }

  uint32_t* tile = args.tiles + static_cast<size_t>(wg) * MI355X_DPMQ_WG_WORDS;
#pragma unroll
  for (uint32_t rb = 0; rb < 2; ++rb)
#pragma unroll
    for (uint32_t cb = 0; cb < 2; ++cb)
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r) {
        uint32_t word = __float_as_uint(acc[rb][cb][r]);
#if defined(MI355X_TEST_INJECT)
        if (args.inject_kind == MI355X_DPMQ_INJECT_MFMA && wg == args.inject_wg && wave == args.inject_wave &&
            lane == args.inject_lane && (rb * 2u + cb) * 16u + r == args.inject_index)
          word ^= args.inject_mask;
#endif
        tile[(row0 + 32u * rb + (r & 3u) + 8u * (r >> 2) + 4u * hi) * MI355X_DPMQ_TILE + col0 + 32u * cb + (lane & 31u)] = word;
      }

  atomicXor(&ctr[wave * 6u + 0u], fax);
  atomicAdd(&ctr[wave * 6u + 1u], fas);
  atomicXor(&ctr[wave * 6u + 2u], fbx);
  atomicAdd(&ctr[wave * 6u + 3u], fbs);
  atomicXor(&ctr[wave * 6u + 4u], fsx);
  atomicAdd(&ctr[wave * 6u + 5u], fss);
  if (lane == 0) ctr[24u + wave] = __builtin_amdgcn_s_getreg(MI355X_DPMQ_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DPMQ_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPMQREC_MAGIC) v = MI355X_DPMQ_MAGIC;
    if (tid == MI355X_DPMQREC_WG) v = wg;
    if (tid == MI355X_DPMQREC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPMQREC_XCC) v = (__builtin_amdgcn_s_getreg(MI355X_DPMQ_HWREG_XCC_ID) & 0xF) | (hsteps << 8);
    if (tid >= MI355X_DPMQREC_HWID && tid < MI355X_DPMQREC_HWID + 4) v = ctr[24u + tid - MI355X_DPMQREC_HWID];
    if (tid >= MI355X_DPMQREC_FOLD) v = ctr[tid - MI355X_DPMQREC_FOLD];
    args.records[static_cast<size_t>(wg) * MI355X_DPMQ_REC_WORDS + tid] = v;
  }
}
