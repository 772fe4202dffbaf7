// gfx950 (CDNA4) fused attention kernels: see datapath_attn_kernel.h for the
// problem, why every word is exact, the two rules, the LDS layout and the lane
// maps.
//
// mi355x_attn_fill: heads * qblocks workgroups x 256 lanes write Q, K and V into
// device memory, 16 bytes a store, grid-strided.
//
// mi355x_mfma_datapath_attn: heads * qblocks workgroups x 256 lanes (4 waves, 32
// queries each). No inter-workgroup synchronisation and no waiting loop; where
// the workgroups land is reported (XCC id, HW_ID per wave), not arranged. Per
// block of 64 keys:
//   wait for the block's direct-to-LDS loads, barrier, issue the next block's
//   loads into the other buffer; 8 MFMAs S^T = K . Q^T (ds_read_b128 for K, Q in
//   registers); row max (v_max3_f32, v_permlane32_swap); rescale of O and l by
//   v_ldexp_f32; v_exp_f32, v_cvt_pk_bf16_f32; 8 v_permlane32_swap that make the
//   P^T fragments; 8 MFMAs O^T += V^T . P^T (ds_read_b64_tr_b16 for V).
// Accumulator register r of lane l of a 32x32 block is
// D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31]: rows are keys of S^T and d of O^T, the
// column is the lane's query.
#include <hip/hip_runtime.h>

#include "datapath_attn_kernel.h"

typedef float dpat_f32x4 __attribute__((ext_vector_type(4)));
typedef float dpat_f32x16 __attribute__((ext_vector_type(16)));
typedef float dpat_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 dpat_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 dpat_bf16x8 __attribute__((ext_vector_type(8)));
typedef short dpat_i16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t dpat_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t dpat_u32x4 __attribute__((ext_vector_type(4)));

#define MI355X_DPAT_GLOBAL(p) ((const __attribute__((address_space(1))) void*)(p))
#define MI355X_DPAT_LDS(p) ((__attribute__((address_space(3))) void*)(p))

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPAT_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPAT_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))
// s_waitcnt vmcnt(0): expcnt and lgkmcnt left at their maxima
#define MI355X_DPAT_WAIT_VM0 0x0F70

extern "C" __global__ __launch_bounds__(MI355X_DPAT_THREADS) void mi355x_attn_fill(mi355x_datapath_attn_args args) {
  const uint32_t wg = blockIdx.x;
  if (!dpat_sizes_ok(args.heads, args.qblocks, args.kblocks) || wg >= args.heads * args.qblocks) return;
  const uint32_t nq = args.qblocks * MI355X_DPAT_QBLOCK, nk = args.kblocks * MI355X_DPAT_KBLOCK;
  const uint32_t q_chunks = args.heads * nq * (MI355X_DPAT_D / 8u);  // 16-byte chunks of 8 elements
  const uint32_t kv_chunks = args.heads * nk * (MI355X_DPAT_D / 8u);
  for (uint32_t c = wg * MI355X_DPAT_THREADS + threadIdx.x; c < q_chunks + 2u * kv_chunks;
       c += args.heads * args.qblocks * MI355X_DPAT_THREADS) {
    dpat_u32x4 v;
    if (c < q_chunks) {
      const uint32_t row = c / 8u, pair = (c % 8u) * 4u, head = row / nq, query = row - head * nq;
      const uint32_t seed = dpat_head_seed(args.nonce, head);
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) v[d] = dpat_q_dword(args.nonce, seed, query, pair + d);
      reinterpret_cast<dpat_u32x4*>(args.q)[c] = v;
    } else {
      const uint32_t ck = (c - q_chunks) % kv_chunks;
      const uint32_t row = ck / 8u, pair = (ck % 8u) * 4u, head = row / nk, key = row - head * nk;
      const uint32_t seed = dpat_head_seed(args.nonce, head);
      if (c < q_chunks + kv_chunks) {
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) v[d] = dpat_k_dword(args.nonce, seed, key, pair + d);
        reinterpret_cast<dpat_u32x4*>(args.k)[ck] = v;
      } else {
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d)
          v[d] = dpat_v_elem(seed, key, 2u * (pair + d)) | (dpat_v_elem(seed, key, 2u * (pair + d) + 1u) << 16);
        reinterpret_cast<dpat_u32x4*>(args.v)[ck] = v;
      }
    }
  }
}

// xor and sum of the 16-bit elements of a fragment's dwords, folded lane by lane
__device__ inline void dpat_fold(uint32_t w, uint32_t& fx, uint32_t& fs) {
  fx ^= w;
  fs += (w & 0xFFFFu) + (w >> 16);
}

// written as two maxima: the compiler makes one v_max3_f32 of them, and knows what the instruction before needs
__device__ inline float dpat_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// two f32 to one dword of bf16, round to nearest even (v_cvt_pk_bf16_f32): the low half is `a`
__device__ inline uint32_t dpat_cvt_pk(float a, float b) {
  const dpat_f32x2 f = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, dpat_bf16x2));
}

// v_permlane32_swap: lanes 32..63 of `x` change places with lanes 0..31 of `y`; [0] is the new x, [1] the new y
__device__ inline dpat_u32x2 dpat_swap(uint32_t x, uint32_t y) {
  return __builtin_bit_cast(dpat_u32x2, __builtin_amdgcn_permlane32_swap(x, y, false, false));
}

extern "C" __global__ __launch_bounds__(MI355X_DPAT_THREADS) void mi355x_mfma_datapath_attn(
    mi355x_datapath_attn_args args) {
  // One variable per buffer, and the loop written out for an even and an odd block: see mi355x_mfma_datapath_gemm.
  __shared__ __attribute__((aligned(1024))) unsigned char lds0[2 * MI355X_DPAT_LDS_TILE_BYTES];
  __shared__ __attribute__((aligned(1024))) unsigned char lds1[2 * MI355X_DPAT_LDS_TILE_BYTES];
  __shared__ uint32_t ctr[16 + 4 + 1];  // the folds as in the record, HW_ID per wave, exp_inexact
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lane = tid & 63u;
  const uint32_t wg = blockIdx.x;
  const uint32_t kblocks = args.kblocks;
  // the operands are sized by heads, qblocks and kblocks
  if (!dpat_sizes_ok(args.heads, args.qblocks, kblocks) || wg >= args.heads * args.qblocks) return;
  if (tid < 16 + 4 + 1) ctr[tid] = 0;  // the first block's barrier comes before any use

  const uint32_t head = wg / args.qblocks, qb = wg - head * args.qblocks;
  const uint32_t hi = lane >> 5;        // lane group: elements 8*hi.. of a 16-wide MFMA k
  const uint32_t qrow = 32u * wave + (lane & 31u);  // this lane's query of the workgroup's 128
  const size_t kv_head = static_cast<size_t>(head) * kblocks * MI355X_DPAT_KBLOCK * MI355X_DPAT_D * sizeof(uint16_t);
  const unsigned char* kg = reinterpret_cast<const unsigned char*>(args.k) + kv_head;
  const unsigned char* vg = reinterpret_cast<const unsigned char*>(args.v) + kv_head;

  // Q: the four B fragments of the first MFMA, straight from global memory
  dpat_u32x4 qf[4];
  {
    const unsigned char* qg = reinterpret_cast<const unsigned char*>(args.q) +
                              ((static_cast<size_t>(head) * args.qblocks + qb) * MI355X_DPAT_QBLOCK + qrow) * 128u + hi * 16u;
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) qf[c] = *reinterpret_cast<const dpat_u32x4*>(qg + c * 32u);
  }

  // Global byte offsets of this lane's 16 bytes in the wave's two K and two V
  // wave-loads of a block. Wave-load w fills LDS bytes [1024 w, 1024 w + 1024)
  // of the tile, lane l the 16 at 16 l: rows 8w..8w+7. Which global chunk lands
  // there is the swizzle (dpgm_lds_a / dpat_lds_v, inverted).
  uint32_t k_off[2], v_off[2];
#pragma unroll
  for (uint32_t t = 0; t < 2; ++t) {
    const uint32_t row = 8u * (wave * 2u + t) + (lane >> 3), p = lane & 7u;
    k_off[t] = row * 128u + ((p ^ ((row >> 1) & 7u)) << 4);
    v_off[t] = row * 128u + ((p ^ dpat_v_swz(row)) << 4);
  }
  const auto issue_loads = [&](unsigned char* lds, uint32_t s) {
    unsigned char* buf = lds + wave * 2048u;
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t) {
      __builtin_amdgcn_global_load_lds(MI355X_DPAT_GLOBAL(kg + k_off[t] + s * MI355X_DPAT_LDS_TILE_BYTES),
                                       MI355X_DPAT_LDS(buf + t * 1024u), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(MI355X_DPAT_GLOBAL(vg + v_off[t] + s * MI355X_DPAT_LDS_TILE_BYTES),
                                       MI355X_DPAT_LDS(buf + MI355X_DPAT_LDS_TILE_BYTES + t * 1024u), 16, 0, 0);
    }
  };

  // V, transposed read: this lane addresses key 8*hi + ((lane&15)>>2) (+ 16 kc + 4 h), d 16*((lane>>4)&1) + 4*(lane&3)..
  const uint32_t v_key = 8u * hi + ((lane & 15u) >> 2);
  const uint32_t v_d = 16u * ((lane >> 4) & 1u) + 4u * (lane & 3u);  // + 32 * dh

  dpat_f32x16 oacc[2];
#pragma unroll
  for (uint32_t dh = 0; dh < 2; ++dh)
#pragma unroll
    for (uint32_t r = 0; r < 16; ++r) oacc[dh][r] = 0.f;
  float m = MI355X_DPAT_M_START, l = 0.f;
  uint32_t fkx = 0, fks = 0, fvx = 0, fvs = 0, inexact = 0;

  // one block: reads `cur`, which the loads of block s filled, while the loads of block s + 1 fill `nxt`
  const auto step = [&](unsigned char* cur, unsigned char* nxt, uint32_t s) {
    __builtin_amdgcn_s_waitcnt(MI355X_DPAT_WAIT_VM0);  // this wave's loads of block s have landed
    __syncthreads();                                   // and everyone's; everyone has read the other buffer
    if (s + 1u < kblocks) issue_loads(nxt, s + 1u);
    const unsigned char* kt = cur;
    const unsigned char* vt = cur + MI355X_DPAT_LDS_TILE_BYTES;

    // S^T = K . Q^T
    dpat_f32x16 sacc[2];
#pragma unroll
    for (uint32_t sb = 0; sb < 2; ++sb) {
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r) sacc[sb][r] = 0.f;
#pragma unroll
      for (uint32_t c = 0; c < 4; ++c) {
        const dpat_u32x4 kf = *reinterpret_cast<const dpat_u32x4*>(kt + dpgm_lds_a(32u * sb + (lane & 31u), 2u * c + hi));
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) dpat_fold(kf[d], fkx, fks);
        sacc[sb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(dpat_bf16x8, kf),
                                                           __builtin_bit_cast(dpat_bf16x8, qf[c]), sacc[sb], 0, 0, 0);
      }
    }
#if defined(MI355X_TEST_INJECT)
    if (args.inject_kind == MI355X_DPAT_INJECT_S && wg == args.inject_wg && wave == args.inject_wave &&
        lane == args.inject_lane && (args.inject_index >> 5) == s) {
#pragma unroll
      for (uint32_t sb = 0; sb < 2; ++sb)
#pragma unroll
        for (uint32_t r = 0; r < 16; ++r)
          if (sb * 16u + r == (args.inject_index & 31u))
            sacc[sb][r] = __uint_as_float(__float_as_uint(sacc[sb][r]) ^ args.inject_mask);
    }
#endif

    // the row max: 32 registers in the lane, then the other 32 keys from lane ^ 32
    float mx = dpat_max3(sacc[0][0], sacc[0][1], sacc[0][2]);
#pragma unroll
    for (uint32_t r = 3; r < 31; r += 2) mx = dpat_max3(mx, sacc[r >> 4][r & 15u], sacc[(r + 1u) >> 4][(r + 1u) & 15u]);
    mx = fmaxf(mx, sacc[1][15]);
    const dpat_u32x2 both = dpat_swap(__float_as_uint(mx), __float_as_uint(mx));
    const float m_new = dpat_max3(m, __uint_as_float(both[0]), __uint_as_float(both[1]));

    // rule 2: the rescale is v_ldexp_f32 by an integer
    const int k = static_cast<int>(m - m_new);
    m = m_new;
    l = __builtin_ldexpf(l, k);
#pragma unroll
    for (uint32_t dh = 0; dh < 2; ++dh)
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r) oacc[dh][r] = __builtin_ldexpf(oacc[dh][r], k);

    // rule 1: P = v_exp_f32(S - m), rounded to bf16; l from the rounded P
    uint32_t pk[2][8];
#pragma unroll
    for (uint32_t sb = 0; sb < 2; ++sb)
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        const float e0 = __builtin_amdgcn_exp2f(sacc[sb][2u * j] - m_new);
        const float e1 = __builtin_amdgcn_exp2f(sacc[sb][2u * j + 1u] - m_new);
        inexact += ((__float_as_uint(e0) & 0x7FFFFFu) != 0u) + ((__float_as_uint(e1) & 0x7FFFFFu) != 0u);
        pk[sb][j] = dpat_cvt_pk(e0, e1);
        l += __uint_as_float(pk[sb][j] << 16);
        l += __uint_as_float(pk[sb][j] & 0xFFFF0000u);
      }

    // O^T += V^T . P^T, 16 keys at a time: key chunk kc is registers 8*(kc&1).. of sub-block kc>>1
#pragma unroll
    for (uint32_t kc = 0; kc < 4; ++kc) {
      const uint32_t* x = &pk[kc >> 1][4u * (kc & 1u)];  // x[0..1] = registers 0..3, x[2..3] = registers 4..7 of the chunk
      const dpat_u32x2 s0 = dpat_swap(x[0], x[2]), s1 = dpat_swap(x[1], x[3]);
      const dpat_u32x4 pf = {s0[0], s1[0], s0[1], s1[1]};
#pragma unroll
      for (uint32_t dh = 0; dh < 2; ++dh) {
        dpat_u32x4 vf;
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
          const uint32_t key = 16u * kc + 4u * h + v_key, d = 32u * dh + v_d;
          const unsigned char* p = vt + dpat_lds_v(key, d >> 3) + (d & 7u) * 2u;
          const dpat_i16x4 q = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) dpat_i16x4*)(p));
          const dpat_u32x2 w = __builtin_bit_cast(dpat_u32x2, q);
          vf[2u * h] = w[0];
          vf[2u * h + 1u] = w[1];
        }
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) dpat_fold(vf[d], fvx, fvs);
        oacc[dh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(dpat_bf16x8, vf),
                                                           __builtin_bit_cast(dpat_bf16x8, pf), oacc[dh], 0, 0, 0);
      }
    }
  };
  issue_loads(lds0, 0);
#pragma unroll 1
  for (uint32_t s = 0; s < kblocks; s += 2u) {
    step(lds0, lds1, s);
    if (s + 1u >= kblocks) break;
    step(lds1, lds0, s + 1u);
  }

  // the two half-waves' partial sums of l, once
  const dpat_u32x2 lh = dpat_swap(__float_as_uint(l), __float_as_uint(l));
  l = __uint_as_float(lh[0]) + __uint_as_float(lh[1]);

  const size_t row = static_cast<size_t>(wg) * MI355X_DPAT_QBLOCK + qrow;
#pragma unroll
  for (uint32_t dh = 0; dh < 2; ++dh)
#pragma unroll
    for (uint32_t g = 0; g < 4; ++g) {
      dpat_u32x4 w;
#pragma unroll
      for (uint32_t e = 0; e < 4; ++e) {
        w[e] = __float_as_uint(oacc[dh][4u * g + e]);
#if defined(MI355X_TEST_INJECT)
        if (args.inject_kind == MI355X_DPAT_INJECT_O && wg == args.inject_wg && wave == args.inject_wave &&
            lane == args.inject_lane && dh * 16u + 4u * g + e == args.inject_index)
          w[e] ^= args.inject_mask;
#endif
      }
      *reinterpret_cast<dpat_u32x4*>(args.o + row * MI355X_DPAT_D + 32u * dh + 8u * g + 4u * hi) = w;
    }
  if (hi == 0u) {
    const dpat_u32x2 w = {__float_as_uint(m), __float_as_uint(l)};
    *reinterpret_cast<dpat_u32x2*>(args.ml + row * 2u) = w;
  }

  atomicXor(&ctr[wave * 4u + 0u], (fkx ^ (fkx >> 16)) & 0xFFFFu);
  atomicAdd(&ctr[wave * 4u + 1u], fks);
  atomicXor(&ctr[wave * 4u + 2u], (fvx ^ (fvx >> 16)) & 0xFFFFu);
  atomicAdd(&ctr[wave * 4u + 3u], fvs);
  atomicAdd(&ctr[20], inexact);
  if (lane == 0) ctr[16u + wave] = __builtin_amdgcn_s_getreg(MI355X_DPAT_HWREG_HW_ID);
  __syncthreads();

  if (tid < MI355X_DPAT_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPATREC_MAGIC) v = MI355X_DPAT_MAGIC;
    if (tid == MI355X_DPATREC_WG) v = wg;
    if (tid == MI355X_DPATREC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPATREC_XCC) v = __builtin_amdgcn_s_getreg(MI355X_DPAT_HWREG_XCC_ID) & 0xF;
    if (tid >= MI355X_DPATREC_HWID && tid < MI355X_DPATREC_HWID + 4) v = ctr[16u + tid - MI355X_DPATREC_HWID];
    if (tid == MI355X_DPATREC_HEADS) v = args.heads;
    if (tid == MI355X_DPATREC_QBLOCKS) v = args.qblocks;
    if (tid == MI355X_DPATREC_KBLOCKS) v = kblocks;
    if (tid == MI355X_DPATREC_EXP_INEXACT) v = ctr[20];
    if (tid >= MI355X_DPATREC_FOLD && tid < MI355X_DPATREC_FOLD + 16) v = ctr[tid - MI355X_DPATREC_FOLD];
    args.records[static_cast<size_t>(wg) * MI355X_DPAT_REC_WORDS + tid] = v;
  }
}
