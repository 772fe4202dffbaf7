// gfx950 (CDNA4) split-K GEMM kernels: see datapath_splitk_kernel.h for the
// problem, why any arrival order is exact, the LDS layout, the swizzle and the
// ledger.
//
// mi355x_splitk_fill: tiles * splits workgroups x 256 lanes write A, B, D = C and
// the zeroed ledger into device memory, 16 bytes a store, grid-strided.
//
// mi355x_mfma_datapath_splitk: tiles * splits workgroups x 256 lanes (4 waves,
// 2 x 2). No inter-workgroup synchronisation and no waiting loop; where the
// workgroups land is reported (XCC id, HW_ID per wave), not arranged. Per k-step
// of 64:
//   wait for the step's direct-to-LDS loads, barrier, issue the next step's
//   loads into the other buffer, then two 32-wide sub-steps of four A fragments
//   (ds_read_b128), four B fragments (two ds_read_b64_tr_b16 each) and sixteen
//   v_mfma_f32_16x16x32_bf16, each on the accumulator the previous sub-step left.
// Accumulator register r of lane l of a 16x16 block is D[4*(l>>4) + r][l&15].
// Then 64 no-return f32 atomic adds a lane into D_t and six integer atomics a
// workgroup into the tile's ledger.
//
// mi355x_splitk_drain: one workgroup a tile copies D_t and the ledger to the
// host-visible buffers.
#include <hip/hip_runtime.h>

#include "datapath_splitk_kernel.h"

typedef float dpsk_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 dpsk_bf16x8 __attribute__((ext_vector_type(8)));
typedef short dpsk_i16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t dpsk_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t dpsk_u32x4 __attribute__((ext_vector_type(4)));

#define MI355X_DPSK_GLOBAL(p) ((const __attribute__((address_space(1))) void*)(p))
#define MI355X_DPSK_LDS(p) ((__attribute__((address_space(3))) void*)(p))

// s_getreg_b32 HW_REG_XCC_ID (hwreg 20), bits [3:0]; HW_REG_HW_ID (hwreg 4)
#define MI355X_DPSK_HWREG_XCC_ID ((20) | (0 << 6) | ((16 - 1) << 11))
#define MI355X_DPSK_HWREG_HW_ID ((4) | (0 << 6) | ((32 - 1) << 11))
// s_waitcnt vmcnt(0): expcnt and lgkmcnt left at their maxima
#define MI355X_DPSK_WAIT_VM0 0x0F70

extern "C" __global__ __launch_bounds__(MI355X_DPSK_THREADS) void mi355x_splitk_fill(mi355x_datapath_splitk_args args) {
  const uint32_t wg = blockIdx.x;
  if (!dpsk_sizes_ok(args.tiles, args.splits, args.ksteps) || wg >= args.tiles * args.splits) return;
  const uint32_t ksteps_total = args.splits * args.ksteps;
  const uint32_t K = ksteps_total * MI355X_DPGM_KSTEP;
  const uint32_t panel_chunks = MI355X_DPGM_TILE * (K / 8u);  // 16-byte chunks of 8 elements
  const uint32_t a_chunks = args.tiles * panel_chunks;
  const uint32_t b_chunks = K * (MI355X_DPGM_TILE / 8u);
  const uint32_t d_chunks = args.tiles * (MI355X_DPSK_TILE_WORDS / 4u);  // 16-byte chunks of 4 words
  const uint32_t l_chunks = args.tiles * (MI355X_DPSK_LEDGER_WORDS / 4u);
  for (uint32_t c = wg * MI355X_DPSK_THREADS + threadIdx.x; c < a_chunks + b_chunks + d_chunks + l_chunks;
       c += args.tiles * args.splits * MI355X_DPSK_THREADS) {
    dpsk_u32x4 v = {0u, 0u, 0u, 0u};
    if (c < a_chunks) {
      const uint32_t panel = c / panel_chunks, in_panel = c - panel * panel_chunks;
      const uint32_t row = in_panel / (K / 8u), k = (in_panel % (K / 8u)) * 8u;
      const uint32_t seed = dpgm_wg_seed(args.nonce, panel);
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) v[d] = dpgm_a_dword(seed, ksteps_total, row, k + 2u * d);
      reinterpret_cast<dpsk_u32x4*>(args.a)[c] = v;
    } else if (c < a_chunks + b_chunks) {
      const uint32_t cb = c - a_chunks;
      const uint32_t k = cb / (MI355X_DPGM_TILE / 8u), col = (cb % (MI355X_DPGM_TILE / 8u)) * 8u;
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d)
        v[d] = dpgm_b_elem(args.nonce, k, col + 2u * d) | (dpgm_b_elem(args.nonce, k, col + 2u * d + 1u) << 16);
      reinterpret_cast<dpsk_u32x4*>(args.b)[cb] = v;
    } else if (c < a_chunks + b_chunks + d_chunks) {
      const uint32_t cd = c - a_chunks - b_chunks;
      const uint32_t tile = cd / (MI355X_DPSK_TILE_WORDS / 4u), word = (cd % (MI355X_DPSK_TILE_WORDS / 4u)) * 4u;
      const uint32_t seed = dpgm_wg_seed(args.nonce, tile);
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d)
        v[d] = dpgm_c_word(seed, args.nonce, word / MI355X_DPGM_TILE, word % MI355X_DPGM_TILE + d);
      reinterpret_cast<dpsk_u32x4*>(args.d)[cd] = v;
    } else {
      reinterpret_cast<dpsk_u32x4*>(args.ledger)[c - a_chunks - b_chunks - d_chunks] = v;
    }
  }
}

// xor and sum of the 16-bit elements of a fragment's dwords, folded lane by lane
__device__ inline void dpsk_fold(uint32_t w, uint32_t& fx, uint32_t& fs) {
  fx ^= w;
  fs += (w & 0xFFFFu) + (w >> 16);
}

extern "C" __global__ __launch_bounds__(MI355X_DPSK_THREADS) void mi355x_mfma_datapath_splitk(
    mi355x_datapath_splitk_args args) {
  // One variable per buffer, and the loop written out for an even and an odd step: see mi355x_mfma_datapath_gemm.
  __shared__ __attribute__((aligned(1024))) unsigned char lds0[MI355X_DPGM_LDS_BYTES / 2];
  __shared__ __attribute__((aligned(1024))) unsigned char lds1[MI355X_DPGM_LDS_BYTES / 2];
  __shared__ uint32_t ctr[16 + 4];  // the folds as in the record, then HW_ID per wave
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lane = tid & 63u;
  const uint32_t wg = blockIdx.x;
  const uint32_t ksteps = args.ksteps;
  // the operands are sized by tiles and splits * ksteps
  if (!dpsk_sizes_ok(args.tiles, args.splits, ksteps) || wg >= args.tiles * args.splits) return;
  if (tid < 16 + 4) ctr[tid] = 0;  // the first step's barrier comes before any use

  const uint32_t tile = wg / args.splits, split = wg - tile * args.splits;
  const uint32_t K = args.splits * ksteps * MI355X_DPGM_KSTEP;  // of the whole panel: A's row pitch in elements
  const uint32_t k0 = split * ksteps * MI355X_DPGM_KSTEP;       // where this workgroup's range starts
  const unsigned char* ag = reinterpret_cast<const unsigned char*>(args.a) +
                            (static_cast<size_t>(tile) * MI355X_DPGM_TILE * K + k0) * sizeof(uint16_t);
  const unsigned char* bg = reinterpret_cast<const unsigned char*>(args.b) + static_cast<size_t>(k0) * 256u;

  // Global byte offsets of this lane's 16 bytes in the wave's four A and four B
  // wave-loads of a step. Wave-load w fills LDS bytes [1024 w, 1024 w + 1024) of
  // the tile, lane l the 16 at 16 l: A rows 8w..8w+7, B rows 4w..4w+3. Which
  // global chunk lands there is the swizzle (dpgm_lds_a / dpsk_lds_b, inverted).
  uint32_t a_off[4], b_off[4];
#pragma unroll
  for (uint32_t t = 0; t < 4; ++t) {
    const uint32_t w = wave * 4u + t;
    const uint32_t row = 8u * w + (lane >> 3), kc = (lane & 7u) ^ ((row >> 1) & 7u);
    a_off[t] = row * K * 2u + kc * 16u;
    const uint32_t k = 4u * w + (lane >> 4), nc = (lane & 15u) ^ dpsk_b_swz(k);
    b_off[t] = k * 256u + nc * 16u;
  }
  const auto issue_loads = [&](unsigned char* lds, uint32_t s) {
    unsigned char* buf = lds + wave * 4096u;
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) {
      __builtin_amdgcn_global_load_lds(MI355X_DPSK_GLOBAL(ag + a_off[t] + s * 128u), MI355X_DPSK_LDS(buf + t * 1024u),
                                       16, 0, 0);
      __builtin_amdgcn_global_load_lds(MI355X_DPSK_GLOBAL(bg + b_off[t] + s * (MI355X_DPGM_KSTEP * 256u)),
                                       MI355X_DPSK_LDS(buf + MI355X_DPGM_LDS_TILE_BYTES + t * 1024u), 16, 0, 0);
    }
  };

  // the wave's sub-tile and this lane's place in its fragments
  const uint32_t row0 = 64u * (wave >> 1), col0 = 64u * (wave & 1u);
  const uint32_t g = lane >> 4;                        // k-group: k 8*g.. of a 32-wide sub-step
  const uint32_t a_row = row0 + (lane & 15u);          // + 16 * rb: (a_row >> 1) & 7 is the same for every rb
  const uint32_t a_swz = (a_row >> 1) & 7u;
  // B, transposed read: this lane addresses row (k) 8*g + 4*h + ((lane&15)>>2), columns 4*(lane&3).. of column block cb
  const uint32_t b_k = 8u * g + ((lane & 15u) >> 2);   // + 32 * kk + 4 * h
  const uint32_t b_n = col0 + 4u * (lane & 3u);        // + 16 * cb

  dpsk_f32x4 acc[4][4];
#pragma unroll
  for (uint32_t rb = 0; rb < 4; ++rb)
#pragma unroll
    for (uint32_t cb = 0; cb < 4; ++cb) acc[rb][cb] = dpsk_f32x4{0.f, 0.f, 0.f, 0.f};

  uint32_t fax = 0, fas = 0, fbx = 0, fbs = 0;
  // one k-step: reads `cur`, which the loads of step s filled, while the loads of step s + 1 fill `nxt`
  const auto step = [&](unsigned char* cur, unsigned char* nxt, uint32_t s) {
    __builtin_amdgcn_s_waitcnt(MI355X_DPSK_WAIT_VM0);  // this wave's loads of step s have landed
    __syncthreads();                                   // and everyone's; everyone has read the other buffer
    if (s + 1u < ksteps) issue_loads(nxt, s + 1u);
    const unsigned char* at = cur;
    const unsigned char* bt = at + MI355X_DPGM_LDS_TILE_BYTES;
#pragma unroll
    for (uint32_t kk = 0; kk < 2; ++kk) {
      dpsk_u32x4 af[4], bf[4];
#pragma unroll
      for (uint32_t rb = 0; rb < 4; ++rb) {
        af[rb] = *reinterpret_cast<const dpsk_u32x4*>(at + (a_row + 16u * rb) * 128u + (((4u * kk + g) ^ a_swz) << 4));
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) dpsk_fold(af[rb][d], fax, fas);
      }
#pragma unroll
      for (uint32_t cb = 0; cb < 4; ++cb) {
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
          const uint32_t k = 32u * kk + 4u * h + b_k, n = b_n + 16u * cb;
          const unsigned char* p = bt + dpsk_lds_b(k, n >> 3) + (n & 7u) * 2u;
          const dpsk_i16x4 q = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) dpsk_i16x4*)(p));
          const dpsk_u32x2 w = __builtin_bit_cast(dpsk_u32x2, q);
          bf[cb][2u * h] = w[0];
          bf[cb][2u * h + 1u] = w[1];
        }
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) dpsk_fold(bf[cb][d], fbx, fbs);
      }
#pragma unroll
      for (uint32_t rb = 0; rb < 4; ++rb)
#pragma unroll
        for (uint32_t cb = 0; cb < 4; ++cb)
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dpsk_bf16x8, af[rb]),
                                                                __builtin_bit_cast(dpsk_bf16x8, bf[cb]), acc[rb][cb], 0, 0, 0);
    }
  };
  issue_loads(lds0, 0);
#pragma unroll 1
  for (uint32_t s = 0; s < ksteps; s += 2u) {
    step(lds0, lds1, s);
    if (s + 1u >= ksteps) break;
    step(lds1, lds0, s + 1u);
  }

  // the tail: this workgroup's partial into D_t, whoever else is adding to the same words
  float* dt = args.d + static_cast<size_t>(tile) * MI355X_DPSK_TILE_WORDS;
#pragma unroll
  for (uint32_t rb = 0; rb < 4; ++rb)
#pragma unroll
    for (uint32_t cb = 0; cb < 4; ++cb)
#pragma unroll
      for (uint32_t r = 0; r < 4; ++r) {
        float v = acc[rb][cb][r];
#if defined(MI355X_TEST_INJECT)
        const bool hit = args.inject_kind != MI355X_DPSK_INJECT_NONE && wg == args.inject_wg && wave == args.inject_wave &&
                         lane == args.inject_lane && (rb * 4u + cb) * 4u + r == args.inject_index;
        if (hit && args.inject_kind == MI355X_DPSK_INJECT_DROP) continue;
        if (hit) v = __uint_as_float(__float_as_uint(v) ^ args.inject_mask);
#endif
        __hip_atomic_fetch_add(dt + (row0 + 16u * rb + 4u * g + r) * MI355X_DPGM_TILE + col0 + 16u * cb + (lane & 15u), v,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }

  atomicXor(&ctr[wave * 4u + 0u], (fax ^ (fax >> 16)) & 0xFFFFu);
  atomicAdd(&ctr[wave * 4u + 1u], fas);
  atomicXor(&ctr[wave * 4u + 2u], (fbx ^ (fbx >> 16)) & 0xFFFFu);
  atomicAdd(&ctr[wave * 4u + 3u], fbs);
  if (lane == 0) ctr[16u + wave] = __builtin_amdgcn_s_getreg(MI355X_DPSK_HWREG_HW_ID);
  __syncthreads();

  // the ledger: waves 0 and 2 read all of the workgroup's A between them, waves 0 and 1 all of its B
  uint32_t* led = args.ledger + static_cast<size_t>(tile) * MI355X_DPSK_LEDGER_WORDS;
  if (tid == MI355X_DPSKLED_ARRIVALS) __hip_atomic_fetch_add(led + tid, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == MI355X_DPSKLED_WHO) __hip_atomic_fetch_xor(led + tid, args.nonce ^ wg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == MI355X_DPSKLED_A_SUM) __hip_atomic_fetch_add(led + tid, ctr[1] + ctr[9], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == MI355X_DPSKLED_A_XOR) __hip_atomic_fetch_xor(led + tid, ctr[0] ^ ctr[8], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == MI355X_DPSKLED_B_SUM) __hip_atomic_fetch_add(led + tid, ctr[3] + ctr[7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == MI355X_DPSKLED_B_XOR) __hip_atomic_fetch_xor(led + tid, ctr[2] ^ ctr[6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  if (tid < MI355X_DPSK_REC_WORDS) {
    uint32_t v = 0;
    if (tid == MI355X_DPSKREC_MAGIC) v = MI355X_DPSK_MAGIC;
    if (tid == MI355X_DPSKREC_WG) v = wg;
    if (tid == MI355X_DPSKREC_NONCE) v = args.nonce ^ wg;
    if (tid == MI355X_DPSKREC_XCC) v = __builtin_amdgcn_s_getreg(MI355X_DPSK_HWREG_XCC_ID) & 0xF;
    if (tid >= MI355X_DPSKREC_HWID && tid < MI355X_DPSKREC_HWID + 4) v = ctr[16u + tid - MI355X_DPSKREC_HWID];
    if (tid == MI355X_DPSKREC_TILES) v = args.tiles;
    if (tid == MI355X_DPSKREC_SPLITS) v = args.splits;
    if (tid == MI355X_DPSKREC_KSTEPS) v = ksteps;
    if (tid >= MI355X_DPSKREC_FOLD && tid < MI355X_DPSKREC_FOLD + 16) v = ctr[tid - MI355X_DPSKREC_FOLD];
    args.records[static_cast<size_t>(wg) * MI355X_DPSK_REC_WORDS + tid] = v;
  }
}

extern "C" __global__ __launch_bounds__(MI355X_DPSK_THREADS) void mi355x_splitk_drain(mi355x_datapath_splitk_args args) {
  const uint32_t tile = blockIdx.x;
  if (!dpsk_sizes_ok(args.tiles, args.splits, args.ksteps) || tile >= args.tiles) return;
  const dpsk_u32x4* src = reinterpret_cast<const dpsk_u32x4*>(args.d) + static_cast<size_t>(tile) * (MI355X_DPSK_TILE_WORDS / 4u);
  dpsk_u32x4* dst = reinterpret_cast<dpsk_u32x4*>(args.out_d) + static_cast<size_t>(tile) * (MI355X_DPSK_TILE_WORDS / 4u);
#pragma unroll 4
  for (uint32_t c = threadIdx.x; c < MI355X_DPSK_TILE_WORDS / 4u; c += MI355X_DPSK_THREADS) dst[c] = src[c];
  if (threadIdx.x < MI355X_DPSK_LEDGER_WORDS / 4u)
    reinterpret_cast<dpsk_u32x4*>(args.out_ledger)[tile * (MI355X_DPSK_LEDGER_WORDS / 4u) + threadIdx.x] =
        reinterpret_cast<const dpsk_u32x4*>(args.ledger)[tile * (MI355X_DPSK_LEDGER_WORDS / 4u) + threadIdx.x];
}
