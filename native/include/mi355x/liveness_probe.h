// Host side of the per-device MFMA liveness probe.
//
// Two launch paths for the same gfx950 code object:
//   * HSA-direct (mi355x_hsa_*): ROCr only, code object loaded from the
//     embedded .hsaco, one AQL kernel-dispatch packet on a private queue,
//     output in fine-grained host memory — exactly one dispatch per probe and
//     no HIP runtime start-up cost. This is what the plugin's health loop and
//     the benchmark's container entrypoint run by default.
//   * HIP (mi355x_probe_*): the same kernel through the HIP runtime, for the
//     in-process `_hip` extension and as a cross-check.
#pragma once

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int ordinal;            // HIP / HSA GPU agent ordinal probed
  int ok;                 // 1 = tile bit-exact, nonce echoed, no runtime error
  int hip_error;          // first hipError_t / hsa_status_t seen (0 = none)
  int mismatches;         // elements differing from the host reference
  uint32_t nonce;
  uint32_t xcc_id;        // HW_REG_XCC_ID of the wave that ran
  uint32_t hw_id;
  int iters;
  int dispatches;         // GPU dispatches issued by this probe
  int kfd_node_id;        // kfd topology node of the agent (-1 if unknown)
  double kernel_us;       // dispatch start->end (HSA profiling) or hipEvent time
  double setup_us;        // code object load + queue/stream + buffers
  double total_us;        // everything for this device, including verify
  // HSA path phases (us): 0 code object load+freeze, 1 queue+signal+buffers
  // (on a helper thread, overlapped with 0), 2 unused, 3 doorbell -> completion
  // signal observed on the host
  double phase_us[4];
  char runtime[8];        // "hsa" | "hip"
  char pci_bus_id[32];    // dddd:bb:dd.f
  char arch[64];          // e.g. "gfx950" / "gfx950:sramecc+:xnack-"
  char name[128];
  char uuid[40];
  int pci_domain, pci_bus, pci_device;
  int cu_count;
  uint64_t total_mem;
  // kept-queue path: the verdict belongs to a dispatch submitted by an earlier
  // probe (1), and how long the current outstanding dispatch has been pending
  int late;
  double pending_s;
  char error[160];
} mi355x_probe_result;

// ---- HIP path -------------------------------------------------------------
int mi355x_probe_device_count(void);
int mi355x_probe_device(int ordinal, uint32_t nonce, int iters, mi355x_probe_result* out);
int mi355x_probe_identify(int ordinal, mi355x_probe_result* out);
// 1 (default): the probe creates its own non-blocking stream; 0: it uses the
// null stream (measurement of what the stream's queue costs a HIP program)
void mi355x_probe_set_stream_mode(int own);
// 1: a probe's stream, events and buffers are kept until mi355x_probe_release()
// instead of freed before it returns -- the container entrypoint reports
// "ready" at the verified tile and tears down after its JSON line is out, as
// the HSA path does (mi355x_hsa_probe_defer_release)
void mi355x_probe_defer_release(int on);
void mi355x_probe_release(void);

// ---- HSA-direct path ------------------------------------------------------
// hsa_init + GPU agent enumeration; returns the number of GPU agents or
// -hsa_status_t. Idempotent.
int mi355x_hsa_probe_init(void);
int mi355x_hsa_probe_device(int ordinal, uint32_t nonce, int iters, double timeout_s, mi355x_probe_result* out);
int mi355x_hsa_probe_identify(int ordinal, mi355x_probe_result* out);
void mi355x_hsa_probe_shutdown(void);
// With defer on, probe resources (queue, executable, buffers) outlive the
// verdict until mi355x_hsa_probe_release(): a caller that reports readiness
// takes teardown off its critical path.
void mi355x_hsa_probe_defer_release(int on);
void mi355x_hsa_probe_release(void);
// With keep on, each device's queue, executable and buffers are created by its
// first probe and reused by every later one (released by shutdown, or dropped
// after a failed probe). A kept probe is one AQL packet: no kfd ioctl, so no
// HWS runlist update that would preempt the queues of the pods on that GPU.
void mi355x_hsa_probe_keep(int on);
// Debug fault injection: flip one bit of output word `word` (0..1023; -1 = off)
// of every later probe on `ordinal` (-1 = all devices) before verification.
// The verdict path (tile compare, JSON, plugin health) sees a wrong MFMA result.
void mi355x_hsa_probe_corrupt(int word, int ordinal);
// Runtime start-up split of the last mi355x_hsa_probe_init (us): dlopen of
// ROCr (its constructors), pre-open of /dev/kfd (on a second thread,
// overlapped with the dlopen), hsa_init, agent enumeration, pool discovery.
void mi355x_hsa_init_phases(double out_us[5]);

// ---- xGMI / PCIe peer probe ------------------------------
// `bytes` of a nonce-derived pattern filled in src's HBM, copied src -> dst
// HBM by the DMA engines over the link between them (`reps` times, best time
// kept), then dst -> host and verified word by word. Link properties are ROCr's
// view of dst's HBM pool from src. src == dst exercises the same path on one
// device (single-GPU boxes).
typedef struct {
  int src, dst;              // HSA GPU agent ordinals
  int ok;
  int hsa_error;
  uint32_t value;            // fill pattern
  int access;                // hsa_amd_memory_pool_access_t of dst HBM from src
  int link_type;             // hsa_amd_link_info_type_t of the first hop (4 = xGMI, 2 = PCIe)
  uint32_t hops;
  uint32_t numa_distance;
  uint32_t link_max_bw_mbps; // ROCr's link bandwidth figure for the first hop
  int reps;
  uint64_t bytes;
  uint64_t mismatches;
  double copy_us_best;
  double gbps_best;
  double total_us;
  char src_bus_id[32];
  char dst_bus_id[32];
  char error[160];
} mi355x_peer_result;

int mi355x_hsa_peer_probe(int src, int dst, uint32_t nonce, uint64_t bytes, int reps, double timeout_s,
                          mi355x_peer_result* out);

// ---- full-chip sweep (every CU of every XCD) --------------------------------
// One workgroup per CU (each holds the CU's whole 160 KiB LDS), all resident
// at once (bounded wait), each checks 4 MFMA tiles against the VALU, writes
// and cross-reads the whole LDS, and reports its XCC / CU ids; the host
// verifies records and wave 0's tiles bit-exactly and counts the distinct
// CUs and XCDs that ran.
typedef struct {
  int ordinal;
  int ok;                 // every record present and correct, every tile exact, all XCDs seen
                          // (XCDs are not counted against num_xcc when the agent reports none)
  int hsa_error;
  uint32_t nonce;
  int iters;
  int grid;               // workgroups launched (= agent CU count)
  int cu_count;           // HSA_AMD_AGENT_INFO_COMPUTE_UNIT_COUNT
  int num_xcc;            // HSA_AMD_AGENT_INFO_NUM_XCC
  int records_ok;         // workgroups whose record is present, echoed the nonce and found no fault
  uint32_t mfma_bad;      // MFMA elements differing from the VALU recomputation (all waves; like
                          // every count below, over present records only)
  uint32_t lds_bad;       // LDS words read back wrong
  uint32_t tile_bad;      // wave-0 tile elements differing from the host reference
  int cus_covered;        // distinct (XCC, SE, SH, CU) that ran a workgroup
  int xccs_covered;
  int all_resident;       // every record ok and every workgroup saw the whole grid resident before working
  int wgs_per_xcc[16];
  double kernel_us;       // dispatch start -> end (HSA profiling)
  double arrival_spread_us;  // first to last workgroup arrival (s_memrealtime), present records
  double total_us;
  // > 0: an earlier sweep on this device has not completed for this long; its
  // queue and buffers stay allocated and no new sweep is submitted (at most one
  // outstanding sweep per device, so a wedged GPU leaks one queue, not one per cadence)
  double in_flight_s;
  int kept_queue;         // ran on the device's kept probe queue (--serve --keep), no queue of its own
  // the agent the check ran on, as in mi355x_probe_result: -1 and "" when the check never reached a device
  int kfd_node_id;
  char pci_bus_id[32];    // dddd:bb:dd.f
  char error[160];
} mi355x_sweep_result;

int mi355x_hsa_chip_sweep(int ordinal, uint32_t nonce, int iters, double timeout_s, mi355x_sweep_result* out);

// ---- throughput check (idle GPUs only: it owns the chip for a few ms) --------
// HBM: fill `bytes` of device memory with an address-derived pattern (write
// bandwidth), read it back and verify every word (read bandwidth). MFMA: two
// register-resident bf16 v_mfma_f32_32x32x16 chains per wave, two waves per
// SIMD on every CU (sustained TFLOP/s), with each workgroup's shader clock
// from s_memtime / s_memrealtime, folded per XCD; every wave's accumulator
// checksum must be bit-identical (same operands everywhere).
typedef struct {
  int ordinal;
  int ok;                    // pattern exact, checksums identical and finite, every record present, all XCDs
                             // ran (not counted against num_xcc when the agent reports none)
  int hsa_error;
  uint32_t nonce;
  uint64_t bytes;
  int cu_count;
  int num_xcc;
  double fill_us;            // kernel times (HSA dispatch profiling)
  double check_us;           // first read pass (right after the fill)
  double check2_us;          // second read pass
  double hbm_write_gbps;
  double hbm_read_gbps;      // from the faster read pass that has a time
  uint64_t hbm_bad_words;    // 32-bit words read back wrong (the pass that found more)
  uint64_t hbm_bad_words_pass2;
  int64_t hbm_first_bad;     // lowest failing 16-byte unit, -1 if none (also when the counter names no unit
                             // of the buffer: the kernels never wrote it, `error` says so)
  int mfma_iters;            // MFMA pairs per wave
  int mfma_grid;             // workgroups (MI355X_BURN_WGS_PER_CU per CU)
  int mfma_records_ok;
  int mfma_checksum_mismatch;  // waves whose checksum word differs from wave 0 of the first present record;
                               // every wave when that word is NaN or Inf (a correct checksum is finite)
  int mfma_xccs;             // distinct XCDs that ran burn workgroups
  double mfma_us;
  double mfma_tflops;        // dense bf16, from the dispatch time
  double clock_mhz_min;      // per-workgroup shader clock during the MFMA loop
  double clock_mhz_median;   // medians here are the upper one: sorted[n / 2]
  double clock_mhz_max;
  double xcd_clock_mhz[16];  // median per XCD (0 = no workgroup with a measurable interval seen)
  double total_us;
  double in_flight_s;        // > 0: an earlier sweep / check on this device has not completed
  int kept_queue;            // ran on the device's kept probe queue (--serve --keep)
  // the agent the check ran on, as in mi355x_probe_result: -1 and "" when the check never reached a device
  int kfd_node_id;
  char pci_bus_id[32];    // dddd:bb:dd.f
  char error[160];
} mi355x_perf_result;

int mi355x_hsa_perf_check(int ordinal, uint32_t nonce, uint64_t bytes, int mfma_iters, double timeout_s,
                          mi355x_perf_result* out);
// Debug fault injection: the fill pass writes 16-byte unit `unit` with its
// first word inverted, so the check pass must report exactly one bad word
// there (UINT64_MAX = off).
void mi355x_hsa_perf_poison(uint64_t unit);

// ---- MFMA datapath check (full-width, bit-exact) ------------------------------
// One straight-line workgroup per CU (no residency wait: where they land is
// reported, not arranged), four waves each, four v_mfma_f32_32x32x2_f32 stages
// per wave on operands whose words toggle all 32 bits of the A, B and C input
// paths and of D, every stage exact by construction. Each wave checks its
// accumulators against a VALU fmaf chain; the host checks wave 0's four tiles
// of every workgroup bit for bit and names the first wrong word.
typedef struct {
  int ordinal;
  int ok;                 // every record present, no device-side mismatch, every tile word exact
  int hsa_error;
  uint32_t nonce;
  int grid;               // workgroups launched (= agent CU count)
  int cu_count;
  int num_xcc;
  int records_ok;         // workgroups whose record is present, echoed the nonce and found no fault
  uint32_t mfma_bad;      // MFMA elements differing from the VALU chain (all waves and stages, present records)
  uint32_t stage_bad[4];  // the same per stage
  uint32_t tile_bad;      // wave-0 tile words differing from the host reference (present records)
  // the first wrong tile word in (workgroup, stage, word) order; -1 / 0 when there is none
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;     // row * 32 + column
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor; // got ^ want: the stuck or flipped bits
  // where the workgroups ran (reported, never required: the kernel does not wait for residency)
  int cus_covered;        // distinct (XCC, SE, SH, CU)
  int simds_covered;      // distinct (XCC, SE, SH, CU, SIMD) over all four waves
  int xccs_covered;
  double kernel_us;       // dispatch start -> end (HSA profiling)
  double total_us;
  double in_flight_s;     // > 0: an earlier sweep / check on this device has not completed
  int kept_queue;         // ran on the device's kept probe queue (--serve --keep)
  // the agent the check ran on, as in mi355x_probe_result: -1 and "" when the check never reached a device
  int kfd_node_id;
  char pci_bus_id[32];    // dddd:bb:dd.f
  char error[160];
} mi355x_datapath_result;

int mi355x_hsa_datapath_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_result* out);
// Debug fault injection: flip bit `bit` of word `word` (0..1023) of workgroup
// 0's stage `stage` tile of every later check on `ordinal` (-1 = all devices)
// before the verdict; stage < 0 = off.
void mi355x_hsa_datapath_corrupt(int stage, int word, int bit, int ordinal);

// ---- int8 MFMA datapath check (128-bit operands, bit-exact) -------------------
// The same shape as the check above (one straight-line workgroup per CU, four
// waves each, no device memory), on the wide operand form: four
// v_mfma_i32_32x32x32_i8 stages and one v_mfma_i32_16x16x64_i8 stage per wave,
// 4-VGPR A and B operands whose words toggle all 32 bits, int32 sums that
// cannot overflow. Each wave checks its accumulators against a v_dot4
// recomputation; the host checks wave 0's five tiles of every workgroup word
// for word and names the first wrong one.
typedef struct {
  int ordinal;
  int ok;                 // every record present, no device-side mismatch, every tile word exact
  int hsa_error;
  uint32_t nonce;
  int grid;               // workgroups launched (= agent CU count)
  int cu_count;
  int num_xcc;
  int records_ok;         // workgroups whose record is present, echoed the nonce and found no fault
  uint32_t mfma_bad;      // MFMA elements differing from the recomputation (all waves and stages, present records)
  uint32_t stage_bad[5];  // the same per stage
  uint32_t tile_bad;      // wave-0 tile words differing from the host reference (present records)
  // the first wrong tile word in (workgroup, stage, word) order; -1 / 0 when there is none
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;     // row * 32 + column (stage 4: row * 16 + column)
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor; // got ^ want: the stuck or flipped bits
  // where the workgroups ran (reported, never required: the kernel does not wait for residency)
  int cus_covered;        // distinct (XCC, SE, SH, CU)
  int simds_covered;      // distinct (XCC, SE, SH, CU, SIMD) over all four waves
  int xccs_covered;
  double kernel_us;       // dispatch start -> end (HSA profiling)
  double total_us;
  double in_flight_s;     // > 0: an earlier sweep / check on this device has not completed
  int kept_queue;         // ran on the device's kept probe queue (--serve --keep)
  // the agent the check ran on, as in mi355x_probe_result: -1 and "" when the check never reached a device
  int kfd_node_id;
  char pci_bus_id[32];    // dddd:bb:dd.f
  char error[160];
} mi355x_datapath_i8_result;

int mi355x_hsa_datapath_i8_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_i8_result* out);
// Debug fault injection: flip bit `bit` of word `word` (0..1023; stage 4:
// 0..255) of workgroup 0's stage `stage` tile of every later int8 check on
// `ordinal` (-1 = all devices) before the verdict; stage < 0 = off.
void mi355x_hsa_datapath_i8_corrupt(int stage, int word, int bit, int ordinal);

// ---- bf16 MFMA datapath check (128-bit operands, bit-exact) -------------------
// The same shape again, on the instructions pods mostly run: four
// v_mfma_f32_32x32x16_bf16 stages and one v_mfma_f32_16x16x32_bf16 stage per
// wave, with operands chosen so that every product and every partial sum, in
// any order, is an exact f32 (datapath_bf16_kernel.h). Each wave checks its
// accumulators, as words, against a VALU fmaf recomputation; the host checks
// wave 0's five tiles of every workgroup word for word. The result has the
// int8 check's fields with the same meaning (mfma_bad counts f32 words).
typedef mi355x_datapath_i8_result mi355x_datapath_bf16_result;

int mi355x_hsa_datapath_bf16_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_bf16_result* out);
// Debug fault injection, as mi355x_hsa_datapath_i8_corrupt, for every later bf16 check.
void mi355x_hsa_datapath_bf16_corrupt(int stage, int word, int bit, int ordinal);

// ---- fp8 / MX-scaled MFMA datapath check (64- and 256-bit operands, bit-exact) --
// The same shape once more, on the 8-bit float part of the matrix core: three
// v_mfma_f32_32x32x16_{fp8,bf8}_{fp8,bf8} stages, one
// v_mfma_f32_16x16x32_bf8_fp8 stage, three v_mfma_scale_f32_32x32x64_f8f6f4
// stages and one v_mfma_scale_f32_16x16x128_f8f6f4 stage per wave, on e4m3 /
// e5m2 operands and E8M0 scales for which every product and every partial sum,
// in any order, is an exact f32 (datapath_fp8_kernel.h). Each wave checks its
// accumulators, as words, against a VALU fmaf recomputation; the host checks
// wave 0's eight tiles of every workgroup word for word. The fields have the
// int8 check's meanings (mfma_bad counts f32 words); stage_bad has 8 entries.
typedef struct {
  int ordinal;
  int ok;
  int hsa_error;
  uint32_t nonce;
  int grid;
  int cu_count;
  int num_xcc;
  int records_ok;
  uint32_t mfma_bad;
  uint32_t stage_bad[8];
  uint32_t tile_bad;
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;     // row * 32 + column (stages 3 and 7: row * 16 + column)
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor;
  int cus_covered;
  int simds_covered;
  int xccs_covered;
  double kernel_us;
  double total_us;
  double in_flight_s;
  int kept_queue;
  int kfd_node_id;
  char pci_bus_id[32];
  char error[160];
} mi355x_datapath_fp8_result;

int mi355x_hsa_datapath_fp8_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_fp8_result* out);
// Debug fault injection, as mi355x_hsa_datapath_i8_corrupt, for every later fp8 check (stage 0..7).
void mi355x_hsa_datapath_fp8_corrupt(int stage, int word, int bit, int ordinal);

// ---- f16 MFMA datapath check (128- and 64-bit operands, bit-exact) -------------
// The same shape for IEEE half operands: three one-hot stages, one sum stage of
// v_mfma_f32_32x32x16_f16, and one sum stage each of v_mfma_f32_16x16x32_f16
// and the legacy 64-bit-operand forms v_mfma_f32_32x32x8_f16 and
// v_mfma_f32_16x16x16_f16 per wave, on operands for which every product and
// every partial sum, in any order, is an exact f32 (datapath_f16_kernel.h).
// Each wave checks its accumulators, as words, against a VALU fmaf
// recomputation; the host checks wave 0's seven tiles of every workgroup word
// for word. The fields have the int8 check's meanings (mfma_bad counts f32
// words); stage_bad has 7 entries.
typedef struct {
  int ordinal;
  int ok;
  int hsa_error;
  uint32_t nonce;
  int grid;
  int cu_count;
  int num_xcc;
  int records_ok;
  uint32_t mfma_bad;
  uint32_t stage_bad[7];
  uint32_t tile_bad;
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;     // row * 32 + column (stages 4 and 6: row * 16 + column)
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor;
  int cus_covered;
  int simds_covered;
  int xccs_covered;
  double kernel_us;
  double total_us;
  double in_flight_s;
  int kept_queue;
  int kfd_node_id;
  char pci_bus_id[32];
  char error[160];
} mi355x_datapath_f16_result;

int mi355x_hsa_datapath_f16_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_f16_result* out);
// Debug fault injection, as mi355x_hsa_datapath_i8_corrupt, for every later f16 check (stage 0..6).
void mi355x_hsa_datapath_f16_corrupt(int stage, int word, int bit, int ordinal);

// ---- f64 MFMA datapath check (64-bit operands and accumulators, bit-exact) -----
// The same shape for doubles: nine v_mfma_f64_16x16x4_f64 (two one-hot stages
// of two passes, the second on complemented operands, a stage whose outputs
// are exact 53-bit products, a sum stage, and the three neg forms of a sum
// stage) and three v_mfma_f64_4x4x4_4b_f64 per wave, on operands for which
// every product and every partial sum, in any order, is an exact double
// (datapath_f64_kernel.h). Each wave checks its accumulators, as 32-bit words,
// against a VALU fma recomputation; the host checks wave 0's twelve tiles of
// every workgroup word for word in integer arithmetic. The fields have the int8
// check's meanings (mfma_bad counts 32-bit words); stage_bad has 7 entries.
typedef struct {
  int ordinal;
  int ok;
  int hsa_error;
  uint32_t nonce;
  int grid;
  int cu_count;
  int num_xcc;
  int records_ok;
  uint32_t mfma_bad;
  uint32_t stage_bad[7];
  uint32_t tile_bad;
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;     // within the stage: (tile * doubles of a tile + double) * 2 + high word
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor;
  int cus_covered;
  int simds_covered;
  int xccs_covered;
  double kernel_us;
  double total_us;
  double in_flight_s;
  int kept_queue;
  int kfd_node_id;
  char pci_bus_id[32];
  char error[160];
} mi355x_datapath_f64_result;

int mi355x_hsa_datapath_f64_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_f64_result* out);
// Debug fault injection, as mi355x_hsa_datapath_i8_corrupt, for every later f64 check (stage 0..6).
void mi355x_hsa_datapath_f64_corrupt(int stage, int word, int bit, int ordinal);

// ---- fp6 / fp4 MX-scaled MFMA datapath check (192- and 128-bit operands, bit-exact) -----
// The same shape for the narrow formats of the MX-scaled forms: six
// v_mfma_scale_f32_32x32x64_f8f6f4 and two v_mfma_scale_f32_16x16x128_f8f6f4
// per wave with e2m3, e3m2 and e2m1 operands of 6 and 4 dwords (and e4m3 by
// e2m1, the MXFP4-weights pairing), four one-hot stages and four product stages
// on operands and E8M0 scales for which every partial sum, in any order, is an
// exact f32 (datapath_f6f4_kernel.h). Each wave checks its accumulators, as
// words, against a VALU fmaf recomputation over integer-decoded operands; the
// host checks wave 0's eight tiles of every workgroup word for word. The fields
// have the int8 check's meanings; stage_bad has 8 entries.
typedef struct {
  int ordinal;
  int ok;
  int hsa_error;
  uint32_t nonce;
  int grid;
  int cu_count;
  int num_xcc;
  int records_ok;
  uint32_t mfma_bad;
  uint32_t stage_bad[8];
  uint32_t tile_bad;
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;     // row * dim + col of the stage's tile
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor;
  int cus_covered;
  int simds_covered;
  int xccs_covered;
  double kernel_us;
  double total_us;
  double in_flight_s;
  int kept_queue;
  int kfd_node_id;
  char pci_bus_id[32];
  char error[160];
} mi355x_datapath_f6f4_result;

int mi355x_hsa_datapath_f6f4_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_f6f4_result* out);
// Debug fault injection, as mi355x_hsa_datapath_i8_corrupt, for every later f6f4 check (stage 0..7).
void mi355x_hsa_datapath_f6f4_corrupt(int stage, int word, int bit, int ordinal);

// ---- sparse (2:4) MFMA datapath check (index operand and B selection, bit-exact) -----
// The same shape for the structured-sparsity instructions, which no other check
// issues: ten v_smfmac_* per wave -- v_smfmac_f32_32x32x32_f16 (four stages),
// 16x16x64_f16, 32x32x32_bf16, 16x16x64_bf16, v_smfmac_i32_32x32x64_i8,
// 16x16x128_i8 and v_smfmac_f32_32x32x64_fp8_bf8 -- on a compressed A, its index
// register and a dense B: four selection stages, whose every output names the
// row of B the index picked, and six sum stages on operands for which every
// partial sum, in any order, is exact (datapath_sparse_kernel.h). Each wave
// checks its accumulators, as words, against a VALU recomputation that walks the
// compressed elements and picks B's row through the same index words; the host
// checks wave 0's ten tiles of every workgroup word for word. The fields have
// the int8 check's meanings; stage_bad has 10 entries.
typedef struct {
  int ordinal;
  int ok;
  int hsa_error;
  uint32_t nonce;
  int grid;
  int cu_count;
  int num_xcc;
  int records_ok;
  uint32_t mfma_bad;
  uint32_t stage_bad[10];
  uint32_t tile_bad;
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;     // row * dim + col of the stage's tile
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor;
  int cus_covered;
  int simds_covered;
  int xccs_covered;
  double kernel_us;
  double total_us;
  double in_flight_s;
  int kept_queue;
  int kfd_node_id;
  char pci_bus_id[32];
  char error[160];
} mi355x_datapath_sparse_result;

int mi355x_hsa_datapath_sparse_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_sparse_result* out);
// Debug fault injection, as mi355x_hsa_datapath_i8_corrupt, for every later sparse check (stage 0..9).
void mi355x_hsa_datapath_sparse_corrupt(int stage, int word, int bit, int ordinal);

// ---- bf16 GEMM pipeline check (HBM to LDS to MFMA chains, bit-exact) -----
// The datapath checks above build operands in registers and issue one MFMA per
// stage. This one is a small real GEMM (datapath_gemm_kernel.h): mi355x_gemm_fill
// writes a bf16 A panel per workgroup and one shared B panel into device memory,
// and mi355x_mfma_datapath_gemm, one workgroup per CU, moves them into LDS with
// the direct-to-LDS loads (global_load_lds_dwordx4), out of it with 128-bit and
// transposed (ds_read_b64_tr_b16) reads, and through dependent chains of
// 4 * ksteps v_mfma_f32_32x32x16_bf16 per accumulator while the next tile's
// loads are in flight. The operands make every partial sum exact in any order,
// so the host checks every D word exactly (datapath_gemm_verify.h) and, per wave,
// a fold of the fragments that came out of LDS. stage_bad: wrong fold words of
// the A feed, of the B feed, wrong D words; mfma_bad = the feeds' sum, tile_bad
// = the D words. first_bad_word: the wave's fold word (wave * 2 + {xor, sum})
// for stages 0 and 1, row * 128 + column for stage 2.
typedef struct {
  int ordinal;
  int ok;
  int hsa_error;
  uint32_t nonce;
  int grid;
  int ksteps;             // K / 64
  int cu_count;
  int num_xcc;
  int records_ok;
  uint32_t mfma_bad;
  uint32_t stage_bad[3];
  uint32_t tile_bad;
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor;
  int cus_covered;
  int simds_covered;
  int xccs_covered;
  double fill_us;         // GPU time of mi355x_gemm_fill
  double kernel_us;       // GPU time of mi355x_mfma_datapath_gemm
  double verify_us;       // host time of the verdict
  double total_us;
  double in_flight_s;
  int kept_queue;
  int kfd_node_id;
  char pci_bus_id[32];
  char error[160];
} mi355x_datapath_gemm_result;

int mi355x_hsa_datapath_gemm_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_gemm_result* out);
// Debug fault injection, as mi355x_hsa_datapath_i8_corrupt, for every later GEMM check: bit `bit` of word `word` of
// workgroup 0's stage-`stage` data (0: A fold word, 1: B fold word, 2: D word) is flipped before the verdict.
void mi355x_hsa_datapath_gemm_corrupt(int stage, int word, int bit, int ordinal);

// ---- split-K GEMM check (partial tiles summed by L2 atomics, bit-exact) ----
// In the checks above a workgroup writes only words no other workgroup touches.
// Here (datapath_splitk_kernel.h) cu_count / 8 tiles of 128 x 128 are each
// computed by 8 workgroups, one per eighth of K = 2048, on the GEMM check's
// operands: mi355x_splitk_fill writes A, B, D = C and a zeroed ledger into device
// memory; mi355x_mfma_datapath_splitk computes each partial through chains of
// v_mfma_f32_16x16x32_bf16 and adds it into D with no-return, agent-scope
// global_atomic_add_f32, and updates the tile's ledger with global_atomic_add /
// global_atomic_xor; mi355x_splitk_drain copies D and the ledgers to host memory.
// Every sum is exact in any arrival order, so the host checks every D word
// exactly (datapath_splitk_verify.h). stage_bad: wrong fold words of the A feed,
// of the B feed, wrong D words, wrong ledger words; mfma_bad = the feeds' sum,
// tile_bad = the D words, ledger_bad = the ledger words; records_ok counts exact
// tiles and first_bad_wg names a tile. first_bad_word: wg * 8 + wave * 2 +
// {xor, sum} for stages 0 and 1, tile * 16384 + row * 128 + column for stage 2,
// tile * 8 + ledger word for stage 3.
typedef struct {
  int ordinal;
  int ok;
  int hsa_error;
  uint32_t nonce;
  int grid;               // tiles * splits workgroups
  int tiles;
  int splits;
  int ksteps;             // k-steps of 64 a workgroup
  int cu_count;
  int num_xcc;
  int records_ok;
  uint32_t mfma_bad;
  uint32_t stage_bad[4];
  uint32_t tile_bad;
  uint32_t ledger_bad;
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor;
  int cus_covered;
  int simds_covered;
  int xccs_covered;
  int xccs_per_tile_min;  // the fewest distinct XCDs among one tile's contributors: reported, not judged
  double fill_us;         // GPU time of mi355x_splitk_fill
  double kernel_us;       // GPU time of mi355x_mfma_datapath_splitk
  double drain_us;        // GPU time of mi355x_splitk_drain
  double verify_us;       // host time of the verdict
  double total_us;
  double in_flight_s;
  int kept_queue;
  int kfd_node_id;
  char pci_bus_id[32];
  char error[160];
} mi355x_datapath_splitk_result;

int mi355x_hsa_datapath_splitk_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_splitk_result* out);
// Debug fault injection, as mi355x_hsa_datapath_i8_corrupt, for every later split-K check: bit `bit` of word `word`
// (numbered as first_bad_word) of the stage-`stage` data is flipped before the verdict.
void mi355x_hsa_datapath_splitk_corrupt(int stage, int word, int bit, int ordinal);

// ---- fused attention check (MFMA, online softmax, MFMA; bit-exact) ----
// The checks above cover what a tenant's GEMM does. Here (datapath_attn_kernel.h)
// cu_count / 4 heads of 256 keys and 512 queries, d = 64, go through a
// flash-attention loop: mi355x_attn_fill writes Q, K and V into device memory;
// mi355x_mfma_datapath_attn computes S^T = K . Q^T by v_mfma_f32_32x32x16_bf16,
// the running row max (v_max3_f32, v_permlane32_swap), P = v_exp_f32(S - m) packed
// by v_cvt_pk_bf16_f32 and moved across the half-waves by v_permlane32_swap into
// the B operand of O^T += V^T . P^T, with O and l rescaled by v_ldexp_f32 between
// the MFMAs. Every m, l and O word is exact in any order, so the host checks
// every one (datapath_attn_verify.h). stage_bad: wrong fold words of the K feed,
// of the V feed, wrong m / l words, wrong O words; mfma_bad = the feeds' sum,
// tile_bad = the m / l and O words; records_ok counts exact workgroups.
// first_bad_word: wg * 8 + wave * 2 + {xor, sum} for stages 0 and 1,
// wg * 256 + query * 2 + {m, l} for stage 2, wg * 8192 + query * 64 + d for stage 3.
typedef struct {
  int ordinal;
  int ok;
  int hsa_error;
  uint32_t nonce;
  int grid;               // heads * qblocks workgroups
  int heads;
  int qblocks;            // blocks of 128 queries a head
  int kblocks;            // blocks of 64 keys a head
  int cu_count;
  int num_xcc;
  int records_ok;
  uint32_t mfma_bad;
  uint32_t stage_bad[4];
  uint32_t tile_bad;
  uint32_t exp_inexact;   // v_exp_f32 results that were not exact powers of two: reported, not judged
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor;
  int cus_covered;
  int simds_covered;
  int xccs_covered;
  double fill_us;         // GPU time of mi355x_attn_fill
  double kernel_us;       // GPU time of mi355x_mfma_datapath_attn
  double verify_us;       // host time of the verdict
  double total_us;
  double in_flight_s;
  int kept_queue;
  int kfd_node_id;
  char pci_bus_id[32];
  char error[160];
} mi355x_datapath_attn_result;

int mi355x_hsa_datapath_attn_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_attn_result* out);
// Debug fault injection, as mi355x_hsa_datapath_i8_corrupt, for every later attention check: bit `bit` of word `word`
// (numbered as first_bad_word) of the stage-`stage` data is flipped before the verdict.
void mi355x_hsa_datapath_attn_corrupt(int stage, int word, int bit, int ordinal);

// ---- MXFP4 GEMM pipeline check (scaled-MFMA chains from HBM, bit-exact) ----
// The GEMM checks above are bf16. Here (datapath_mxgemm_kernel.h) mi355x_mxgemm_fill
// writes a packed e2m1 A panel and its E8M0 block scales per workgroup, and one
// shared K-major B panel with its scales, into device memory;
// mi355x_mfma_datapath_mxgemm, one workgroup per CU, moves the operands into LDS
// with global_load_lds_dwordx4 and out of it with ds_read_b128 (one read is one
// lane's 32-element fragment, one scale block), loads the scale bytes into
// registers a step ahead, gathers them with v_perm_b32, and runs dependent chains
// of 4 * ksteps v_mfma_scale_f32_32x32x64_f8f6f4 per accumulator, each with its
// own op_sel byte of the scale VGPRs. Every D word is exact in any order, so the
// host checks every one (datapath_mxgemm_verify.h) and, per wave, a fold of the
// fragments and of the scale VGPRs. stage_bad: wrong fold words of the A feed,
// of the B feed, of the scale feed, wrong D words; mfma_bad = the three feeds'
// sum, tile_bad = the D words; records_ok counts exact workgroups.
// first_bad_word: wg * 16 + wave * 2 + {xor, sum} for stages 0, 1 and 2,
// wg * 16384 + row * 128 + column for stage 3.
typedef struct {
  int ordinal;
  int ok;
  int hsa_error;
  uint32_t nonce;
  int grid;
  int ksteps;             // K / 256
  int cu_count;
  int num_xcc;
  int records_ok;
  uint32_t mfma_bad;
  uint32_t stage_bad[4];
  uint32_t tile_bad;
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor;
  int cus_covered;
  int simds_covered;
  int xccs_covered;
  double fill_us;         // GPU time of mi355x_mxgemm_fill
  double kernel_us;       // GPU time of mi355x_mfma_datapath_mxgemm
  double verify_us;       // host time of the verdict
  double total_us;
  double in_flight_s;
  int kept_queue;
  int kfd_node_id;
  char pci_bus_id[32];
  char error[160];
} mi355x_datapath_mxgemm_result;

int mi355x_hsa_datapath_mxgemm_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_mxgemm_result* out);
// Debug fault injection, as mi355x_hsa_datapath_i8_corrupt, for every later MXFP4 GEMM check: bit `bit` of word `word`
// (numbered as first_bad_word) of the stage-`stage` data is flipped before the verdict.
void mi355x_hsa_datapath_mxgemm_corrupt(int stage, int word, int bit, int ordinal);

// ---- MX quantise check (MFMA, scaled convert, scaled MFMA, bit-exact) ----
// The checks above take their e2m1 operands and E8M0 scales ready-made. Here
// (datapath_mxquant_kernel.h) mi355x_mxquant_fill writes a bf16 token panel X per
// workgroup and shared W1 (bf16), W2 (packed e2m1, K-major) and W2's scale bytes;
// mi355x_mfma_datapath_mxquant, one workgroup per CU, runs a two-layer MLP tile:
// per slab of 128 hidden columns H^T = W1 . X^T by v_mfma_f32_32x32x16_bf16, the
// absolute maximum of each 32-wide block (v_max3_f32, v_permlane32_swap), the
// E8M0 byte from its exponent field, v_cvt_scalef32_pk_fp4_f32 to packed e2m1,
// an LDS round trip, and Y += Q . W2^T by v_mfma_scale_f32_32x32x64_f8f6f4 with
// the block scales just made. Every code, scale byte and Y word is exact, so the
// host checks every one (datapath_mxquant_verify.h). stage_bad: wrong fold words
// of the W1 feed, of the W2 and scale feed, wrong dwords of the quantised image,
// wrong Y words; mfma_bad = the two feeds' sum, tile_bad = the Y words;
// records_ok counts exact workgroups. first_bad_word: wg * 16 + wave * 2 +
// {xor, sum} for stage 0, wg * 16 + wave * 4 + {W2 xor, W2 sum, scale xor, scale
// sum} for stage 1, wg * 2176 * hsteps + dword for stage 2, wg * 16384 + row *
// 128 + column for stage 3.
typedef struct {
  int ordinal;
  int ok;
  int hsa_error;
  uint32_t nonce;
  int grid;
  int hsteps;             // hidden / 128
  int cu_count;
  int num_xcc;
  int records_ok;
  uint32_t mfma_bad;
  uint32_t stage_bad[4];
  uint32_t tile_bad;
  int first_bad_wg;
  int first_bad_stage;
  int first_bad_word;
  uint32_t first_bad_got;
  uint32_t first_bad_want;
  uint32_t first_bad_xor;
  int cus_covered;
  int simds_covered;
  int xccs_covered;
  double fill_us;         // GPU time of mi355x_mxquant_fill
  double kernel_us;       // GPU time of mi355x_mfma_datapath_mxquant
  double verify_us;       // host time of the verdict
  double total_us;
  double in_flight_s;
  int kept_queue;
  int kfd_node_id;
  char pci_bus_id[32];
  char error[160];
} mi355x_datapath_mxquant_result;

int mi355x_hsa_datapath_mxquant_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_mxquant_result* out);
// Debug fault injection, as mi355x_hsa_datapath_i8_corrupt, for every later MX quantise check: bit `bit` of word `word`
// (numbered as first_bad_word) of the stage-`stage` data is flipped before the verdict.
void mi355x_hsa_datapath_mxquant_corrupt(int stage, int word, int bit, int ordinal);

#ifdef __cplusplus
}
#endif
