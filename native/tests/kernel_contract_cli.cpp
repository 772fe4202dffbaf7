// Host-only view of the kernel contract in liveness_kernel.h, of
// probe_verify.h::verify_tile and of the chip_verify.h verdicts, for
// tests/test_kernel_reference.py and tests/test_verdict_reference.py: the
// operand generators at given indices, the layout of the four kernel-argument
// structs, and the host's verdict on tiles and records read from stdin, printed
// as the probe prints it (probe_json.h). No HIP, no GPU.
//
//   kernel_contract_cli gen     < requests    one value per request line:
//        a i k nonce | b k j nonce | c i j nonce | sweep_nonce nonce wg wave |
//        lds i nonce wg | hbm word seed | burn lane j nonce
//   kernel_contract_cli layout                "struct field offset" / "struct sizeof n" lines
//   kernel_contract_cli inject-layout         "define NAME n" lines of the iteration bound and the injection
//        contract and, when compiled with -DMI355X_TEST_INJECT=1 (as the test-only code object is),
//        mi355x_sweep_args with its trailing injection fields, as `layout` prints a struct
//   kernel_contract_cli verify  < records     one "ok mismatches error" line per binary record:
//        uint32 nonce, int32 iters, 1024 floats, 4 meta words
//   kernel_contract_cli sweep-verdict < cases  sweep_json lines of mi355x::sweep_verdict. A case:
//        uint32 grid, nonce, int32 iters, num_xcc, uint32 variants; grid*16 record words; grid*1024 floats;
//        then per variant: uint32 n and n patches (uint32 array, index, value), array 0 = records,
//        1 = tiles as words. One line for the case as given, then one per variant: the case with
//        that variant's words replaced (each variant starts from the case as given).
//   kernel_contract_cli perf-verdict < cases   perf_json lines of mi355x::perf_verdict. A case:
//        uint32 burn_wgs, nonce, int32 num_xcc, mfma_iters, uint64 bytes, double fill_us, check_us,
//        check2_us, mfma_us, uint32 variants, pad; 4 counter words; burn_wgs*16 record words; variants
//        as above, array 0 = records, 1 = counters.
//   kernel_contract_cli json sweep|perf I U32 U64 I64 D ERRHEX
//        the JSON of a result whose every int is I, uint32_t U32, uint64_t U64, int64_t I64, double D
//        and whose error is the bytes ERRHEX names (at most 159), pci_bus_id the first 31 of them
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "chip_verify.h"
#include "liveness_kernel.h"
#include "probe_json.h"
#include "probe_verify.h"

static int cmd_gen() {
  char line[256];
  while (std::fgets(line, sizeof(line), stdin)) {
    char name[32];
    unsigned long long x = 0, y = 0, z = 0;
    const int n = std::sscanf(line, "%31s %llu %llu %llu", name, &x, &y, &z);
    if (n < 1) continue;
    const std::string g = name;
    if (g == "a" && n == 4) {
      std::printf("%d\n", (int)probe_a((int)x, (int)y, (uint32_t)z));
    } else if (g == "b" && n == 4) {
      std::printf("%d\n", (int)probe_b((int)x, (int)y, (uint32_t)z));
    } else if (g == "c" && n == 4) {
      std::printf("%d\n", (int)probe_c((int)x, (int)y, (uint32_t)z));
    } else if (g == "sweep_nonce" && n == 4) {
      std::printf("%" PRIu32 "\n", sweep_nonce((uint32_t)x, (uint32_t)y, (uint32_t)z));
    } else if (g == "lds" && n == 4) {
      std::printf("%" PRIu32 "\n", sweep_lds_pattern((uint32_t)x, (uint32_t)y, (uint32_t)z));
    } else if (g == "hbm" && n == 3) {
      std::printf("%" PRIu32 "\n", hbm_pattern((uint64_t)x, (uint32_t)y));
    } else if (g == "burn" && n == 4) {
      std::printf("%u\n", (unsigned)burn_bf16_bits((uint32_t)x, (uint32_t)y, (uint32_t)z));
    } else {
      std::fprintf(stderr, "bad gen request: %s", line);
      return 2;
    }
  }
  return 0;
}

#define FIELD(S, F) std::printf("%s %s %zu\n", #S, #F, offsetof(S, F))
#define SIZE(S) std::printf("%s sizeof %zu\n", #S, sizeof(S))

static int cmd_layout() {
  FIELD(mi355x_liveness_args, out);
  FIELD(mi355x_liveness_args, meta);
  FIELD(mi355x_liveness_args, scratch);
  FIELD(mi355x_liveness_args, nonce);
  FIELD(mi355x_liveness_args, iters);
  SIZE(mi355x_liveness_args);
  FIELD(mi355x_sweep_args, records);
  FIELD(mi355x_sweep_args, tiles);
  FIELD(mi355x_sweep_args, arrive);
  FIELD(mi355x_sweep_args, nonce);
  FIELD(mi355x_sweep_args, iters);
  FIELD(mi355x_sweep_args, grid);
  FIELD(mi355x_sweep_args, wait_ticks);
  SIZE(mi355x_sweep_args);
  FIELD(mi355x_hbm_args, buf);
  FIELD(mi355x_hbm_args, n16);
  FIELD(mi355x_hbm_args, bad);
  FIELD(mi355x_hbm_args, first_bad);
  FIELD(mi355x_hbm_args, threads);
  FIELD(mi355x_hbm_args, poison_unit);
  FIELD(mi355x_hbm_args, seed);
  FIELD(mi355x_hbm_args, pad);
  SIZE(mi355x_hbm_args);
  FIELD(mi355x_burn_args, records);
  FIELD(mi355x_burn_args, hbm_counters);
  FIELD(mi355x_burn_args, hbm_counters_host);
  FIELD(mi355x_burn_args, nonce);
  FIELD(mi355x_burn_args, iters);
  SIZE(mi355x_burn_args);
  return 0;
}

#define DEFINE(N) std::printf("define %s %llu\n", #N, static_cast<unsigned long long>(N))

static int cmd_inject_layout() {
#if defined(MI355X_TEST_INJECT)
  FIELD(mi355x_sweep_args, records);
  FIELD(mi355x_sweep_args, tiles);
  FIELD(mi355x_sweep_args, arrive);
  FIELD(mi355x_sweep_args, nonce);
  FIELD(mi355x_sweep_args, iters);
  FIELD(mi355x_sweep_args, grid);
  FIELD(mi355x_sweep_args, wait_ticks);
  FIELD(mi355x_sweep_args, inject_kind);
  FIELD(mi355x_sweep_args, inject_wg);
  FIELD(mi355x_sweep_args, inject_wave);
  FIELD(mi355x_sweep_args, inject_lane);
  FIELD(mi355x_sweep_args, inject_index);
  FIELD(mi355x_sweep_args, inject_mask);
  SIZE(mi355x_sweep_args);
#endif
  DEFINE(MI355X_PROBE_MAX_ITERS);
  DEFINE(MI355X_SWEEP_THREADS);
  DEFINE(MI355X_SWEEP_LDS_WORDS);
  DEFINE(MI355X_INJECT_NONE);
  DEFINE(MI355X_INJECT_MFMA);
  DEFINE(MI355X_INJECT_LDS);
  return 0;
}

static int cmd_verify() {
  struct {
    uint32_t nonce;
    int32_t iters;
    float out[MI355X_PROBE_OUT];
    uint32_t meta[MI355X_META_WORDS];
  } rec;
  size_t got;
  while ((got = std::fread(&rec, 1, sizeof(rec), stdin)) == sizeof(rec)) {
    mi355x_probe_result r;
    std::memset(&r, 0, sizeof(r));
    mi355x::verify_tile(rec.out, rec.meta, rec.nonce, rec.iters, &r);
    std::printf("%d\t%d\t%s\n", r.ok, r.mismatches, r.error);
  }
  if (got != 0) {
    std::fprintf(stderr, "truncated verify record: %zu of %zu bytes\n", got, sizeof(rec));
    return 2;
  }
  return 0;
}

static constexpr uint32_t kMaxWgs = 4096;   // mi355x_hsa_chip_sweep refuses more than 1024 CUs

template <typename T>
static bool read_n(T* dst, size_t n) {
  return std::fread(dst, sizeof(T), n, stdin) == n;
}

struct Patch {
  uint32_t array, index, value;
};

// One variant's patches applied to arrays[0] / arrays[1] (as 32-bit words of
// the given lengths), `run` called, and the words put back.
template <typename F>
static bool with_variant(uint32_t* const arrays[2], const size_t lens[2], F run) {
  uint32_t n = 0;
  if (!read_n(&n, 1) || n > (1u << 24)) return false;
  std::vector<Patch> patches(n);
  if (n && !read_n(patches.data(), n)) return false;
  std::vector<uint32_t> saved(n);
  for (uint32_t i = 0; i < n; ++i) {
    const Patch& p = patches[i];
    if (p.array > 1 || p.index >= lens[p.array]) return false;
    saved[i] = arrays[p.array][p.index];
    arrays[p.array][p.index] = p.value;
  }
  run();
  for (uint32_t i = n; i-- > 0;) arrays[patches[i].array][patches[i].index] = saved[i];
  return true;
}

static int cmd_sweep_verdict() {
  struct {
    uint32_t grid, nonce;
    int32_t iters, num_xcc;
    uint32_t variants;
  } h;
  size_t got;
  while ((got = std::fread(&h, 1, sizeof(h), stdin)) == sizeof(h)) {
    if (h.grid == 0 || h.grid > kMaxWgs) {
      std::fprintf(stderr, "sweep case: grid %u\n", h.grid);
      return 2;
    }
    std::vector<uint32_t> records(static_cast<size_t>(h.grid) * MI355X_SWEEP_REC_WORDS);
    std::vector<uint32_t> tiles(static_cast<size_t>(h.grid) * MI355X_PROBE_OUT);
    if (!read_n(records.data(), records.size()) || !read_n(tiles.data(), tiles.size())) {
      std::fprintf(stderr, "truncated sweep case\n");
      return 2;
    }
    auto run = [&] {
      mi355x_sweep_result r;
      std::memset(&r, 0, sizeof(r));
      r.kfd_node_id = -1;  // records handed over by a test: no agent
      r.nonce = h.nonce;
      r.iters = h.iters;
      r.num_xcc = h.num_xcc;
      r.grid = static_cast<int>(h.grid);
      std::vector<float> f(tiles.size());
      std::memcpy(f.data(), tiles.data(), tiles.size() * sizeof(float));
      mi355x::sweep_verdict(records.data(), f.data(), h.grid, &r);
      std::printf("%s\n", mi355x::sweep_json(r).c_str());
    };
    run();
    uint32_t* const arrays[2] = {records.data(), tiles.data()};
    const size_t lens[2] = {records.size(), tiles.size()};
    for (uint32_t v = 0; v < h.variants; ++v)
      if (!with_variant(arrays, lens, run)) {
        std::fprintf(stderr, "bad sweep variant %u\n", v);
        return 2;
      }
  }
  if (got != 0) {
    std::fprintf(stderr, "truncated sweep header: %zu bytes\n", got);
    return 2;
  }
  return 0;
}

static int cmd_perf_verdict() {
  struct {
    uint32_t burn_wgs, nonce;
    int32_t num_xcc, mfma_iters;
    uint64_t bytes;
    double fill_us, check_us, check2_us, mfma_us;
    uint32_t variants, pad;
  } h;
  static_assert(sizeof(h) == 64, "perf case header");
  size_t got;
  while ((got = std::fread(&h, 1, sizeof(h), stdin)) == sizeof(h)) {
    if (h.burn_wgs == 0 || h.burn_wgs > kMaxWgs) {
      std::fprintf(stderr, "perf case: burn_wgs %u\n", h.burn_wgs);
      return 2;
    }
    std::vector<uint32_t> counters(4);
    std::vector<uint32_t> records(static_cast<size_t>(h.burn_wgs) * MI355X_PERF_REC_WORDS);
    if (!read_n(counters.data(), 4) || !read_n(records.data(), records.size())) {
      std::fprintf(stderr, "truncated perf case\n");
      return 2;
    }
    auto run = [&] {
      mi355x_perf_result r;
      std::memset(&r, 0, sizeof(r));
      r.kfd_node_id = -1;  // records handed over by a test: no agent
      r.nonce = h.nonce;
      r.bytes = h.bytes;
      r.num_xcc = h.num_xcc;
      r.mfma_iters = h.mfma_iters;
      r.mfma_grid = static_cast<int>(h.burn_wgs);
      r.fill_us = h.fill_us;
      r.check_us = h.check_us;
      r.check2_us = h.check2_us;
      r.mfma_us = h.mfma_us;
      mi355x::perf_verdict(records.data(), counters.data(), h.burn_wgs, &r);
      std::printf("%s\n", mi355x::perf_json(r).c_str());
    };
    run();
    uint32_t* const arrays[2] = {records.data(), counters.data()};
    const size_t lens[2] = {records.size(), counters.size()};
    for (uint32_t v = 0; v < h.variants; ++v)
      if (!with_variant(arrays, lens, run)) {
        std::fprintf(stderr, "bad perf variant %u\n", v);
        return 2;
      }
  }
  if (got != 0) {
    std::fprintf(stderr, "truncated perf header: %zu bytes\n", got);
    return 2;
  }
  return 0;
}

static void set_error(char (&dst)[160], const char* hex) {
  size_t n = 0;
  for (; hex[0] && hex[1] && n + 1 < sizeof(dst); hex += 2) {
    const char b[3] = {hex[0], hex[1], 0};
    dst[n++] = static_cast<char>(std::strtoul(b, nullptr, 16));
  }
  dst[n] = 0;
}

static int cmd_json(int argc, char** argv) {
  if (argc != 9) return 2;
  const std::string kind = argv[2];
  const int i = static_cast<int>(std::strtoll(argv[3], nullptr, 0));
  const uint32_t u = static_cast<uint32_t>(std::strtoull(argv[4], nullptr, 0));
  const uint64_t u64 = std::strtoull(argv[5], nullptr, 0);
  const int64_t i64 = std::strtoll(argv[6], nullptr, 0);
  const double d = std::strtod(argv[7], nullptr);
  if (kind == "sweep") {
    mi355x_sweep_result r;
    std::memset(&r, 0, sizeof(r));
    r.ordinal = r.ok = r.hsa_error = r.iters = r.grid = r.cu_count = r.num_xcc = r.records_ok = r.cus_covered =
        r.xccs_covered = r.all_resident = r.kept_queue = r.kfd_node_id = i;
    for (int& w : r.wgs_per_xcc) w = i;
    r.nonce = r.mfma_bad = r.lds_bad = r.tile_bad = u;
    r.kernel_us = r.arrival_spread_us = r.total_us = r.in_flight_s = d;
    set_error(r.error, argv[8]);
    std::snprintf(r.pci_bus_id, sizeof(r.pci_bus_id), "%s", r.error);
    std::printf("%s\n", mi355x::sweep_json(r).c_str());
  } else if (kind == "perf") {
    mi355x_perf_result r;
    std::memset(&r, 0, sizeof(r));
    r.ordinal = r.ok = r.hsa_error = r.cu_count = r.num_xcc = r.mfma_iters = r.mfma_grid = r.mfma_records_ok =
        r.mfma_checksum_mismatch = r.mfma_xccs = r.kept_queue = r.kfd_node_id = i;
    r.nonce = u;
    r.bytes = r.hbm_bad_words = r.hbm_bad_words_pass2 = u64;
    r.hbm_first_bad = i64;
    r.fill_us = r.check_us = r.check2_us = r.hbm_write_gbps = r.hbm_read_gbps = r.mfma_us = r.mfma_tflops =
        r.clock_mhz_min = r.clock_mhz_median = r.clock_mhz_max = r.total_us = r.in_flight_s = d;
    for (double& c : r.xcd_clock_mhz) c = d;
    set_error(r.error, argv[8]);
    std::snprintf(r.pci_bus_id, sizeof(r.pci_bus_id), "%s", r.error);
    std::printf("%s\n", mi355x::perf_json(r).c_str());
  } else {
    return 2;
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "gen") return cmd_gen();
  if (cmd == "layout") return cmd_layout();
  if (cmd == "inject-layout") return cmd_inject_layout();
  if (cmd == "verify") return cmd_verify();
  if (cmd == "sweep-verdict") return cmd_sweep_verdict();
  if (cmd == "perf-verdict") return cmd_perf_verdict();
  if (cmd == "json") return cmd_json(argc, argv);
  std::fprintf(stderr, "usage: %s gen|layout|inject-layout|verify|sweep-verdict|perf-verdict|json\n", argv[0]);
  return 2;
}
