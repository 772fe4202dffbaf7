// Host-only view of the kernel contract in liveness_kernel.h and of
// probe_verify.h::verify_tile, for tests/test_kernel_reference.py: the operand
// generators at given indices, the layout of the four kernel-argument structs,
// and verify_tile's verdict on tiles read from stdin. No HIP, no GPU.
//
//   kernel_contract_cli gen     < requests    one value per request line:
//        a i k nonce | b k j nonce | c i j nonce | sweep_nonce nonce wg wave |
//        lds i nonce wg | hbm word seed | burn lane j nonce
//   kernel_contract_cli layout                "struct field offset" / "struct sizeof n" lines
//   kernel_contract_cli verify  < records     one "ok mismatches error" line per binary record:
//        uint32 nonce, int32 iters, 1024 floats, 4 meta words
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "liveness_kernel.h"
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

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "gen") return cmd_gen();
  if (cmd == "layout") return cmd_layout();
  if (cmd == "verify") return cmd_verify();
  std::fprintf(stderr, "usage: %s gen|layout|verify\n", argv[0]);
  return 2;
}
