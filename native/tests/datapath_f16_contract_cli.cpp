// Host-only view of the f16 MFMA datapath check's contract
// (datapath_f16_kernel.h) and of its verdict (datapath_f16_verify.h), for
// tests/test_native_datapath_f16.py and tests/test_gpu_datapath_f16.py. No HIP,
// no GPU.
//
//   datapath_f16_contract_cli gen     < requests    one unsigned word per request line, or a whole tile:
//        a stage row block dword nw | b stage col block dword nw | c stage row col nw |
//        wave_nonce nonce wg wave | tile stage nw   (the expected tile: 1024 or 256 words on one line)
//   datapath_f16_contract_cli layout                "struct field offset" / "struct sizeof n" / "define NAME n" lines
//   datapath_f16_contract_cli inject-layout         "define NAME n" lines of the injection contract and, when compiled
//        with -DMI355X_TEST_INJECT=1 (as the test-only code object is), mi355x_datapath_f16_args with its
//        trailing injection fields
//   datapath_f16_contract_cli verdict < cases       datapath_f16_json lines of mi355x::datapath_f16_verdict. A case:
//        uint32 grid, nonce, variants; grid*16 record words; grid*5632 tile words; then per variant:
//        uint32 n and n patches (uint32 array, index, value), array 0 = records, 1 = tiles. One line
//        for the case as given, then one per variant: the case with that variant's words replaced
//        (each variant starts from the case as given).
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "datapath_f16_kernel.h"
#include "datapath_f16_verify.h"
#include "probe_json.h"

static int cmd_gen() {
  char line[256];
  while (std::fgets(line, sizeof(line), stdin)) {
    char name[32];
    unsigned long long v[5] = {0, 0, 0, 0, 0};
    const int n = std::sscanf(line, "%31s %llu %llu %llu %llu %llu", name, &v[0], &v[1], &v[2], &v[3], &v[4]);
    if (n < 1) continue;
    const std::string g = name;
    const uint32_t s = static_cast<uint32_t>(v[0]);
    const bool stage_ok = v[0] < MI355X_DPHF_STAGES;
    if ((g == "a" || g == "b") && n == 6 && stage_ok && v[1] < dphf_dim(s) && v[2] < dphf_blocks(s) &&
        v[3] < dphf_dwords(s)) {
      const uint32_t w = g == "a" ? dphf_a_word(s, (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4])
                                  : dphf_b_word(s, (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4]);
      std::printf("%" PRIu32 "\n", w);
    } else if (g == "c" && n == 5 && stage_ok && v[1] < dphf_dim(s) && v[2] < dphf_dim(s)) {
      std::printf("%" PRIu32 "\n", dphf_c_word(s, (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]));
    } else if (g == "wave_nonce" && n == 4) {
      std::printf("%" PRIu32 "\n", dphf_wave_nonce((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]));
    } else if (g == "tile" && n == 3 && stage_ok) {
      uint32_t want[MI355X_DPHF_TILE];
      mi355x::datapath_f16_expected_tile(s, (uint32_t)v[1], want);
      const uint32_t words = dphf_dim(s) * dphf_dim(s);
      for (uint32_t k = 0; k < words; ++k) std::printf("%s%" PRIu32, k ? " " : "", want[k]);
      std::printf("\n");
    } else {
      std::fprintf(stderr, "bad gen request: %s", line);
      return 2;
    }
  }
  return 0;
}

#define FIELD(S, F) std::printf("%s %s %zu\n", #S, #F, offsetof(S, F))
#define SIZE(S) std::printf("%s sizeof %zu\n", #S, sizeof(S))
#define DEFINE(N) std::printf("define %s %llu\n", #N, static_cast<unsigned long long>(N))

static int cmd_layout() {
  FIELD(mi355x_datapath_f16_args, records);
  FIELD(mi355x_datapath_f16_args, tiles);
  FIELD(mi355x_datapath_f16_args, nonce);
  FIELD(mi355x_datapath_f16_args, grid);
  SIZE(mi355x_datapath_f16_args);
  DEFINE(MI355X_DPHF_THREADS);
  DEFINE(MI355X_DPHF_STAGES);
  DEFINE(MI355X_DPHF_TILE);
  DEFINE(MI355X_DPHF_TILE16);
  DEFINE(MI355X_DPHF_WG_WORDS);
  DEFINE(MI355X_DPHF_REC_WORDS);
  DEFINE(MI355X_DPHF_MAGIC);
  DEFINE(MI355X_DPHFREC_MAGIC);
  DEFINE(MI355X_DPHFREC_WG);
  DEFINE(MI355X_DPHFREC_NONCE);
  DEFINE(MI355X_DPHFREC_XCC);
  DEFINE(MI355X_DPHFREC_HWID);
  DEFINE(MI355X_DPHFREC_BAD);
  return 0;
}

static int cmd_inject_layout() {
#if defined(MI355X_TEST_INJECT)
  FIELD(mi355x_datapath_f16_args, records);
  FIELD(mi355x_datapath_f16_args, tiles);
  FIELD(mi355x_datapath_f16_args, nonce);
  FIELD(mi355x_datapath_f16_args, grid);
  FIELD(mi355x_datapath_f16_args, inject_kind);
  FIELD(mi355x_datapath_f16_args, inject_wg);
  FIELD(mi355x_datapath_f16_args, inject_wave);
  FIELD(mi355x_datapath_f16_args, inject_lane);
  FIELD(mi355x_datapath_f16_args, inject_index);
  FIELD(mi355x_datapath_f16_args, inject_mask);
  SIZE(mi355x_datapath_f16_args);
#endif
  DEFINE(MI355X_DPHF_INJECT_NONE);
  DEFINE(MI355X_DPHF_INJECT_MFMA);
  return 0;
}

static constexpr uint32_t kMaxWgs = 4096;  // mi355x_hsa_datapath_f16_check refuses more than 1024 CUs

template <typename T>
static bool read_n(T* dst, size_t n) {
  return std::fread(dst, sizeof(T), n, stdin) == n;
}

struct Patch {
  uint32_t array, index, value;
};

static int cmd_verdict() {
  struct {
    uint32_t grid, nonce, variants;
  } h;
  size_t got;
  while ((got = std::fread(&h, 1, sizeof(h), stdin)) == sizeof(h)) {
    if (h.grid == 0 || h.grid > kMaxWgs) {
      std::fprintf(stderr, "datapath f16 case: grid %u\n", h.grid);
      return 2;
    }
    std::vector<uint32_t> records(static_cast<size_t>(h.grid) * MI355X_DPHF_REC_WORDS);
    std::vector<uint32_t> tiles(static_cast<size_t>(h.grid) * MI355X_DPHF_WG_WORDS);
    if (!read_n(records.data(), records.size()) || !read_n(tiles.data(), tiles.size())) {
      std::fprintf(stderr, "truncated datapath f16 case\n");
      return 2;
    }
    auto run = [&] {
      mi355x_datapath_f16_result r;
      std::memset(&r, 0, sizeof(r));
      r.kfd_node_id = -1;  // records handed over by a test: no agent
      r.nonce = h.nonce;
      r.grid = static_cast<int>(h.grid);
      mi355x::datapath_f16_verdict(records.data(), tiles.data(), h.grid, &r);
      std::printf("%s\n", mi355x::datapath_f16_json(r).c_str());
    };
    run();
    std::vector<uint32_t>* const arrays[2] = {&records, &tiles};
    for (uint32_t v = 0; v < h.variants; ++v) {
      uint32_t n = 0;
      if (!read_n(&n, 1) || n > (1u << 24)) {
        std::fprintf(stderr, "bad datapath f16 variant %u\n", v);
        return 2;
      }
      std::vector<Patch> patches(n);
      if (n && !read_n(patches.data(), n)) {
        std::fprintf(stderr, "truncated datapath f16 variant %u\n", v);
        return 2;
      }
      for (const Patch& p : patches)
        if (p.array > 1 || p.index >= arrays[p.array]->size()) {
          std::fprintf(stderr, "datapath f16 variant %u: patch out of range\n", v);
          return 2;
        }
      std::vector<uint32_t> saved(n);
      for (uint32_t i = 0; i < n; ++i) {
        saved[i] = (*arrays[patches[i].array])[patches[i].index];
        (*arrays[patches[i].array])[patches[i].index] = patches[i].value;
      }
      run();
      for (uint32_t i = n; i-- > 0;) (*arrays[patches[i].array])[patches[i].index] = saved[i];
    }
  }
  if (got != 0) {
    std::fprintf(stderr, "truncated datapath f16 header: %zu bytes\n", got);
    return 2;
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "gen") return cmd_gen();
  if (cmd == "layout") return cmd_layout();
  if (cmd == "inject-layout") return cmd_inject_layout();
  if (cmd == "verdict") return cmd_verdict();
  std::fprintf(stderr, "usage: %s gen|layout|inject-layout|verdict\n", argv[0]);
  return 2;
}
