// Host-only view of the bf16 GEMM pipeline check's contract (datapath_gemm_kernel.h), of its verdict
// (datapath_gemm_verify.h) and of the kind's reply documents (probe_json.h), for
// tests/test_native_datapath_gemm.py. No HIP, no GPU.
//
//   datapath_gemm_contract_cli operands GRID NONCE KSTEPS   what mi355x_gemm_fill writes, as bytes: GRID panels of
//        128 x K bf16 of A, then K x 128 bf16 of B
//   datapath_gemm_contract_cli image GRID NONCE KSTEPS      the image of a correct run, as bytes: GRID * 32 record words
//        (XCC id and HW_ID zero), then GRID * 16384 D words
//   datapath_gemm_contract_cli verdict GRID NONCE KSTEPS FILE   the datapath_gemm_json line of
//        mi355x::datapath_gemm_verdict on the image in FILE (the same layout); another length is refused (exit 2)
//   datapath_gemm_contract_cli replies                      the kind's documents, one a line: the device object of a
//        check that reached no device, the one-shot document and the serve reply around it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "datapath_gemm_kernel.h"
#include "datapath_gemm_verify.h"
#include "probe_json.h"

static constexpr uint32_t kMaxWgs = 1024;  // one workgroup per CU; mi355x_hsa_datapath_gemm_check refuses more CUs

static bool sizes(char** argv, uint32_t* grid, uint32_t* nonce, uint32_t* ksteps) {
  *grid = static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 0));
  *nonce = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 0));
  *ksteps = static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 0));
  const bool ok = *grid != 0 && *grid <= kMaxWgs && *ksteps != 0 && *ksteps <= MI355X_DPGM_KSTEPS_MAX;
  if (!ok) std::fprintf(stderr, "datapath gemm: grid %u ksteps %u\n", *grid, *ksteps);
  return ok;
}

static int cmd_operands(uint32_t grid, uint32_t nonce, uint32_t ksteps) {
  const mi355x::GemmB b(nonce, ksteps);
  std::vector<uint16_t> row(b.K);
  std::vector<int16_t> units(b.K);
  for (uint32_t wg = 0; wg < grid; ++wg)
    for (uint32_t i = 0; i < MI355X_DPGM_TILE; ++i) {
      mi355x::datapath_gemm_a_row(dpgm_wg_seed(nonce, wg), ksteps, i, row.data(), units.data());
      if (std::fwrite(row.data(), sizeof(uint16_t), row.size(), stdout) != row.size()) return 1;
    }
  return std::fwrite(b.elem.data(), sizeof(uint16_t), b.elem.size(), stdout) == b.elem.size() ? 0 : 1;
}

static int cmd_image(uint32_t grid, uint32_t nonce, uint32_t ksteps) {
  const mi355x::GemmB b(nonce, ksteps);
  std::vector<uint32_t> words(static_cast<size_t>(grid) * (MI355X_DPGM_REC_WORDS + MI355X_DPGM_WG_WORDS), 0u);
  uint32_t* tiles = words.data() + static_cast<size_t>(grid) * MI355X_DPGM_REC_WORDS;
  for (uint32_t wg = 0; wg < grid; ++wg) {
    uint32_t* r = words.data() + static_cast<size_t>(wg) * MI355X_DPGM_REC_WORDS;
    r[MI355X_DPGMREC_MAGIC] = MI355X_DPGM_MAGIC;
    r[MI355X_DPGMREC_WG] = wg;
    r[MI355X_DPGMREC_NONCE] = nonce ^ wg;
    r[MI355X_DPGMREC_KSTEPS] = ksteps;
    mi355x::datapath_gemm_expected(b, nonce, wg, tiles + static_cast<size_t>(wg) * MI355X_DPGM_WG_WORDS,
                                   r + MI355X_DPGMREC_FOLD);
  }
  return std::fwrite(words.data(), sizeof(uint32_t), words.size(), stdout) == words.size() ? 0 : 1;
}

static int cmd_verdict(uint32_t grid, uint32_t nonce, uint32_t ksteps, const char* path) {
  std::vector<uint32_t> words(static_cast<size_t>(grid) * (MI355X_DPGM_REC_WORDS + MI355X_DPGM_WG_WORDS) + 1);
  std::FILE* f = std::fopen(path, "rb");
  const size_t got = f ? std::fread(words.data(), sizeof(uint32_t), words.size(), f) : 0;
  if (f) std::fclose(f);
  if (got != words.size() - 1) {
    std::fprintf(stderr, "datapath gemm image: %zu words, want %zu\n", got, words.size() - 1);
    return 2;
  }
  mi355x_datapath_gemm_result r;
  std::memset(&r, 0, sizeof(r));
  r.kfd_node_id = -1;  // records handed over by a test: no agent
  r.nonce = nonce;
  r.grid = static_cast<int>(grid);
  r.ksteps = static_cast<int>(ksteps);
  mi355x::datapath_gemm_verdict(words.data(), words.data() + static_cast<size_t>(grid) * MI355X_DPGM_REC_WORDS, grid,
                                ksteps, &r);
  std::printf("%s\n", mi355x::datapath_gemm_json(r).c_str());
  return 0;
}

static int cmd_replies() {
  auto r = mi355x::blank_result<mi355x_datapath_gemm_result>(99, 7000);
  std::snprintf(r.error, sizeof(r.error), "no such GPU (count=1)");
  const std::string device = mi355x::datapath_gemm_json(r);
  std::printf("%s\n", device.c_str());
  std::printf("%s\n", mi355x::oneshot_check_json("datapath_gemm", false, 1, 1, 2, 3, "[" + device + "]").c_str());
  std::printf("%s\n", mi355x::serve_reply_json(true, 5, "datapath_gemm", false, 1, 3, "[" + device + "]").c_str());
  std::printf("%s\n", mi355x::serve_reply_json(false, 0, "probe", true, 1, 3, "[]").c_str());
  return 0;
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  uint32_t grid = 0, nonce = 0, ksteps = 0;
  if (cmd == "operands" && argc == 5) return sizes(argv, &grid, &nonce, &ksteps) ? cmd_operands(grid, nonce, ksteps) : 2;
  if (cmd == "image" && argc == 5) return sizes(argv, &grid, &nonce, &ksteps) ? cmd_image(grid, nonce, ksteps) : 2;
  if (cmd == "verdict" && argc == 6)
    return sizes(argv, &grid, &nonce, &ksteps) ? cmd_verdict(grid, nonce, ksteps, argv[5]) : 2;
  if (cmd == "replies" && argc == 2) return cmd_replies();
  std::fprintf(stderr, "usage: %s operands|image GRID NONCE KSTEPS | verdict GRID NONCE KSTEPS FILE | replies\n", argv[0]);
  return 2;
}
