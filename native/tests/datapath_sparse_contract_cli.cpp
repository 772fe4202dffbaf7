// Host-only view of the sparse (2:4) MFMA datapath check's contract
// (datapath_sparse_kernel.h), of its verdict (datapath_sparse_verify.h) and of the
// kind's reply documents (probe_json.h), for tests/test_native_datapath_sparse.py.
// No HIP, no GPU.
//
//   datapath_sparse_contract_cli image GRID NONCE        the recipe's image on stdout, as bytes: GRID * 32 record
//        words of workgroups that found nothing (XCC id and HW_ID zero), then GRID * 7936 tile words
//   datapath_sparse_contract_cli verdict GRID NONCE FILE the datapath_sparse_json line of mi355x::datapath_sparse_verdict
//        on the image in FILE (the same layout); a file of another length is refused (exit 2)
//   datapath_sparse_contract_cli replies                 the kind's documents, one a line: the device object of a
//        check that reached no device, the one-shot document and the serve reply around it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "datapath_sparse_kernel.h"
#include "datapath_sparse_verify.h"
#include "probe_json.h"

static constexpr uint32_t kMaxWgs = 1024;  // one workgroup per CU; mi355x_hsa_datapath_sparse_check refuses more CUs

static bool grid_nonce(char** argv, uint32_t* grid, uint32_t* nonce) {
  *grid = static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 0));
  *nonce = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 0));
  if (*grid == 0 || *grid > kMaxWgs) std::fprintf(stderr, "datapath sparse: grid %u\n", *grid);
  return *grid != 0 && *grid <= kMaxWgs;
}

static int cmd_image(uint32_t grid, uint32_t nonce) {
  std::vector<uint32_t> words(static_cast<size_t>(grid) * (MI355X_DPSP_REC_WORDS + MI355X_DPSP_WG_WORDS), 0u);
  uint32_t* tiles = words.data() + static_cast<size_t>(grid) * MI355X_DPSP_REC_WORDS;
  for (uint32_t wg = 0; wg < grid; ++wg) {
    uint32_t* r = words.data() + static_cast<size_t>(wg) * MI355X_DPSP_REC_WORDS;
    r[MI355X_DPSPREC_MAGIC] = MI355X_DPSP_MAGIC;
    r[MI355X_DPSPREC_WG] = wg;
    r[MI355X_DPSPREC_NONCE] = nonce ^ wg;
    uint32_t* tile = tiles + static_cast<size_t>(wg) * MI355X_DPSP_WG_WORDS;
    for (uint32_t s = 0; s < MI355X_DPSP_STAGES; ++s)
      mi355x::datapath_sparse_expected_tile(s, dpsp_wave_nonce(nonce, wg, 0), tile + dpsp_tile_offset(s));
  }
  return std::fwrite(words.data(), sizeof(uint32_t), words.size(), stdout) == words.size() ? 0 : 1;
}

static mi355x_datapath_sparse_result blank(uint32_t grid, uint32_t nonce) {
  mi355x_datapath_sparse_result r;
  std::memset(&r, 0, sizeof(r));
  r.kfd_node_id = -1;  // records handed over by a test: no agent
  r.nonce = nonce;
  r.grid = static_cast<int>(grid);
  return r;
}

static int cmd_verdict(uint32_t grid, uint32_t nonce, const char* path) {
  std::vector<uint32_t> words(static_cast<size_t>(grid) * (MI355X_DPSP_REC_WORDS + MI355X_DPSP_WG_WORDS) + 1);
  std::FILE* f = std::fopen(path, "rb");
  const size_t got = f ? std::fread(words.data(), sizeof(uint32_t), words.size(), f) : 0;
  if (f) std::fclose(f);
  if (got != words.size() - 1) {
    std::fprintf(stderr, "datapath sparse image: %zu words, want %zu\n", got, words.size() - 1);
    return 2;
  }
  mi355x_datapath_sparse_result r = blank(grid, nonce);
  mi355x::datapath_sparse_verdict(words.data(), words.data() + static_cast<size_t>(grid) * MI355X_DPSP_REC_WORDS, grid, &r);
  std::printf("%s\n", mi355x::datapath_sparse_json(r).c_str());
  return 0;
}

static int cmd_replies() {
  auto r = mi355x::blank_result<mi355x_datapath_sparse_result>(99, 7000);
  std::snprintf(r.error, sizeof(r.error), "no such GPU (count=1)");
  const std::string device = mi355x::datapath_sparse_json(r);
  std::printf("%s\n", device.c_str());
  std::printf("%s\n", mi355x::oneshot_check_json("datapath_sparse", false, 1, 1, 2, 3, "[" + device + "]").c_str());
  std::printf("%s\n", mi355x::serve_reply_json(true, 5, "datapath_sparse", false, 1, 3, "[" + device + "]").c_str());
  std::printf("%s\n", mi355x::serve_reply_json(false, 0, "probe", true, 1, 3, "[]").c_str());
  return 0;
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  uint32_t grid = 0, nonce = 0;
  if (cmd == "image" && argc == 4) return grid_nonce(argv, &grid, &nonce) ? cmd_image(grid, nonce) : 2;
  if (cmd == "verdict" && argc == 5) return grid_nonce(argv, &grid, &nonce) ? cmd_verdict(grid, nonce, argv[4]) : 2;
  if (cmd == "replies" && argc == 2) return cmd_replies();
  std::fprintf(stderr, "usage: %s image GRID NONCE | verdict GRID NONCE FILE | replies\n", argv[0]);
  return 2;
}
