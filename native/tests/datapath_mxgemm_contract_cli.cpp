// Host-only view of the MXFP4 GEMM pipeline check's contract (datapath_mxgemm_kernel.h), of its verdict
// (datapath_mxgemm_verify.h) and of the kind's reply documents (probe_json.h), for
// tests/test_native_datapath_mxgemm.py. No HIP, no GPU.
//
//   datapath_mxgemm_contract_cli operands GRID NONCE KSTEPS   what mi355x_mxgemm_fill writes, as bytes: GRID panels of
//        128 x K/2 bytes of A, 128 x K/2 bytes of B, GRID panels of 128 x K/32 scale bytes of A, 128 x K/32 of B
//   datapath_mxgemm_contract_cli image GRID NONCE KSTEPS      the image of a correct run, as bytes: GRID * 32 record
//        words (XCC id and HW_ID zero), then GRID * 16384 D words
//   datapath_mxgemm_contract_cli verdict GRID NONCE KSTEPS FILE   the datapath_mxgemm_json line of
//        mi355x::datapath_mxgemm_verdict on the image in FILE (the same layout); another length is refused (exit 2)
//   datapath_mxgemm_contract_cli replies                      the kind's documents, one a line: the device object of a
//        check that reached no device, the one-shot document and the serve reply around it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "datapath_mxgemm_kernel.h"
#include "datapath_mxgemm_verify.h"
#include "probe_json.h"

static bool sizes(char** argv, uint32_t* grid, uint32_t* nonce, uint32_t* ksteps) {
  *grid = static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 0));
  *nonce = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 0));
  *ksteps = static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 0));
  const bool ok = dpmx_sizes_ok(*grid, *ksteps);
  if (!ok) std::fprintf(stderr, "datapath mxgemm: grid %u ksteps %u\n", *grid, *ksteps);
  return ok;
}

template <typename T>
static bool put(const std::vector<T>& v) {
  return std::fwrite(v.data(), sizeof(T), v.size(), stdout) == v.size();
}

static int cmd_operands(uint32_t grid, uint32_t nonce, uint32_t ksteps) {
  const mi355x::MxB b(nonce, ksteps);
  std::vector<uint32_t> a(static_cast<size_t>(grid) * MI355X_DPMX_TILE * (b.K / 8u));
  std::vector<uint8_t> sa(static_cast<size_t>(grid) * MI355X_DPMX_TILE * (b.K / 32u));
  std::vector<int16_t> units(b.K);
  mi355x::MxFold feed, scale;
  for (uint32_t wg = 0; wg < grid; ++wg)
    for (uint32_t i = 0; i < MI355X_DPMX_TILE; ++i) {
      const size_t line = static_cast<size_t>(wg) * MI355X_DPMX_TILE + i;
      mi355x::datapath_mxgemm_line(dpmx_wg_seed(nonce, wg), 0u, ksteps, i, &a[line * (b.K / 8u)], &sa[line * (b.K / 32u)],
                                   units.data(), &feed, &scale);
    }
  return put(a) && put(b.dwords) && put(sa) && put(b.scales) ? 0 : 1;
}

static int cmd_image(uint32_t grid, uint32_t nonce, uint32_t ksteps) {
  const mi355x::MxB b(nonce, ksteps);
  std::vector<uint32_t> words(static_cast<size_t>(grid) * (MI355X_DPMX_REC_WORDS + MI355X_DPMX_WG_WORDS), 0u);
  uint32_t* tiles = words.data() + static_cast<size_t>(grid) * MI355X_DPMX_REC_WORDS;
  for (uint32_t wg = 0; wg < grid; ++wg) {
    uint32_t* r = words.data() + static_cast<size_t>(wg) * MI355X_DPMX_REC_WORDS;
    r[MI355X_DPMXREC_MAGIC] = MI355X_DPMX_MAGIC;
    r[MI355X_DPMXREC_WG] = wg;
    r[MI355X_DPMXREC_NONCE] = nonce ^ wg;
    r[MI355X_DPMXREC_XCC] = ksteps << 8;
    mi355x::datapath_mxgemm_expected(b, nonce, wg, tiles + static_cast<size_t>(wg) * MI355X_DPMX_WG_WORDS,
                                     r + MI355X_DPMXREC_FOLD);
  }
  return put(words) ? 0 : 1;
}

static int cmd_verdict(uint32_t grid, uint32_t nonce, uint32_t ksteps, const char* path) {
  std::vector<uint32_t> words(static_cast<size_t>(grid) * (MI355X_DPMX_REC_WORDS + MI355X_DPMX_WG_WORDS) + 1);
  std::FILE* f = std::fopen(path, "rb");
  const size_t got = f ? std::fread(words.data(), sizeof(uint32_t), words.size(), f) : 0;
  if (f) std::fclose(f);
  if (got != words.size() - 1) {
    std::fprintf(stderr, "datapath mxgemm image: %zu words, want %zu\n", got, words.size() - 1);
    return 2;
  }
  mi355x_datapath_mxgemm_result r;
  std::memset(&r, 0, sizeof(r));
  r.kfd_node_id = -1;  // records handed over by a test: no agent
  r.nonce = nonce;
  r.grid = static_cast<int>(grid);
  r.ksteps = static_cast<int>(ksteps);
  mi355x::datapath_mxgemm_verdict(words.data(), words.data() + static_cast<size_t>(grid) * MI355X_DPMX_REC_WORDS, grid,
                                  ksteps, &r);
  std::printf("%s\n", mi355x::datapath_mxgemm_json(r).c_str());
  return 0;
}

static int cmd_replies() {
  auto r = mi355x::blank_result<mi355x_datapath_mxgemm_result>(99, 7000);
  std::snprintf(r.error, sizeof(r.error), "no such GPU (count=1)");
  const std::string device = mi355x::datapath_mxgemm_json(r);
  std::printf("%s\n", device.c_str());
  std::printf("%s\n", mi355x::oneshot_check_json("datapath_mxgemm", false, 1, 1, 2, 3, "[" + device + "]").c_str());
  std::printf("%s\n", mi355x::serve_reply_json(true, 5, "datapath_mxgemm", false, 1, 3, "[" + device + "]").c_str());
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
