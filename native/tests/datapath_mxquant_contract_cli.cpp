// Host-only view of the MX quantise check's contract (datapath_mxquant_kernel.h), of its verdict
// (datapath_mxquant_verify.h) and of the kind's reply documents (probe_json.h), for
// tests/test_native_datapath_mxquant.py. No HIP, no GPU.
//
//   datapath_mxquant_contract_cli operands GRID NONCE HSTEPS   what mi355x_mxquant_fill writes, as bytes: GRID panels of
//        128 x 128 bf16 of X, 128 HSTEPS x 128 bf16 of W1, 128 x 64 HSTEPS bytes of W2, 128 x 4 HSTEPS scale bytes
//   datapath_mxquant_contract_cli image GRID NONCE HSTEPS      the image of a correct run, as bytes: GRID * 32 record
//        words (XCC id and HW_ID zero), GRID * 2176 HSTEPS words of the quantised images, GRID * 16384 Y words
//   datapath_mxquant_contract_cli verdict GRID NONCE HSTEPS FILE   the datapath_mxquant_json line of
//        mi355x::datapath_mxquant_verdict on the image in FILE (the same layout); another length is refused (exit 2)
//   datapath_mxquant_contract_cli replies                      the kind's documents, one a line: the device object of a
//        check that reached no device, the one-shot document and the serve reply around it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "datapath_mxquant_kernel.h"
#include "datapath_mxquant_verify.h"
#include "probe_json.h"

static bool sizes(char** argv, uint32_t* grid, uint32_t* nonce, uint32_t* hsteps) {
  *grid = static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 0));
  *nonce = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 0));
  *hsteps = static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 0));
  const bool ok = dpmq_sizes_ok(*grid, *hsteps);
  if (!ok) std::fprintf(stderr, "datapath mxquant: grid %u hsteps %u\n", *grid, *hsteps);
  return ok;
}

template <typename T>
static bool put(const std::vector<T>& v) {
  return std::fwrite(v.data(), sizeof(T), v.size(), stdout) == v.size();
}

static int cmd_operands(uint32_t grid, uint32_t nonce, uint32_t hsteps) {
  const mi355x::MqShared sh(nonce, hsteps);
  std::vector<uint32_t> x(static_cast<size_t>(grid) * MI355X_DPMQ_TILE * 64u), w1(static_cast<size_t>(sh.N) * 64u);
  for (uint32_t wg = 0; wg < grid; ++wg)
    for (uint32_t i = 0; i < MI355X_DPMQ_TILE; ++i)
      for (uint32_t p = 0; p < 64; ++p)
        x[(static_cast<size_t>(wg) * MI355X_DPMQ_TILE + i) * 64u + p] = dpmq_x_dword(nonce, dpmq_wg_seed(nonce, wg), i, p);
  for (uint32_t n = 0; n < sh.N; ++n)
    for (uint32_t p = 0; p < 64; ++p) w1[static_cast<size_t>(n) * 64u + p] = dpmq_w1_dword(nonce, n, p);
  return put(x) && put(w1) && put(sh.w2) && put(sh.sb) ? 0 : 1;
}

// the three parts of an image of `grid` workgroups in `words`
struct Parts {
  uint32_t *records, *image, *tiles;
  Parts(std::vector<uint32_t>& words, uint32_t grid, uint32_t hsteps)
      : records(words.data()),
        image(records + static_cast<size_t>(grid) * MI355X_DPMQ_REC_WORDS),
        tiles(image + static_cast<size_t>(grid) * MI355X_DPMQ_IMG_WORDS(hsteps)) {}
};
static size_t image_words(uint32_t grid, uint32_t hsteps) {
  return static_cast<size_t>(grid) * (MI355X_DPMQ_REC_WORDS + MI355X_DPMQ_IMG_WORDS(hsteps) + MI355X_DPMQ_WG_WORDS);
}

static int cmd_image(uint32_t grid, uint32_t nonce, uint32_t hsteps) {
  const mi355x::MqShared sh(nonce, hsteps);
  std::vector<uint32_t> words(image_words(grid, hsteps), 0u);
  const Parts p(words, grid, hsteps);
  for (uint32_t wg = 0; wg < grid; ++wg) {
    uint32_t* r = p.records + static_cast<size_t>(wg) * MI355X_DPMQ_REC_WORDS;
    r[MI355X_DPMQREC_MAGIC] = MI355X_DPMQ_MAGIC;
    r[MI355X_DPMQREC_WG] = wg;
    r[MI355X_DPMQREC_NONCE] = nonce ^ wg;
    r[MI355X_DPMQREC_XCC] = hsteps << 8;
    mi355x::datapath_mxquant_expected(sh, nonce, wg, r + MI355X_DPMQREC_FOLD,
                                      p.image + static_cast<size_t>(wg) * MI355X_DPMQ_IMG_WORDS(hsteps),
                                      p.tiles + static_cast<size_t>(wg) * MI355X_DPMQ_WG_WORDS);
  }
  return put(words) ? 0 : 1;
}

static int cmd_verdict(uint32_t grid, uint32_t nonce, uint32_t hsteps, const char* path) {
  std::vector<uint32_t> words(image_words(grid, hsteps) + 1);
  std::FILE* f = std::fopen(path, "rb");
  const size_t got = f ? std::fread(words.data(), sizeof(uint32_t), words.size(), f) : 0;
  if (f) std::fclose(f);
  if (got != words.size() - 1) {
    std::fprintf(stderr, "datapath mxquant image: %zu words, want %zu\n", got, words.size() - 1);
    return 2;
  }
  mi355x_datapath_mxquant_result r;
  std::memset(&r, 0, sizeof(r));
  r.kfd_node_id = -1;  // records handed over by a test: no agent
  r.nonce = nonce;
  r.grid = static_cast<int>(grid);
  r.hsteps = static_cast<int>(hsteps);
  const Parts p(words, grid, hsteps);
  mi355x::datapath_mxquant_verdict(p.records, p.image, p.tiles, grid, hsteps, &r);
  std::printf("%s\n", mi355x::datapath_mxquant_json(r).c_str());
  return 0;
}

static int cmd_replies() {
  auto r = mi355x::blank_result<mi355x_datapath_mxquant_result>(99, 7000);
  std::snprintf(r.error, sizeof(r.error), "no such GPU (count=1)");
  const std::string device = mi355x::datapath_mxquant_json(r);
  std::printf("%s\n", device.c_str());
  std::printf("%s\n", mi355x::oneshot_check_json("datapath_mxquant", false, 1, 1, 2, 3, "[" + device + "]").c_str());
  std::printf("%s\n", mi355x::serve_reply_json(true, 5, "datapath_mxquant", false, 1, 3, "[" + device + "]").c_str());
  std::printf("%s\n", mi355x::serve_reply_json(false, 0, "probe", true, 1, 3, "[]").c_str());
  return 0;
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  uint32_t grid = 0, nonce = 0, hsteps = 0;
  if (cmd == "operands" && argc == 5) return sizes(argv, &grid, &nonce, &hsteps) ? cmd_operands(grid, nonce, hsteps) : 2;
  if (cmd == "image" && argc == 5) return sizes(argv, &grid, &nonce, &hsteps) ? cmd_image(grid, nonce, hsteps) : 2;
  if (cmd == "verdict" && argc == 6)
    return sizes(argv, &grid, &nonce, &hsteps) ? cmd_verdict(grid, nonce, hsteps, argv[5]) : 2;
  if (cmd == "replies" && argc == 2) return cmd_replies();
  std::fprintf(stderr, "usage: %s operands|image GRID NONCE HSTEPS | verdict GRID NONCE HSTEPS FILE | replies\n", argv[0]);
  return 2;
}
