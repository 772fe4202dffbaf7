// Host-only view of the split-K GEMM check's contract (datapath_splitk_kernel.h), of its verdict
// (datapath_splitk_verify.h) and of the kind's reply documents (probe_json.h), for
// tests/test_native_datapath_splitk.py. No HIP, no GPU.
//
//   datapath_splitk_contract_cli image TILES SPLITS KSTEPS NONCE      the image of a correct run, as bytes:
//        TILES * SPLITS * 32 record words (XCC id and HW_ID zero), then TILES * 16384 D words, then TILES * 8 ledger words
//   datapath_splitk_contract_cli verdict TILES SPLITS KSTEPS NONCE FILE   the datapath_splitk_json line of
//        mi355x::datapath_splitk_verdict on the image in FILE (the same layout); another length is refused (exit 2)
//   datapath_splitk_contract_cli replies                      the kind's documents, one a line: the device object of a
//        check that reached no device, the one-shot document and the serve reply around it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "datapath_splitk_kernel.h"
#include "datapath_splitk_verify.h"
#include "probe_json.h"

static constexpr uint32_t kMaxTiles = 128;  // a tile per 8 CUs; mi355x_hsa_datapath_splitk_check refuses more than 1024 CUs

struct Sizes {
  uint32_t tiles, splits, ksteps, nonce;
  size_t rec_words() const { return static_cast<size_t>(tiles) * splits * MI355X_DPSK_REC_WORDS; }
  size_t d_words() const { return static_cast<size_t>(tiles) * MI355X_DPSK_TILE_WORDS; }
  size_t words() const { return rec_words() + d_words() + static_cast<size_t>(tiles) * MI355X_DPSK_LEDGER_WORDS; }
};

static bool sizes(char** argv, Sizes* z) {
  uint32_t* into[4] = {&z->tiles, &z->splits, &z->ksteps, &z->nonce};
  for (int i = 0; i < 4; ++i) *into[i] = static_cast<uint32_t>(std::strtoul(argv[2 + i], nullptr, 0));
  const bool ok = z->tiles <= kMaxTiles && dpsk_sizes_ok(z->tiles, z->splits, z->ksteps);
  if (!ok) std::fprintf(stderr, "datapath splitk: tiles %u splits %u ksteps %u\n", z->tiles, z->splits, z->ksteps);
  return ok;
}

static int cmd_image(const Sizes& z) {
  const mi355x::GemmB b(z.nonce, z.splits * z.ksteps);
  const std::vector<mi355x::GemmFold> fb = mi355x::datapath_splitk_b_folds(b, z.splits, z.ksteps);
  std::vector<uint32_t> words(z.words(), 0u);
  uint32_t* d = words.data() + z.rec_words();
  uint32_t* ledger = d + z.d_words();
  for (uint32_t t = 0; t < z.tiles; ++t) {
    uint32_t whole_panel_folds[16];  // of the GEMM check's waves: not part of this image
    mi355x::datapath_gemm_expected(b, z.nonce, t, d + static_cast<size_t>(t) * MI355X_DPSK_TILE_WORDS, whole_panel_folds);
    const std::vector<mi355x::GemmFold> fa = mi355x::datapath_splitk_a_folds(z.nonce, t, z.splits, z.ksteps);
    for (uint32_t s = 0; s < z.splits; ++s) {
      const uint32_t wg = t * z.splits + s;
      uint32_t* r = words.data() + static_cast<size_t>(wg) * MI355X_DPSK_REC_WORDS;
      r[MI355X_DPSKREC_MAGIC] = MI355X_DPSK_MAGIC;
      r[MI355X_DPSKREC_WG] = wg;
      r[MI355X_DPSKREC_NONCE] = z.nonce ^ wg;
      r[MI355X_DPSKREC_TILES] = z.tiles;
      r[MI355X_DPSKREC_SPLITS] = z.splits;
      r[MI355X_DPSKREC_KSTEPS] = z.ksteps;
      mi355x::datapath_splitk_folds(fa.data(), fb.data(), s, r + MI355X_DPSKREC_FOLD);
    }
    mi355x::datapath_splitk_ledger(fa.data(), fb.data(), z.nonce, t, z.splits, ledger + t * MI355X_DPSK_LEDGER_WORDS);
  }
  return std::fwrite(words.data(), sizeof(uint32_t), words.size(), stdout) == words.size() ? 0 : 1;
}

static int cmd_verdict(const Sizes& z, const char* path) {
  std::vector<uint32_t> words(z.words() + 1);
  std::FILE* f = std::fopen(path, "rb");
  const size_t got = f ? std::fread(words.data(), sizeof(uint32_t), words.size(), f) : 0;
  if (f) std::fclose(f);
  if (got != words.size() - 1) {
    std::fprintf(stderr, "datapath splitk image: %zu words, want %zu\n", got, words.size() - 1);
    return 2;
  }
  mi355x_datapath_splitk_result r;
  std::memset(&r, 0, sizeof(r));
  r.kfd_node_id = -1;  // records handed over by a test: no agent
  r.nonce = z.nonce;
  r.tiles = static_cast<int>(z.tiles);
  r.splits = static_cast<int>(z.splits);
  r.ksteps = static_cast<int>(z.ksteps);
  r.grid = static_cast<int>(z.tiles * z.splits);
  mi355x::datapath_splitk_verdict(words.data(), words.data() + z.rec_words(), words.data() + z.rec_words() + z.d_words(),
                                  z.tiles, z.splits, z.ksteps, &r);
  std::printf("%s\n", mi355x::datapath_splitk_json(r).c_str());
  return 0;
}

static int cmd_replies() {
  auto r = mi355x::blank_result<mi355x_datapath_splitk_result>(99, 7000);
  std::snprintf(r.error, sizeof(r.error), "no such GPU (count=1)");
  const std::string device = mi355x::datapath_splitk_json(r);
  std::printf("%s\n", device.c_str());
  std::printf("%s\n", mi355x::oneshot_check_json("datapath_splitk", false, 1, 1, 2, 3, "[" + device + "]").c_str());
  std::printf("%s\n", mi355x::serve_reply_json(true, 5, "datapath_splitk", false, 1, 3, "[" + device + "]").c_str());
  std::printf("%s\n", mi355x::serve_reply_json(false, 0, "probe", true, 1, 3, "[]").c_str());
  return 0;
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  Sizes z{};
  if (cmd == "image" && argc == 6) return sizes(argv, &z) ? cmd_image(z) : 2;
  if (cmd == "verdict" && argc == 7) return sizes(argv, &z) ? cmd_verdict(z, argv[6]) : 2;
  if (cmd == "replies" && argc == 2) return cmd_replies();
  std::fprintf(stderr, "usage: %s image TILES SPLITS KSTEPS NONCE | verdict TILES SPLITS KSTEPS NONCE FILE | replies\n", argv[0]);
  return 2;
}
