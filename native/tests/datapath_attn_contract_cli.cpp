// Host-only view of the fused attention check's contract (datapath_attn_kernel.h), of its verdict
// (datapath_attn_verify.h) and of the kind's reply documents (probe_json.h), for
// tests/test_native_datapath_attn.py. No HIP, no GPU.
//
//   datapath_attn_contract_cli image HEADS QBLOCKS KBLOCKS NONCE      the image of a correct run, as bytes:
//        HEADS * QBLOCKS * 32 record words (XCC id, HW_ID and exp_inexact zero), then HEADS * QBLOCKS * 256 m / l words,
//        then HEADS * QBLOCKS * 8192 O words
//   datapath_attn_contract_cli verdict HEADS QBLOCKS KBLOCKS NONCE FILE   the datapath_attn_json line of
//        mi355x::datapath_attn_verdict on the image in FILE (the same layout); another length is refused (exit 2)
//   datapath_attn_contract_cli replies                        the kind's documents, one a line: the device object of a
//        check that reached no device, the one-shot document and the serve reply around it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "datapath_attn_kernel.h"
#include "datapath_attn_verify.h"
#include "probe_json.h"

static constexpr uint32_t kMaxGrid = 1024;  // a workgroup a CU; mi355x_hsa_datapath_attn_check refuses more than 1024 CUs

struct Sizes {
  uint32_t heads, qblocks, kblocks, nonce;
  size_t grid() const { return static_cast<size_t>(heads) * qblocks; }
  size_t rec_words() const { return grid() * MI355X_DPAT_REC_WORDS; }
  size_t ml_words() const { return grid() * MI355X_DPAT_ML_WORDS; }
  size_t words() const { return rec_words() + ml_words() + grid() * MI355X_DPAT_O_WORDS; }
};

static bool sizes(char** argv, Sizes* z) {
  uint32_t* into[4] = {&z->heads, &z->qblocks, &z->kblocks, &z->nonce};
  for (int i = 0; i < 4; ++i) *into[i] = static_cast<uint32_t>(std::strtoul(argv[2 + i], nullptr, 0));
  const bool ok = dpat_sizes_ok(z->heads, z->qblocks, z->kblocks) && z->grid() <= kMaxGrid;
  if (!ok) std::fprintf(stderr, "datapath attn: heads %u qblocks %u kblocks %u\n", z->heads, z->qblocks, z->kblocks);
  return ok;
}

static int cmd_image(const Sizes& z) {
  std::vector<uint32_t> words(z.words(), 0u);
  uint32_t* ml = words.data() + z.rec_words();
  uint32_t* o = ml + z.ml_words();
  std::vector<int32_t> s(z.kblocks * MI355X_DPAT_KBLOCK);
  for (uint32_t head = 0; head < z.heads; ++head) {
    const mi355x::AttnHead h(z.nonce, head, z.qblocks, z.kblocks);
    for (uint32_t qb = 0; qb < z.qblocks; ++qb) {
      const uint32_t wg = head * z.qblocks + qb;
      uint32_t* r = words.data() + static_cast<size_t>(wg) * MI355X_DPAT_REC_WORDS;
      r[MI355X_DPATREC_MAGIC] = MI355X_DPAT_MAGIC;
      r[MI355X_DPATREC_WG] = wg;
      r[MI355X_DPATREC_NONCE] = z.nonce ^ wg;
      r[MI355X_DPATREC_HEADS] = z.heads;
      r[MI355X_DPATREC_QBLOCKS] = z.qblocks;
      r[MI355X_DPATREC_KBLOCKS] = z.kblocks;
      mi355x::datapath_attn_folds(h, r + MI355X_DPATREC_FOLD);
      for (uint32_t qi = 0; qi < MI355X_DPAT_QBLOCK; ++qi) {
        const size_t row = static_cast<size_t>(wg) * MI355X_DPAT_QBLOCK + qi;
        const int32_t m = mi355x::datapath_attn_scores(h, qb * MI355X_DPAT_QBLOCK + qi, s.data());
        mi355x::datapath_attn_row(h, s.data(), m, ml + row * 2, o + row * MI355X_DPAT_D);
      }
    }
  }
  return std::fwrite(words.data(), sizeof(uint32_t), words.size(), stdout) == words.size() ? 0 : 1;
}

static int cmd_verdict(const Sizes& z, const char* path) {
  std::vector<uint32_t> words(z.words() + 1);
  std::FILE* f = std::fopen(path, "rb");
  const size_t got = f ? std::fread(words.data(), sizeof(uint32_t), words.size(), f) : 0;
  if (f) std::fclose(f);
  if (got != words.size() - 1) {
    std::fprintf(stderr, "datapath attn image: %zu words, want %zu\n", got, words.size() - 1);
    return 2;
  }
  mi355x_datapath_attn_result r;
  std::memset(&r, 0, sizeof(r));
  r.kfd_node_id = -1;  // records handed over by a test: no agent
  r.nonce = z.nonce;
  r.heads = static_cast<int>(z.heads);
  r.qblocks = static_cast<int>(z.qblocks);
  r.kblocks = static_cast<int>(z.kblocks);
  r.grid = static_cast<int>(z.grid());
  mi355x::datapath_attn_verdict(words.data(), words.data() + z.rec_words(), words.data() + z.rec_words() + z.ml_words(),
                                z.heads, z.qblocks, z.kblocks, &r);
  std::printf("%s\n", mi355x::datapath_attn_json(r).c_str());
  return 0;
}

static int cmd_replies() {
  auto r = mi355x::blank_result<mi355x_datapath_attn_result>(99, 7000);
  std::snprintf(r.error, sizeof(r.error), "no such GPU (count=1)");
  const std::string device = mi355x::datapath_attn_json(r);
  std::printf("%s\n", device.c_str());
  std::printf("%s\n", mi355x::oneshot_check_json("datapath_attn", false, 1, 1, 2, 3, "[" + device + "]").c_str());
  std::printf("%s\n", mi355x::serve_reply_json(true, 5, "datapath_attn", false, 1, 3, "[" + device + "]").c_str());
  std::printf("%s\n", mi355x::serve_reply_json(false, 0, "probe", true, 1, 3, "[]").c_str());
  return 0;
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  Sizes z{};
  if (cmd == "image" && argc == 6) return sizes(argv, &z) ? cmd_image(z) : 2;
  if (cmd == "verdict" && argc == 7) return sizes(argv, &z) ? cmd_verdict(z, argv[6]) : 2;
  if (cmd == "replies" && argc == 2) return cmd_replies();
  std::fprintf(stderr, "usage: %s image HEADS QBLOCKS KBLOCKS NONCE | verdict HEADS QBLOCKS KBLOCKS NONCE FILE | replies\n", argv[0]);
  return 2;
}
