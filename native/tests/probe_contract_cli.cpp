// Host-only driver of the probe's wire format for the CPU tests
// (tests/test_probe_contract.py): what mi355x-liveness-probe prints
// (src/health/probe_json.h) and the request lines its server accepts
// (src/health/probe_request.h), without a GPU.
//
//   probe_contract_cli replies        one JSON document, every value fixed:
//        "devices": per kind (probe = the HSA build's, probe_hip, sweep, perf, datapath, datapath_i8) the
//                   printer's object for a blank_result ("blank") and for a result whose every numeric
//                   field is distinct and non-zero, with num_xcc 8 ("filled8") and 16 ("filled16"), and
//                   whose error holds a quote and a backslash
//        "hello":   the server's first line, runtime up ("ok") and not ("failed")
//        "serve":   per kind the reply around an empty device list, "untagged" and "tagged"
//        "oneshot": per kind (and "identify") the one-shot document around an empty device list
//        "bad_request": "untagged" and "tagged"; "runtime_init_failed"
//   probe_contract_cli replies-bf16   the "devices", "serve" and "oneshot" entries of the datapath_bf16 kind, in
//        a document of its own (tests/test_probe_contract_bf16.py): `replies` stays as recorded
//   probe_contract_cli replies-fp8    the same for the datapath_fp8 kind (tests/test_probe_contract_fp8.py)
//   probe_contract_cli replies-f16    the same for the datapath_f16 kind (tests/test_probe_contract_f16.py)
//   probe_contract_cli parse < lines  per request line one JSON line: the parsed request
//        {"tagged","id","kind","iters","timeout","mib","devices":[[ordinal,nonce,deadline],..]},
//        or "bad request" for a line the server refuses
#include <cstdio>
#include <cstring>
#include <string>

#include "mi355x/liveness_probe.h"
#include "probe_json.h"
#include "probe_request.h"

namespace {

using namespace mi355x;

// distinct non-zero values, in field order
struct Counter {
  int n = 100;  // clear of num_xcc 8 and 16
  int i() { return ++n; }
  uint32_t u() { return static_cast<uint32_t>(++n); }
  double d() { return ++n + 0.25; }
};

const char kError[] = "a \"quoted\" back\\slash";

template <typename R>
void name_agent(R* r, Counter& c) {
  r->kfd_node_id = c.i();
  std::snprintf(r->pci_bus_id, sizeof(r->pci_bus_id), "0000:%02x:00.0", c.i());
  std::snprintf(r->error, sizeof(r->error), "%s", kError);
}

mi355x_probe_result filled_probe() {
  Counter c;
  mi355x_probe_result r{};
  r.ordinal = c.i();
  r.ok = 1;
  r.hip_error = c.i();
  r.mismatches = c.i();
  r.nonce = c.u();
  r.xcc_id = c.u();
  r.hw_id = c.u();
  r.iters = c.i();
  r.dispatches = c.i();
  r.kernel_us = c.d();
  r.setup_us = c.d();
  r.total_us = c.d();
  for (double& p : r.phase_us) p = c.d();
  std::snprintf(r.runtime, sizeof(r.runtime), "hsa");
  std::snprintf(r.arch, sizeof(r.arch), "gfx950:sramecc+:xnack-");
  std::snprintf(r.name, sizeof(r.name), "AMD Instinct MI355X");
  std::snprintf(r.uuid, sizeof(r.uuid), "GPU-0123456789abcdef");
  r.pci_domain = c.i();
  r.pci_bus = c.i();
  r.pci_device = c.i();
  r.cu_count = c.i();
  r.total_mem = static_cast<uint64_t>(c.i()) << 32;
  r.late = 1;
  r.pending_s = c.d();
  name_agent(&r, c);
  return r;
}

mi355x_sweep_result filled_sweep(int num_xcc) {
  Counter c;
  auto r = blank_result<mi355x_sweep_result>(c.i(), c.u());
  r.ok = r.all_resident = r.kept_queue = 1;
  r.hsa_error = c.i();
  r.iters = c.i();
  r.grid = c.i();
  r.cu_count = c.i();
  r.num_xcc = num_xcc;
  r.records_ok = c.i();
  r.mfma_bad = c.u();
  r.lds_bad = c.u();
  r.tile_bad = c.u();
  r.cus_covered = c.i();
  r.xccs_covered = c.i();
  for (int& w : r.wgs_per_xcc) w = c.i();
  r.kernel_us = c.d();
  r.arrival_spread_us = c.d();
  r.total_us = c.d();
  r.in_flight_s = c.d();
  name_agent(&r, c);
  return r;
}

mi355x_perf_result filled_perf(int num_xcc) {
  Counter c;
  auto r = blank_result<mi355x_perf_result>(c.i(), c.u());
  r.ok = r.kept_queue = 1;
  r.hsa_error = c.i();
  r.bytes = static_cast<uint64_t>(c.i()) << 32;
  r.cu_count = c.i();
  r.num_xcc = num_xcc;
  r.fill_us = c.d();
  r.check_us = c.d();
  r.check2_us = c.d();
  r.hbm_write_gbps = c.d();
  r.hbm_read_gbps = c.d();
  r.hbm_bad_words = c.u();
  r.hbm_bad_words_pass2 = c.u();
  r.hbm_first_bad = c.i();
  r.mfma_iters = c.i();
  r.mfma_grid = c.i();
  r.mfma_records_ok = c.i();
  r.mfma_checksum_mismatch = c.i();
  r.mfma_xccs = c.i();
  r.mfma_us = c.d();
  r.mfma_tflops = c.d();
  r.clock_mhz_min = c.d();
  r.clock_mhz_median = c.d();
  r.clock_mhz_max = c.d();
  for (double& x : r.xcd_clock_mhz) x = c.d();
  r.total_us = c.d();
  r.in_flight_s = c.d();
  name_agent(&r, c);
  return r;
}

// mi355x_datapath_result or mi355x_datapath_i8_result (the same field names)
template <typename R>
R filled_datapath(int num_xcc) {
  Counter c;
  auto r = blank_result<R>(c.i(), c.u());
  r.ok = r.kept_queue = 1;
  r.hsa_error = c.i();
  r.grid = c.i();
  r.cu_count = c.i();
  r.num_xcc = num_xcc;
  r.records_ok = c.i();
  r.mfma_bad = c.u();
  for (uint32_t& s : r.stage_bad) s = c.u();
  r.tile_bad = c.u();
  r.first_bad_wg = c.i();
  r.first_bad_stage = c.i();
  r.first_bad_word = c.i();
  r.first_bad_got = c.u();
  r.first_bad_want = c.u();
  r.first_bad_xor = c.u();
  r.cus_covered = c.i();
  r.simds_covered = c.i();
  r.xccs_covered = c.i();
  r.kernel_us = c.d();
  r.total_us = c.d();
  r.in_flight_s = c.d();
  name_agent(&r, c);
  return r;
}

std::string three(const std::string& blank, const std::string& f8, const std::string& f16) {
  return "{\"blank\":" + blank + ",\"filled8\":" + f8 + ",\"filled16\":" + f16 + "}";
}

const char* const kKinds[] = {"probe", "sweep", "perf", "datapath", "datapath_i8"};

int cmd_replies() {
  const uint64_t t0 = 1000000001ull, t1 = 1000000002ull, t2 = 1000000003ull;
  std::string o = "{\n\"devices\":{";
  const mi355x_probe_result blank_probe{};
  o += "\n\"probe\":" + three(device_json(blank_probe, true), device_json(filled_probe(), true),
                             device_json(filled_probe(), true));
  o += ",\n\"probe_hip\":" + three(device_json(blank_probe, false), device_json(filled_probe(), false),
                                  device_json(filled_probe(), false));
  o += ",\n\"sweep\":" + three(sweep_json(blank_result<mi355x_sweep_result>(0, 0)), sweep_json(filled_sweep(8)),
                              sweep_json(filled_sweep(16)));
  o += ",\n\"perf\":" + three(perf_json(blank_result<mi355x_perf_result>(0, 0)), perf_json(filled_perf(8)),
                             perf_json(filled_perf(16)));
  o += ",\n\"datapath\":" + three(datapath_json(blank_result<mi355x_datapath_result>(0, 0)),
                                 datapath_json(filled_datapath<mi355x_datapath_result>(8)),
                                 datapath_json(filled_datapath<mi355x_datapath_result>(16)));
  o += ",\n\"datapath_i8\":" + three(datapath_i8_json(blank_result<mi355x_datapath_i8_result>(0, 0)),
                                    datapath_i8_json(filled_datapath<mi355x_datapath_i8_result>(8)),
                                    datapath_i8_json(filled_datapath<mi355x_datapath_i8_result>(16)));
  o += "},\n\"hello\":{\"ok\":" + serve_hello_json(8, true, t0, t1) + ",\n\"failed\":" +
       serve_hello_json(-4096, false, t0, t1) + "},\n\"serve\":{";
  for (const char* kind : kKinds)
    o += std::string(kind == kKinds[0] ? "" : ",") + "\n\"" + kind + "\":{\"untagged\":" +
         serve_reply_json(false, 0, kind, true, 8, t2, "[]") + ",\n\"tagged\":" +
         serve_reply_json(true, 5, kind, false, 8, t2, "[]") + "}";
  o += "},\n\"oneshot\":{";
  const OneshotProbeTimes times = {t0, t1, t2, 1.25, 2.25, 3.25, 4, {5.5, 6.5, 7.5, 8.5, 9.5}};
  o += "\n\"probe\":" + oneshot_probe_json(true, 8, false, times, "null", "null", "[]");
  o += ",\n\"identify\":" + oneshot_probe_json(false, 8, true, times, "null", "null", "[]");
  for (const char* kind : kKinds)
    if (std::strcmp(kind, "probe") != 0)
      o += std::string(",\n\"") + kind + "\":" + oneshot_check_json(kind, true, 8, t0, t1, t2, "[]");
  o += "},\n\"bad_request\":{\"untagged\":" + bad_request_json(false, 0) + ",\n\"tagged\":" + bad_request_json(true, 5) +
       "},\n\"runtime_init_failed\":" + runtime_init_failed_json(4096, t0, "null") + "\n}\n";
  std::fputs(o.c_str(), stdout);
  return 0;
}

int cmd_replies_bf16() {
  const uint64_t t0 = 1000000001ull, t1 = 1000000002ull, t2 = 1000000003ull;
  const char* kind = "datapath_bf16";
  std::string o = "{\n\"devices\":{\n\"datapath_bf16\":" +
                  three(datapath_bf16_json(blank_result<mi355x_datapath_bf16_result>(0, 0)),
                        datapath_bf16_json(filled_datapath<mi355x_datapath_bf16_result>(8)),
                        datapath_bf16_json(filled_datapath<mi355x_datapath_bf16_result>(16)));
  o += "},\n\"serve\":{\n\"datapath_bf16\":{\"untagged\":" + serve_reply_json(false, 0, kind, true, 8, t2, "[]") +
       ",\n\"tagged\":" + serve_reply_json(true, 5, kind, false, 8, t2, "[]") + "}";
  o += "},\n\"oneshot\":{\n\"datapath_bf16\":" + oneshot_check_json(kind, true, 8, t0, t1, t2, "[]") + "}\n}\n";
  std::fputs(o.c_str(), stdout);
  return 0;
}

int cmd_replies_fp8() {
  const uint64_t t0 = 1000000001ull, t1 = 1000000002ull, t2 = 1000000003ull;
  const char* kind = "datapath_fp8";
  std::string o = "{\n\"devices\":{\n\"datapath_fp8\":" +
                  three(datapath_fp8_json(blank_result<mi355x_datapath_fp8_result>(0, 0)),
                        datapath_fp8_json(filled_datapath<mi355x_datapath_fp8_result>(8)),
                        datapath_fp8_json(filled_datapath<mi355x_datapath_fp8_result>(16)));
  o += "},\n\"serve\":{\n\"datapath_fp8\":{\"untagged\":" + serve_reply_json(false, 0, kind, true, 8, t2, "[]") +
       ",\n\"tagged\":" + serve_reply_json(true, 5, kind, false, 8, t2, "[]") + "}";
  o += "},\n\"oneshot\":{\n\"datapath_fp8\":" + oneshot_check_json(kind, true, 8, t0, t1, t2, "[]") + "}\n}\n";
  std::fputs(o.c_str(), stdout);
  return 0;
}

int cmd_replies_f16() {
  const uint64_t t0 = 1000000001ull, t1 = 1000000002ull, t2 = 1000000003ull;
  const char* kind = "datapath_f16";
  std::string o = "{\n\"devices\":{\n\"datapath_f16\":" +
                  three(datapath_f16_json(blank_result<mi355x_datapath_f16_result>(0, 0)),
                        datapath_f16_json(filled_datapath<mi355x_datapath_f16_result>(8)),
                        datapath_f16_json(filled_datapath<mi355x_datapath_f16_result>(16)));
  o += "},\n\"serve\":{\n\"datapath_f16\":{\"untagged\":" + serve_reply_json(false, 0, kind, true, 8, t2, "[]") +
       ",\n\"tagged\":" + serve_reply_json(true, 5, kind, false, 8, t2, "[]") + "}";
  o += "},\n\"oneshot\":{\n\"datapath_f16\":" + oneshot_check_json(kind, true, 8, t0, t1, t2, "[]") + "}\n}\n";
  std::fputs(o.c_str(), stdout);
  return 0;
}

int cmd_parse() {
  char buf[8192];  // the server's own line buffer
  while (std::fgets(buf, sizeof(buf), stdin)) {
    std::string line = buf;
    strip_eol(&line);
    ServeRequest r;
    if (!parse_request(line, &r)) {
      std::printf("\"bad request\"\n");
      continue;
    }
    std::string devs;
    for (size_t i = 0; i < r.ords.size(); ++i)
      devs += json_format("%s[%d,%u,%.17g]", i ? "," : "", r.ords[i], r.nonces[i], r.timeouts[i]);
    std::printf("{\"tagged\":%s,\"id\":%llu,\"kind\":\"%s\",\"iters\":%d,\"timeout\":%.17g,\"mib\":%llu,\"devices\":[%s]}\n",
                r.tagged ? "true" : "false", r.id, r.kind.c_str(), r.iters, r.timeout_s, r.perf_mib, devs.c_str());
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "replies") return cmd_replies();
  if (cmd == "replies-bf16") return cmd_replies_bf16();
  if (cmd == "replies-fp8") return cmd_replies_fp8();
  if (cmd == "replies-f16") return cmd_replies_f16();
  if (cmd == "parse") return cmd_parse();
  std::fprintf(stderr, "usage: %s replies|replies-bf16|replies-fp8|replies-f16|parse\n", argv[0]);
  return 2;
}
