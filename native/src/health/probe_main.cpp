// mi355x-liveness-probe: run the gfx950 MFMA liveness kernel on GPU agents
// and print one JSON document.
//
//   mi355x-liveness-probe [--devices all|0,2,..] [--nonce N] [--iters N] [--identify] [--timeout S]
//   mi355x-liveness-probe --serve [--keep]  (long-lived; requests on stdin, see serve())
//   mi355x-liveness-probe --sweep [--devices ..]   (every CU of every XCD, see mi355x_chip_sweep)
//   mi355x-liveness-probe --perf [--perf-mib M]     (HBM bandwidth + pattern, sustained MFMA rate, clocks)
//   mi355x-liveness-probe --datapath [--devices ..] (full-width bit-exact MFMA operands, see mi355x_mfma_datapath)
//   mi355x-liveness-probe --datapath-i8 [--devices ..] (128-bit int8 operands, see mi355x_mfma_datapath_i8)
//   mi355x-liveness-probe --datapath-bf16 [--devices ..] (128-bit bf16 operands, see mi355x_mfma_datapath_bf16)
//   mi355x-liveness-probe --datapath-fp8 [--devices ..] (fp8 / MX-scaled operands, see mi355x_mfma_datapath_fp8)
//   mi355x-liveness-probe --datapath-f16 [--devices ..] (128- and 64-bit f16 operands, see mi355x_mfma_datapath_f16)
//   mi355x-liveness-probe --peer [--devices ..] [--peer-bytes B] [--peer-reps R]
//                                      (DMA copy over every GPU pair's link, verified)
//   --corrupt-word K[@O] / $MI355X_PROBE_CORRUPT_FILE: debug fault injection (see refresh_fault_injection)
//   --corrupt-datapath S:W:B[@O]: flip bit B of word W of workgroup 0's stage S tile before the datapath verdict
//   --corrupt-datapath-i8 S:W:B[@O]: the same for the int8 datapath check (S 0..4)
//   --corrupt-datapath-bf16 S:W:B[@O]: the same for the bf16 datapath check (S 0..4)
//   --corrupt-datapath-fp8 S:W:B[@O]: the same for the fp8 datapath check (S 0..7)
//   --corrupt-datapath-f16 S:W:B[@O]: the same for the f16 datapath check (S 0..6)
//
// Built twice from this file: `mi355x-liveness-probe` launches through ROCr
// directly (MI355X_PROBE_HSA; links only libhsa-runtime64, one AQL dispatch),
// `mi355x-liveness-probe-hip` through the HIP runtime.
//
// Exit status: 0 all probed devices live, 1 at least one failed, 2 usage or
// HIP runtime unavailable. The parent (the plugin's health loop, or the
// benchmark's fake container runtime) enforces the deadline by killing us.
#include <signal.h>
#include <sys/prctl.h>
#include <sys/resource.h>
#include <unistd.h>
#include <time.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "init_sampler.h"
#include "liveness_kernel.h"
#include "mi355x/liveness_probe.h"
#include "probe_json.h"
#include "probe_request.h"

// defined by the container-emulation builds (native/tools/probe_emu.cpp) only
extern "C" __attribute__((weak)) const char* mi355x_probe_view_json();

namespace {

double cpu_ms(double* user_ms = nullptr) {
  rusage ru;
  getrusage(RUSAGE_SELF, &ru);
  if (user_ms) *user_ms = ru.ru_utime.tv_sec * 1e3 + ru.ru_utime.tv_usec / 1e3;
  return (ru.ru_utime.tv_sec + ru.ru_stime.tv_sec) * 1e3 + (ru.ru_utime.tv_usec + ru.ru_stime.tv_usec) / 1e3;
}

// read syscalls issued so far (/proc/self/io "syscr"): ROCr's start-up is
// dominated by walking the kfd topology in sysfs, this makes that visible.
long long read_syscalls() {
  FILE* f = std::fopen("/proc/self/io", "r");
  if (!f) return -1;
  char line[128];
  long long v = -1;
  while (std::fgets(line, sizeof(line), f))
    if (std::sscanf(line, "syscr: %lld", &v) == 1) break;
  std::fclose(f);
  return v;
}

uint64_t mono_ns() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return static_cast<uint64_t>(ts.tv_sec) * 1000000000ull + ts.tv_nsec;
}

using mi355x::blank_result;
using mi355x::datapath_bf16_json;
using mi355x::datapath_fp8_json;
using mi355x::datapath_f16_json;
using mi355x::datapath_i8_json;
using mi355x::datapath_json;
using mi355x::json_escape;
using mi355x::parse_request;
using mi355x::perf_json;
using mi355x::ServeRequest;
using mi355x::sweep_json;

#ifdef MI355X_PROBE_HSA
constexpr bool kHsaBuild = true;
#else
constexpr bool kHsaBuild = false;
#endif

std::string device_json(const mi355x_probe_result& r) { return mi355x::device_json(r, kHsaBuild); }

#ifdef MI355X_PROBE_HSA
int device_count() { return mi355x_hsa_probe_init(); }
int probe(int o, uint32_t nonce, int iters, double timeout_s, mi355x_probe_result* r) {
  return mi355x_hsa_probe_device(o, nonce, iters, timeout_s, r);
}
int identify_dev(int o, mi355x_probe_result* r) { return mi355x_hsa_probe_identify(o, r); }
int peer(int a, int b, uint32_t nonce, uint64_t bytes, int reps, double timeout_s, mi355x_peer_result* r) {
  return mi355x_hsa_peer_probe(a, b, nonce, bytes, reps, timeout_s, r);
}
int chip_sweep(int o, uint32_t nonce, int iters, double timeout_s, mi355x_sweep_result* r) {
  return mi355x_hsa_chip_sweep(o, nonce, iters, timeout_s, r);
}
int perf_check(int o, uint32_t nonce, uint64_t bytes, int iters, double timeout_s, mi355x_perf_result* r) {
  return mi355x_hsa_perf_check(o, nonce, bytes, iters, timeout_s, r);
}
void perf_poison(uint64_t unit) { mi355x_hsa_perf_poison(unit); }
int datapath_check(int o, uint32_t nonce, double timeout_s, mi355x_datapath_result* r) {
  return mi355x_hsa_datapath_check(o, nonce, timeout_s, r);
}
void datapath_corrupt(int stage, int word, int bit, int ordinal) {
  mi355x_hsa_datapath_corrupt(stage, word, bit, ordinal);
}
int datapath_i8_check(int o, uint32_t nonce, double timeout_s, mi355x_datapath_i8_result* r) {
  return mi355x_hsa_datapath_i8_check(o, nonce, timeout_s, r);
}
void datapath_i8_corrupt(int stage, int word, int bit, int ordinal) {
  mi355x_hsa_datapath_i8_corrupt(stage, word, bit, ordinal);
}
int datapath_bf16_check(int o, uint32_t nonce, double timeout_s, mi355x_datapath_bf16_result* r) {
  return mi355x_hsa_datapath_bf16_check(o, nonce, timeout_s, r);
}
void datapath_bf16_corrupt(int stage, int word, int bit, int ordinal) {
  mi355x_hsa_datapath_bf16_corrupt(stage, word, bit, ordinal);
}
int datapath_fp8_check(int o, uint32_t nonce, double timeout_s, mi355x_datapath_fp8_result* r) {
  return mi355x_hsa_datapath_fp8_check(o, nonce, timeout_s, r);
}
void datapath_fp8_corrupt(int stage, int word, int bit, int ordinal) {
  mi355x_hsa_datapath_fp8_corrupt(stage, word, bit, ordinal);
}
int datapath_f16_check(int o, uint32_t nonce, double timeout_s, mi355x_datapath_f16_result* r) {
  return mi355x_hsa_datapath_f16_check(o, nonce, timeout_s, r);
}
void datapath_f16_corrupt(int stage, int word, int bit, int ordinal) {
  mi355x_hsa_datapath_f16_corrupt(stage, word, bit, ordinal);
}
void init_phases(double out[5]) { mi355x_hsa_init_phases(out); }
void defer_teardown() { mi355x_hsa_probe_defer_release(1); }
void teardown() { mi355x_hsa_probe_release(); }
void runtime_shutdown() { mi355x_hsa_probe_shutdown(); }
void keep_resources(bool on) { mi355x_hsa_probe_keep(on ? 1 : 0); }
void set_corrupt(int word, int ordinal) { mi355x_hsa_probe_corrupt(word, ordinal); }
void set_stream_mode(bool) {}  // the HSA path has one queue per device
#else
void set_stream_mode(bool own) { mi355x_probe_set_stream_mode(own ? 1 : 0); }
void set_corrupt(int, int) {}
void keep_resources(bool) {}  // the HIP build reuses its runtime's queues anyway
void init_phases(double out[5]) { out[0] = out[1] = out[2] = out[3] = out[4] = 0; }
void defer_teardown() { mi355x_probe_defer_release(1); }
void teardown() { mi355x_probe_release(); }
void runtime_shutdown() {}
int device_count() { return mi355x_probe_device_count(); }
int probe(int o, uint32_t nonce, int iters, double, mi355x_probe_result* r) {
  return mi355x_probe_device(o, nonce, iters, r);
}
int identify_dev(int o, mi355x_probe_result* r) { return mi355x_probe_identify(o, r); }
// the checks this build does not have: `blank` with the reason, status 1
template <typename R>
int needs_hsa_build(const char* flag, const R& blank, R* r) {
  *r = blank;
  std::snprintf(r->error, sizeof(r->error), "%s needs the HSA-direct build (mi355x-liveness-probe)", flag);
  return 1;
}
int chip_sweep(int o, uint32_t nonce, int iters, double, mi355x_sweep_result* r) {
  auto blank = blank_result<mi355x_sweep_result>(o, nonce);
  blank.iters = iters;
  return needs_hsa_build("--sweep", blank, r);
}
void perf_poison(uint64_t) {}
void datapath_corrupt(int, int, int, int) {}
int datapath_check(int o, uint32_t nonce, double, mi355x_datapath_result* r) {
  return needs_hsa_build("--datapath", blank_result<mi355x_datapath_result>(o, nonce), r);
}
void datapath_i8_corrupt(int, int, int, int) {}
int datapath_i8_check(int o, uint32_t nonce, double, mi355x_datapath_i8_result* r) {
  return needs_hsa_build("--datapath-i8", blank_result<mi355x_datapath_i8_result>(o, nonce), r);
}
void datapath_bf16_corrupt(int, int, int, int) {}
int datapath_bf16_check(int o, uint32_t nonce, double, mi355x_datapath_bf16_result* r) {
  return needs_hsa_build("--datapath-bf16", blank_result<mi355x_datapath_bf16_result>(o, nonce), r);
}
void datapath_fp8_corrupt(int, int, int, int) {}
int datapath_fp8_check(int o, uint32_t nonce, double, mi355x_datapath_fp8_result* r) {
  return needs_hsa_build("--datapath-fp8", blank_result<mi355x_datapath_fp8_result>(o, nonce), r);
}
void datapath_f16_corrupt(int, int, int, int) {}
int datapath_f16_check(int o, uint32_t nonce, double, mi355x_datapath_f16_result* r) {
  return needs_hsa_build("--datapath-f16", blank_result<mi355x_datapath_f16_result>(o, nonce), r);
}
int perf_check(int o, uint32_t nonce, uint64_t bytes, int iters, double, mi355x_perf_result* r) {
  auto blank = blank_result<mi355x_perf_result>(o, nonce);
  blank.bytes = bytes;
  blank.mfma_iters = iters;
  return needs_hsa_build("--perf", blank, r);
}
int peer(int a, int b, uint32_t, uint64_t bytes, int reps, double, mi355x_peer_result* r) {
  mi355x_peer_result blank{};
  blank.src = a;
  blank.dst = b;
  blank.bytes = bytes;
  blank.reps = reps;
  return needs_hsa_build("--peer", blank, r);
}
#endif

// Debug fault injection for tests of the verdict path on real hardware:
// "K" or "K@O" (flip one bit of output word K, on ordinal O only) from
// --corrupt-word, or from the file named by $MI355X_PROBE_CORRUPT_FILE, which
// is re-read before every request so a test can turn it on and off under a
// running server. Empty / missing = off.
int g_flag_corrupt_word = -1;
int g_flag_corrupt_ordinal = -1;

void parse_corrupt(const char* spec, int* word, int* ordinal) {
  *word = -1;
  *ordinal = -1;
  if (!spec || !*spec) return;
  char* end = nullptr;
  const long w = std::strtol(spec, &end, 0);
  if (end == spec) return;
  *word = static_cast<int>(w);
  if (*end == '@') *ordinal = std::atoi(end + 1);
}

void refresh_fault_injection() {
  int word = g_flag_corrupt_word, ordinal = g_flag_corrupt_ordinal;
  if (const char* path = std::getenv("MI355X_PROBE_CORRUPT_FILE")) {
    char buf[64] = {0};
    if (FILE* f = std::fopen(path, "r")) {
      if (!std::fgets(buf, sizeof(buf), f)) buf[0] = 0;
      std::fclose(f);
    }
    int fw, fo;
    parse_corrupt(buf, &fw, &fo);
    if (fw >= 0) {
      word = fw;
      ordinal = fo;
    }
  }
  set_corrupt(word, ordinal);
}

// Probe (or identify) a set of ordinals, one host thread per GPU so an 8-GPU
// request pays one device setup, not eight. Returns true when all are live.
bool run_batch(const std::vector<int>& ords, const std::vector<uint32_t>& nonces, int iters,
               const std::vector<double>& timeouts, bool identify, int n, std::vector<mi355x_probe_result>& results) {
  results.assign(ords.size(), mi355x_probe_result{});
  iters = probe_clamp_iters(iters);  // --iters and serve's "probe <iters>": the tile is exact up to the bound only
  std::vector<int> rcs(ords.size(), 1);
  auto run_one = [&](size_t i) {
    if (ords[i] < 0 || ords[i] >= n) {
      results[i].ordinal = ords[i];
      std::snprintf(results[i].error, sizeof(results[i].error), "no such GPU (count=%d)", n);
      return;
    }
    rcs[i] = identify ? identify_dev(ords[i], &results[i]) : probe(ords[i], nonces[i], iters, timeouts[i], &results[i]);
    if (identify && rcs[i] == 0) results[i].ok = 1;
  };
  if (ords.size() > 1) {
    std::vector<std::thread> ths;
    for (size_t i = 0; i < ords.size(); ++i) ths.emplace_back(run_one, i);
    for (auto& t : ths) t.join();
  } else if (!ords.empty()) {
    run_one(0);
  }
  bool all_ok = !ords.empty();
  for (int rc : rcs) all_ok = all_ok && rc == 0;
  return all_ok;
}

std::string peer_json(const mi355x_peer_result& r) {
  char buf[1024];
  std::snprintf(buf, sizeof(buf),
                "{\"src\":%d,\"dst\":%d,\"src_bus_id\":\"%s\",\"dst_bus_id\":\"%s\",\"ok\":%s,\"hsa_error\":%d,"
                "\"access\":%d,\"link_type\":%d,\"hops\":%u,\"numa_distance\":%u,\"link_max_bw_mbps\":%u,"
                "\"bytes\":%llu,\"reps\":%d,\"mismatches\":%llu,\"copy_us_best\":%.2f,\"gbps_best\":%.2f,"
                "\"total_us\":%.1f,\"error\":\"%s\"}",
                r.src, r.dst, json_escape(r.src_bus_id).c_str(), json_escape(r.dst_bus_id).c_str(),
                r.ok ? "true" : "false", r.hsa_error, r.access, r.link_type, r.hops, r.numa_distance,
                r.link_max_bw_mbps, static_cast<unsigned long long>(r.bytes), r.reps,
                static_cast<unsigned long long>(r.mismatches), r.copy_us_best, r.gbps_best, r.total_us,
                json_escape(r.error).c_str());
  return buf;
}

// --peer: every ordered pair of the selected GPUs (or the one GPU with itself),
// one pair at a time so each copy has its link to itself.
int run_peer(const std::vector<int>& ords, uint32_t nonce, uint64_t bytes, int reps, double timeout_s, int n) {
  std::vector<std::pair<int, int>> pairs;
  if (ords.size() == 1) {
    pairs.emplace_back(ords[0], ords[0]);
  } else {
    for (int a : ords)
      for (int b : ords)
        if (a != b) pairs.emplace_back(a, b);
  }
  bool all_ok = !pairs.empty();
  std::string o = "[";
  for (size_t i = 0; i < pairs.size(); ++i) {
    mi355x_peer_result r;
    const int rc = peer(pairs[i].first, pairs[i].second, nonce + static_cast<uint32_t>(i), bytes, reps, timeout_s, &r);
    all_ok = all_ok && rc == 0;
    if (i) o += ",";
    o += peer_json(r);
    if (r.hsa_error == -1) break;  // a copy is still in flight: stop touching the devices
  }
  std::printf("{\"peer\":true,\"ok\":%s,\"hip_device_count\":%d,\"t_ready_ns\":%llu,\"pairs\":%s]}\n",
              all_ok ? "true" : "false", n, static_cast<unsigned long long>(mono_ns()), o.c_str());
  std::fflush(stdout);
  return all_ok ? 0 : 1;
}

// A whole-chip check on each selected GPU, one host thread per GPU (every GPU
// has its own CUs, HBM and matrix cores): `call` runs it on one device,
// `to_json` prints that device's result. `json` becomes the reply's "devices"
// array; true when every device passed.
template <typename R, typename Call>
bool run_on_each(const std::vector<int>& ords, const std::vector<uint32_t>& nonces, const std::vector<double>& timeouts,
                 int n, Call call, std::string (*to_json)(const R&), std::string& json) {
  std::vector<R> res(ords.size());
  std::vector<int> rcs(ords.size(), 1);
  auto one = [&](size_t i) {
    if (ords[i] < 0 || ords[i] >= n) {
      res[i] = blank_result<R>(ords[i], 0);  // this reply carries no nonce
      std::snprintf(res[i].error, sizeof(res[i].error), "no such GPU (count=%d)", n);
      return;
    }
    rcs[i] = call(ords[i], nonces[i], timeouts[i], &res[i]);
  };
  std::vector<std::thread> ths;
  for (size_t i = 0; i < ords.size(); ++i) ths.emplace_back(one, i);
  for (auto& t : ths) t.join();
  bool ok = !ords.empty();
  json = "[";
  for (size_t i = 0; i < res.size(); ++i) {
    ok = ok && rcs[i] == 0;
    if (i) json += ",";
    json += to_json(res[i]);
  }
  json += "]";
  return ok;
}

// --sweep / --perf / --datapath / --datapath-i8 / --datapath-bf16 / --datapath-fp8 / --datapath-f16 and the
// server's requests of those kinds.
// `iters`: the sweep's tile iterations or the throughput check's MFMA
// iterations; `bytes`: the throughput check's HBM buffer.
bool run_check(const std::string& kind, const std::vector<int>& ords, const std::vector<uint32_t>& nonces, int iters,
               uint64_t bytes, const std::vector<double>& timeouts, int n, std::string& json) {
  if (kind == "sweep")
    return run_on_each(ords, nonces, timeouts, n, [=](int o, uint32_t nonce, double t, mi355x_sweep_result* r) {
      return chip_sweep(o, nonce, iters, t, r);
    }, sweep_json, json);
  if (kind == "perf")
    return run_on_each(ords, nonces, timeouts, n, [=](int o, uint32_t nonce, double t, mi355x_perf_result* r) {
      return perf_check(o, nonce, bytes, iters, t, r);
    }, perf_json, json);
  if (kind == "datapath_i8")
    return run_on_each(ords, nonces, timeouts, n, [](int o, uint32_t nonce, double t, mi355x_datapath_i8_result* r) {
      return datapath_i8_check(o, nonce, t, r);
    }, datapath_i8_json, json);
  if (kind == "datapath_bf16")
    return run_on_each(ords, nonces, timeouts, n, [](int o, uint32_t nonce, double t, mi355x_datapath_bf16_result* r) {
      return datapath_bf16_check(o, nonce, t, r);
    }, datapath_bf16_json, json);
  if (kind == "datapath_fp8")
    return run_on_each(ords, nonces, timeouts, n, [](int o, uint32_t nonce, double t, mi355x_datapath_fp8_result* r) {
      return datapath_fp8_check(o, nonce, t, r);
    }, datapath_fp8_json, json);
  if (kind == "datapath_f16")
    return run_on_each(ords, nonces, timeouts, n, [](int o, uint32_t nonce, double t, mi355x_datapath_f16_result* r) {
      return datapath_f16_check(o, nonce, t, r);
    }, datapath_f16_json, json);
  return run_on_each(ords, nonces, timeouts, n, [](int o, uint32_t nonce, double t, mi355x_datapath_result* r) {
    return datapath_check(o, nonce, t, r);
  }, datapath_json, json);
}

// "S:W:B" or "S:W:B@O" of --corrupt-datapath and of its -i8, -bf16, -fp8 and -f16 siblings
bool parse_corrupt_datapath(const char* spec, int out[4]) {
  out[3] = -1;
  char tail = 0;
  const int n = std::sscanf(spec, "%d:%d:%d@%d%c", &out[0], &out[1], &out[2], &out[3], &tail);
  return n == 3 || n == 4;
}

std::string devices_json(const std::vector<mi355x_probe_result>& results) {
  std::string o = "[";
  for (size_t i = 0; i < results.size(); ++i) {
    if (i) o += ",";
    o += device_json(results[i]);
  }
  return o + "]";
}

// --serve: a long-lived prober for the plugin's health loop. The runtime is
// initialised once; every request line
//     [@<id> ]probe <iters> <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]sweep <iters> <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]perf <mfma_iters> <timeout_s> <mib> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]datapath <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]datapath_i8 <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]datapath_bf16 <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]datapath_fp8 <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]datapath_f16 <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
// is answered with one JSON line {"id":..,"ok":..,"t_ready_ns":..,"devices":[..]}
// ("id" only for a tagged request). A device's own deadline replaces the
// request's timeout for that device: the plugin gives GPUs that run other
// processes' kernels a short one, since a dispatch queued behind them is
// inconclusive anyway and its verdict is collected by the next request.
// Tagged requests are answered on worker threads, in completion order (the
// HSA build): a PreStartContainer check of one GPU never waits behind a
// health sweep still waiting for another GPU. Requests on the same device
// serialise on its kept queue (each waits no longer than its own deadline).
// "quit" or EOF on stdin ends the server, and so does the parent's death
// (PR_SET_PDEATHSIG). Spawning a fresh probe process per pulse would create
// and tear down a kfd process each time, and a GPU process that starts while
// such a teardown is in flight blocks in open("/dev/kfd") for up to ~150 ms
// (profiles/archive/measurements_r1_r3.md §3c): a pod admitted during a health sweep would pay it.
// With --keep the per-device queue, executable and buffers also stay: a probe
// is then one AQL packet, with no queue creation (an HWS runlist update that
// preempts every queue on that GPU, ~5 ms, profiles/archive/measurements_r1_r3.md §3f) per pulse.
#ifdef MI355X_PROBE_HSA
constexpr bool kConcurrentServe = true;
#else
constexpr bool kConcurrentServe = false;  // the HIP build answers in order
#endif
constexpr int kMaxServeWorkers = 64;  // beyond this a tagged request is answered inline

std::mutex g_out_mu;

void emit_line(const std::string& s) {
  std::lock_guard<std::mutex> lk(g_out_mu);
  std::fputs(s.c_str(), stdout);
  std::fputc('\n', stdout);
  std::fflush(stdout);
}

// One request, start to reply line; then the runtime's deferred frees.
void answer(const ServeRequest& r, int n) {
  refresh_fault_injection();
  defer_teardown();
  std::string body;
  bool ok;
  if (r.kind != "probe") {
    ok = run_check(r.kind, r.ords, r.nonces, r.iters, static_cast<uint64_t>(r.perf_mib) << 20, r.timeouts, n, body);
  } else {
    std::vector<mi355x_probe_result> results;
    ok = run_batch(r.ords, r.nonces, r.iters, r.timeouts, false, n, results);
    body = devices_json(results);
  }
  emit_line(mi355x::serve_reply_json(r.tagged, r.id, r.kind, ok, n, mono_ns(), body));
  teardown();  // queues/executables go, the runtime (and the kfd process) stays
}

// Tagged requests go to a pool of worker threads that stay for the server's
// life (a thread per request cost its creation on every probe); the pool
// grows while every worker is busy -- a request stuck on a wedged device
// holds its worker, not the others -- up to kMaxServeWorkers, beyond which
// a request is answered inline.
struct ServePool {
  std::mutex mu;
  std::condition_variable cv, done;
  std::deque<ServeRequest> q;
  int workers = 0, idle = 0, busy = 0;
  bool stop = false;
};

void serve_worker(ServePool* pool, int n) {
  while (true) {
    ServeRequest r;
    {
      std::unique_lock<std::mutex> lk(pool->mu);
      pool->idle++;
      pool->cv.wait(lk, [pool] { return pool->stop || !pool->q.empty(); });
      pool->idle--;
      if (pool->q.empty()) return;  // stopping
      r = std::move(pool->q.front());
      pool->q.pop_front();
      pool->busy++;
    }
    answer(r, n);  // no lock held: a request may take its whole deadline
    {
      std::lock_guard<std::mutex> lk(pool->mu);
      pool->busy--;
    }
    pool->done.notify_all();
  }
}

int serve(int n, uint64_t t_start, uint64_t t_runtime) {
  prctl(PR_SET_PDEATHSIG, SIGKILL);
  if (getppid() == 1) return 0;  // parent already gone
  emit_line(mi355x::serve_hello_json(n, kConcurrentServe, t_start, t_runtime));
  if (n < 0) return 2;
  ServePool pool;
  std::vector<std::thread> threads;
  std::string line;
  char buf[8192];
  while (std::fgets(buf, sizeof(buf), stdin)) {
    line = buf;
    mi355x::strip_eol(&line);
    if (line.empty()) continue;
    if (line == "quit") break;
    ServeRequest r;
    if (!parse_request(line, &r)) {
      emit_line(mi355x::bad_request_json(r.tagged, r.id));
      continue;
    }
    bool queued = false;
    if (r.tagged && kConcurrentServe) {
      std::lock_guard<std::mutex> lk(pool.mu);
      if (pool.idle > static_cast<int>(pool.q.size()) || pool.workers < kMaxServeWorkers) {
        if (pool.idle <= static_cast<int>(pool.q.size())) {
          pool.workers++;
          threads.emplace_back(serve_worker, &pool, n);
        }
        pool.q.push_back(std::move(r));
        pool.cv.notify_one();
        queued = true;
      }
    }
    if (!queued) answer(r, n);
  }
  {
    // every worker's waits are bounded by its deadlines; one stuck inside the
    // runtime past that keeps the runtime up: exit without shutting it down
    std::unique_lock<std::mutex> lk(pool.mu);
    const bool drained =
        pool.done.wait_for(lk, std::chrono::seconds(60), [&] { return pool.q.empty() && pool.busy == 0; });
    if (!drained) {
      std::fflush(stdout);
      std::_Exit(0);
    }
    pool.stop = true;
    pool.cv.notify_all();
  }
  for (auto& t : threads) t.join();
  runtime_shutdown();
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t t_start = mono_ns();
  std::string devices = "all";
  uint32_t nonce = static_cast<uint32_t>(t_start ^ (t_start >> 32));
  int iters = 4;
  double timeout_s = 5.0;
  bool identify = false;
  int sample_us = 0;
  std::string exit_mode = "shutdown";
  bool serve_mode = false;
  bool keep = false;  // --serve --keep: per-device queue/executable/buffers live across requests
  bool peer_mode = false;
  bool sweep_mode = false;
  bool perf_mode = false;
  bool datapath_mode = false;
  bool datapath_i8_mode = false;
  bool datapath_bf16_mode = false;
  bool datapath_fp8_mode = false;
  bool datapath_f16_mode = false;
  uint64_t perf_mib = 4096;
  int perf_iters = 1 << 16;
  uint64_t peer_bytes = 64ull << 20;
  int peer_reps = 3;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&](const char* what) -> const char* {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "missing value for %s\n", what);
        std::exit(2);
      }
      return argv[++i];
    };
    if (a == "--devices") {
      devices = next("--devices");
    } else if (a == "--nonce") {
      nonce = static_cast<uint32_t>(std::strtoul(next("--nonce"), nullptr, 0));
    } else if (a == "--iters") {
      iters = std::atoi(next("--iters"));
    } else if (a == "--timeout") {
      timeout_s = std::atof(next("--timeout"));
    } else if (a == "--sample-init") {
      sample_us = std::atoi(next("--sample-init"));
    } else if (a == "--exit") {
      exit_mode = next("--exit");
      if (exit_mode != "shutdown" && exit_mode != "release" && exit_mode != "fast") {
        std::fprintf(stderr, "--exit must be shutdown|release|fast\n");
        return 2;
      }
    } else if (a == "--identify") {
      identify = true;
    } else if (a == "--serve") {
      serve_mode = true;
    } else if (a == "--keep") {
      keep = true;
    } else if (a == "--peer") {
      peer_mode = true;
    } else if (a == "--sweep") {
      sweep_mode = true;
    } else if (a == "--perf") {
      perf_mode = true;
    } else if (a == "--datapath") {
      datapath_mode = true;
    } else if (a == "--corrupt-datapath") {
      int c[4];
      if (!parse_corrupt_datapath(next("--corrupt-datapath"), c)) {
        std::fprintf(stderr, "--corrupt-datapath must be STAGE:WORD:BIT[@ORDINAL]\n");
        return 2;
      }
      datapath_corrupt(c[0], c[1], c[2], c[3]);
    } else if (a == "--datapath-i8") {
      datapath_i8_mode = true;
    } else if (a == "--corrupt-datapath-i8") {
      int c[4];
      if (!parse_corrupt_datapath(next("--corrupt-datapath-i8"), c)) {
        std::fprintf(stderr, "--corrupt-datapath-i8 must be STAGE:WORD:BIT[@ORDINAL]\n");
        return 2;
      }
      datapath_i8_corrupt(c[0], c[1], c[2], c[3]);
    } else if (a == "--datapath-bf16") {
      datapath_bf16_mode = true;
    } else if (a == "--corrupt-datapath-bf16") {
      int c[4];
      if (!parse_corrupt_datapath(next("--corrupt-datapath-bf16"), c)) {
        std::fprintf(stderr, "--corrupt-datapath-bf16 must be STAGE:WORD:BIT[@ORDINAL]\n");
        return 2;
      }
      datapath_bf16_corrupt(c[0], c[1], c[2], c[3]);
    } else if (a == "--datapath-fp8") {
      datapath_fp8_mode = true;
    } else if (a == "--corrupt-datapath-fp8") {
      int c[4];
      if (!parse_corrupt_datapath(next("--corrupt-datapath-fp8"), c)) {
        std::fprintf(stderr, "--corrupt-datapath-fp8 must be STAGE:WORD:BIT[@ORDINAL]\n");
        return 2;
      }
      datapath_fp8_corrupt(c[0], c[1], c[2], c[3]);
    } else if (a == "--datapath-f16") {
      datapath_f16_mode = true;
    } else if (a == "--corrupt-datapath-f16") {
      int c[4];
      if (!parse_corrupt_datapath(next("--corrupt-datapath-f16"), c)) {
        std::fprintf(stderr, "--corrupt-datapath-f16 must be STAGE:WORD:BIT[@ORDINAL]\n");
        return 2;
      }
      datapath_f16_corrupt(c[0], c[1], c[2], c[3]);
    } else if (a == "--perf-mib") {
      perf_mib = std::strtoull(next("--perf-mib"), nullptr, 0);
    } else if (a == "--perf-iters") {
      perf_iters = std::atoi(next("--perf-iters"));
    } else if (a == "--poison-hbm") {
      perf_poison(std::strtoull(next("--poison-hbm"), nullptr, 0));
    } else if (a == "--peer-bytes") {
      peer_bytes = std::strtoull(next("--peer-bytes"), nullptr, 0);
    } else if (a == "--corrupt-word") {
      parse_corrupt(next("--corrupt-word"), &g_flag_corrupt_word, &g_flag_corrupt_ordinal);
    } else if (a == "--hip-stream") {
      const std::string m = next("--hip-stream");
      if (m != "own" && m != "null") {
        std::fprintf(stderr, "--hip-stream must be own|null\n");
        return 2;
      }
      set_stream_mode(m == "own");
    } else if (a == "--peer-reps") {
      peer_reps = std::atoi(next("--peer-reps"));
    } else if (a == "-h" || a == "--help") {
      std::printf("usage: %s [--devices all|0,1,..] [--nonce N] [--iters N] [--identify] [--timeout S] "
                  "[--sample-init PERIOD_US] [--exit shutdown|release|fast] [--serve [--keep]] [--peer [--peer-bytes B] [--peer-reps R]] [--sweep] "
                  "[--perf [--perf-mib M] [--perf-iters N] [--poison-hbm UNIT]] [--datapath [--corrupt-datapath S:W:B[@ORDINAL]]] "
                  "[--datapath-i8 [--corrupt-datapath-i8 S:W:B[@ORDINAL]]] "
                  "[--datapath-bf16 [--corrupt-datapath-bf16 S:W:B[@ORDINAL]]] "
                  "[--datapath-fp8 [--corrupt-datapath-fp8 S:W:B[@ORDINAL]]] "
                  "[--datapath-f16 [--corrupt-datapath-f16 S:W:B[@ORDINAL]]] "
                  "[--corrupt-word K[@ORDINAL]] [--hip-stream own|null]\n",
                  argv[0]);
      return 0;
    } else {
      std::fprintf(stderr, "unknown argument %s\n", a.c_str());
      return 2;
    }
  }

  mi355x::InitSampler sampler(sample_us > 0 ? sample_us : 1);
  if (sample_us > 0) sampler.start();
  const int n = device_count();
  if (sample_us > 0) sampler.stop();
  const std::string init_profile = sample_us > 0 ? sampler.json() : "null";
  const uint64_t t_runtime = mono_ns();  // HIP runtime + ROCr initialised
  double cpu_user_runtime = 0;
  const double cpu_runtime = cpu_ms(&cpu_user_runtime);
  const long long syscr_runtime = read_syscalls();
  // the view's effect on the runtime's start-up walk, read at the same point as syscr
  const std::string view_runtime = mi355x_probe_view_json ? mi355x_probe_view_json() : "";
  double iph[5];
  init_phases(iph);
  if (serve_mode) {
    keep_resources(keep);
    return serve(n, t_start, t_runtime);
  }
  if (n < 0) {
    std::printf("%s\n", mi355x::runtime_init_failed_json(-n, t_start, init_profile).c_str());
    return 2;
  }
  std::vector<int> ords;
  if (devices == "all") {
    for (int i = 0; i < n; ++i) ords.push_back(i);
  } else {
    size_t pos = 0;
    while (pos <= devices.size()) {
      size_t c = devices.find(',', pos);
      if (c == std::string::npos) c = devices.size();
      std::string tok = devices.substr(pos, c - pos);
      if (!tok.empty()) ords.push_back(std::atoi(tok.c_str()));
      pos = c + 1;
    }
  }

  if (peer_mode) return run_peer(ords, nonce, peer_bytes, peer_reps, timeout_s, n);
  std::vector<uint32_t> nonces;
  for (size_t i = 0; i < ords.size(); ++i) nonces.push_back(nonce + static_cast<uint32_t>(i));
  const std::vector<double> timeouts(ords.size(), timeout_s);
  if (perf_mode || datapath_mode || datapath_i8_mode || datapath_bf16_mode || datapath_fp8_mode ||
      datapath_f16_mode || sweep_mode) {
    const char* kind = perf_mode ? "perf" : datapath_mode ? "datapath" : datapath_i8_mode ? "datapath_i8"
                       : datapath_bf16_mode ? "datapath_bf16" : datapath_fp8_mode ? "datapath_fp8"
                       : datapath_f16_mode ? "datapath_f16" : "sweep";
    std::string body;
    const bool ok = run_check(kind, ords, nonces, perf_mode ? perf_iters : iters, perf_mib << 20, timeouts, n, body);
    std::printf("%s\n", mi355x::oneshot_check_json(kind, ok, n, t_start, t_runtime, mono_ns(), body).c_str());
    std::fflush(stdout);
    return ok ? 0 : 1;
  }
  std::vector<mi355x_probe_result> results;
  // Queues/executables are torn down after the verdict is printed: the caller
  // (container runtime, health loop) only waits for the JSON line.
  refresh_fault_injection();
  defer_teardown();
  const bool all_ok = run_batch(ords, nonces, iters, timeouts, identify, n, results);
  const uint64_t t_ready = mono_ns();
  const double cpu_ready = cpu_ms();
  const mi355x::OneshotProbeTimes times = {t_start, t_runtime, t_ready, cpu_runtime, cpu_user_runtime, cpu_ready,
                                           syscr_runtime, {iph[0], iph[1], iph[2], iph[3], iph[4]}};
  std::printf("%s\n", mi355x::oneshot_probe_json(all_ok, n, identify, times, init_profile,
                                                 mi355x_probe_view_json ? view_runtime : "null", devices_json(results))
                          .c_str());
  std::fflush(stdout);
  // After the verdict. The exit mode was an experiment: the kernel's kfd
  // process teardown after we are gone costs the same either way
  // (profiles/archive/measurements_r1_r3.md §3c).
  const int code = all_ok ? 0 : 1;
  if (exit_mode == "fast") std::_Exit(code);
  teardown();
  if (exit_mode == "shutdown") runtime_shutdown();
  return code;
}
