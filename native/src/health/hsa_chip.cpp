// The full-chip sweep (mi355x_hsa_chip_sweep: every CU of every XCD runs the
// MFMA tile and reports where it ran), the throughput check
// (mi355x_hsa_perf_check: HBM write / read over a verified pattern, sustained
// bf16 MFMA rate, per-XCD clocks) and the MFMA datapath check
// (mi355x_hsa_datapath_check: full-width operands, bit-exact) and its int8
// and bf16 siblings (mi355x_hsa_datapath_i8_check, mi355x_hsa_datapath_bf16_check:
// 128-bit operands; mi355x_hsa_datapath_fp8_check: fp8 and MX-scaled operands;
// mi355x_hsa_datapath_f16_check: f16 operands, the legacy 64-bit forms too), all on the
// device's kept queue when there is one. They share one path: Check
// (the steps before a check's own part, the timed dispatch, the return
// conventions), DeviceWork (the queue and executable) and Buffers (the pool
// memory, owned). A dispatch that outlives its deadline is parked in an
// in-flight registry with everything it may still write.
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "chip_verify.h"
#include "datapath_bf16_verify.h"
#include "datapath_f16_verify.h"
#include "datapath_fp8_verify.h"
#include "datapath_i8_verify.h"
#include "datapath_verify.h"
#include "hsa_runtime.h"
#include "probe_json.h"
#include "probe_verify.h"

using namespace mi355x::hsa_rt;  // NOLINT(build/namespaces)

namespace mi355x::hsa_rt {
namespace {

// A chip sweep or check whose completion signal did not fire within its
// deadline: the dispatch may still write its records, so none of its resources
// can be freed until it completes. One per device at most (Check::begin
// refuses to submit another while it is outstanding).
struct SweepInFlight {
  hsa_code_object_reader_t reader{};  // null when the kept queue / executable were borrowed
  hsa_executable_t exe{};
  hsa_queue_t* queue = nullptr;
  std::shared_ptr<SigRef> sig;
  std::vector<void*> bufs;  // in allocation order (Buffers::release)
  std::chrono::steady_clock::time_point since{};

  void release() {
    for (auto it = bufs.rbegin(); it != bufs.rend(); ++it) H().hsa_amd_memory_pool_free(*it);
    if (queue) H().hsa_queue_destroy(queue);
    if (exe.handle) H().hsa_executable_destroy(exe);
    if (reader.handle) H().hsa_code_object_reader_destroy(reader);
    sig.reset();
  }
};
std::mutex g_sweep_mu;
std::vector<std::pair<int, SweepInFlight>> g_sweep_in_flight;

}  // namespace

// > 0 (seconds outstanding) when an earlier sweep or throughput check on
// `ordinal` is still running; a completed one is freed here.
double in_flight_for(int ordinal) {
  std::lock_guard<std::mutex> lk(g_sweep_mu);
  for (auto it = g_sweep_in_flight.begin(); it != g_sweep_in_flight.end(); ++it) {
    if (it->first != ordinal) continue;
    if (H().hsa_signal_load_scacquire(it->second.sig->s) < 1) {
      it->second.release();
      g_sweep_in_flight.erase(it);
      return 0;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - it->second.since).count();
    return s > 0 ? s : 1e-9;
  }
  return 0;
}

// runtime shutdown: an outstanding sweep's resources go with the runtime
void forget_in_flight_sweeps() {
  std::lock_guard<std::mutex> lk(g_sweep_mu);
  // a dispatch still running may yet decrement its completion signal: leave
  // the signal to the runtime's own teardown instead of destroying it here
  for (auto& e : g_sweep_in_flight)
    if (e.second.sig && e.second.sig->s.handle && H().hsa_signal_load_scacquire(e.second.sig->s) >= 1)
      e.second.sig->s = hsa_signal_t{};
  g_sweep_in_flight.clear();
}

namespace {

// One AQL kernel dispatch (barrier bit, system-scope fences), no wait.
void submit_kernel(hsa_queue_t* queue, uint64_t kobj, uint32_t gseg, uint32_t pseg, void* kargs, uint32_t wgs,
                   uint32_t wg_threads, hsa_signal_t sig) {
  H().hsa_signal_store_screlease(sig, 1);
  const uint64_t idx = H().hsa_queue_add_write_index_screlease(queue, 1);
  auto* pkt = static_cast<hsa_kernel_dispatch_packet_t*>(queue->base_address) + (idx & (queue->size - 1));
  std::memset(reinterpret_cast<char*>(pkt) + 4, 0, sizeof(*pkt) - 4);
  pkt->workgroup_size_x = static_cast<uint16_t>(wg_threads);
  pkt->workgroup_size_y = 1;
  pkt->workgroup_size_z = 1;
  pkt->grid_size_x = wgs * wg_threads;
  pkt->grid_size_y = 1;
  pkt->grid_size_z = 1;
  pkt->private_segment_size = pseg;
  pkt->group_segment_size = gseg;
  pkt->kernel_object = kobj;
  pkt->kernarg_address = kargs;
  pkt->completion_signal = sig;
  const uint16_t header = static_cast<uint16_t>(
      (HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) | (1 << HSA_PACKET_HEADER_BARRIER) |
      (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) |
      (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE));
  const uint16_t setup = 1 << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS;
  __atomic_store_n(reinterpret_cast<uint32_t*>(pkt), header | (static_cast<uint32_t>(setup) << 16), __ATOMIC_RELEASE);
  H().hsa_signal_store_screlease(queue->doorbell_signal, static_cast<hsa_signal_value_t>(idx));
}

double dispatch_us(const Agent& ag, hsa_signal_t sig) {
  hsa_amd_profiling_dispatch_time_t dt{};
  if (H().hsa_amd_profiling_get_dispatch_time(ag.agent, sig, &dt) != HSA_STATUS_SUCCESS || !g_rt.ts_freq) return 0;
  return static_cast<double>(dt.end - dt.start) * 1e6 / static_cast<double>(g_rt.ts_freq);
}

void set_hsa_error(int* err, char* buf, size_t n, hsa_status_t st, const char* what) {
  *err = static_cast<int>(st);
  const char* msg = nullptr;
  H().hsa_status_string(st, &msg);
  std::snprintf(buf, n, "%s: %s", what, msg ? msg : "hsa error");
}

// The pool memory of one check. It frees what it holds, last allocated first,
// when it goes out of scope -- unless a dispatch that outlived its deadline
// took it along (release). The first failing step is kept (status, what) and
// every later step does nothing, so a check sets all its buffers up and then
// looks at ok() once.
class Buffers {
 public:
  Buffers() = default;
  Buffers(const Buffers&) = delete;
  Buffers& operator=(const Buffers&) = delete;
  ~Buffers() { free(); }

  bool ok() const { return status == HSA_STATUS_SUCCESS; }

  // `bytes` from `pool`; with `allow`, that agent gets access to them
  template <typename T>
  T* alloc(hsa_amd_memory_pool_t pool, size_t bytes, const char* label, const Agent* allow = nullptr,
           const char* allow_label = nullptr) {
    void* p = nullptr;
    if (!ok() || !step(H().hsa_amd_memory_pool_allocate(pool, bytes, 0, &p), label)) return nullptr;
    held_.push_back(p);
    if (allow) step(H().hsa_amd_agents_allow_access(1, &allow->agent, nullptr, p), allow_label);
    return static_cast<T*>(p);
  }
  void fill(uint32_t* p, uint32_t value, size_t words, const char* label) {
    if (ok()) step(H().hsa_amd_memory_fill(p, value, words), label);
  }
  void free() {
    for (; !held_.empty(); held_.pop_back()) H().hsa_amd_memory_pool_free(held_.back());
  }
  // everything held, in allocation order; this set owns nothing afterwards
  std::vector<void*> release() { return std::exchange(held_, {}); }

  hsa_status_t status = HSA_STATUS_SUCCESS;
  const char* what = "";

 private:
  bool step(hsa_status_t st, const char* label) {
    if (ok() && st != HSA_STATUS_SUCCESS) {
      status = st;
      what = label;
    }
    return ok();
  }
  std::vector<void*> held_;
};

// The queue and executable a chip sweep or throughput check runs on. With kept
// resources (--serve --keep) the device's kept queue and executable are
// borrowed -- set up here if no probe has yet -- so the check adds no kfd
// queue: no 181 MB context-save area, no HWS runlist update. The slot's mutex
// is held meanwhile, so no probe packet interleaves. Otherwise a private queue
// and executable are created for the check and destroyed after it.
struct DeviceWork {
  DeviceWork() = default;
  DeviceWork(const DeviceWork&) = delete;
  DeviceWork& operator=(const DeviceWork&) = delete;
  ~DeviceWork() {
    if (abandoned || borrowed()) return;
    if (queue) H().hsa_queue_destroy(queue);
    if (exe.handle) H().hsa_executable_destroy(exe);
    if (reader.handle) H().hsa_code_object_reader_destroy(reader);
  }
  bool borrowed() const { return slot != nullptr; }

  hsa_status_t open(const Agent& agent, int ordinal, const char** what) {
    ag = &agent;
    bool keep;
    {
      std::lock_guard<std::mutex> lk(g_resident_mu);
      keep = g_keep;
    }
    if (keep) {
      Resident* s = resident_slot(ordinal);
      std::unique_lock<std::timed_mutex> lk(s->mu);
      if (!s->ready && !s->pending && !s->blocker) {
        mi355x_probe_result scratch;
        std::memset(&scratch, 0, sizeof(scratch));
        if (setup_resources(agent, s->r, s->k, &scratch))
          s->ready = true;
        else
          s->r.release();
      }
      if (s->ready && !s->pending && !s->blocker) {
        slot = s;
        slot_lk = std::move(lk);
        exe = s->r.exe;
        queue = s->r.queue;
      }
    }
    hsa_status_t st = HSA_STATUS_SUCCESS;
    if (!borrowed()) {
      const size_t co_size = static_cast<size_t>(mi355x_hsaco_end - mi355x_hsaco_start);
      if ((st = H().hsa_code_object_reader_create_from_memory(mi355x_hsaco_start, co_size, &reader)) != 0)
        return *what = "code object", st;
      if ((st = H().hsa_executable_create_alt(HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr,
                                              &exe)) != 0)
        return *what = "executable create", st;
      if ((st = H().hsa_executable_load_agent_code_object(exe, agent.agent, reader, nullptr, nullptr)) != 0)
        return *what = "load code object", st;
      if ((st = H().hsa_executable_freeze(exe, nullptr)) != 0) return *what = "freeze", st;
      if ((st = H().hsa_queue_create(agent.agent, 64, HSA_QUEUE_TYPE_SINGLE, nullptr, nullptr, UINT32_MAX, UINT32_MAX,
                                     &queue)) != 0)
        return *what = "queue create", st;
      H().hsa_amd_profiling_set_profiler_enabled(queue, 1);
    }
    if ((st = H().hsa_signal_create(1, 0, nullptr, &sig->s)) != 0) return *what = "signal create", st;
    return st;
  }

  hsa_status_t symbol(const char* name, KernelInfo* k) {
    hsa_executable_symbol_t sym{};
    const hsa_status_t st = H().hsa_executable_get_symbol_by_name(exe, name, &ag->agent, &sym);
    if (st != HSA_STATUS_SUCCESS) return st;
    H().hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &k->kobj);
    H().hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE, &k->kseg);
    H().hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &k->gseg);
    H().hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &k->pseg);
    return st;
  }

  void submit(const KernelInfo& k, void* kargs, uint32_t wgs, uint32_t wg_threads) {
    submit_kernel(queue, k.kobj, k.gseg, k.pseg, kargs, wgs, wg_threads, sig->s);
  }

  // A dispatch did not complete within its deadline: everything it may still
  // write goes to the in-flight registry (at most one per device: later sweeps
  // and checks fail fast until it completes), and a borrowed kept queue blocks
  // probes until then.
  void abandon(int ordinal, Buffers& bufs, std::chrono::steady_clock::time_point since) {
    abandoned = true;
    SweepInFlight f;
    if (!borrowed()) {
      f.reader = reader;
      f.exe = exe;
      f.queue = queue;
    }
    f.sig = sig;
    f.bufs = bufs.release();
    f.since = since;
    {
      std::lock_guard<std::mutex> lk(g_sweep_mu);
      g_sweep_in_flight.emplace_back(ordinal, std::move(f));
    }
    if (borrowed()) {
      slot->blocker = sig;
      slot->blocked_since = since;  // when the sweep / check was submitted
    }
  }

  const Agent* ag = nullptr;
  Resident* slot = nullptr;
  std::unique_lock<std::timed_mutex> slot_lk;
  hsa_code_object_reader_t reader{};
  hsa_executable_t exe{};
  hsa_queue_t* queue = nullptr;
  std::shared_ptr<SigRef> sig = std::make_shared<SigRef>();
  bool abandoned = false;
};

struct KernelSpec {
  const char* symbol;
  size_t args_bytes;  // what the host writes: the code object's kernarg segment must hold it
};

// What the checks have in common, over their result types (which share field
// names, not layout): begin() up to the kernels' symbols, run() for one timed
// dispatch, finish() / fail() for the return value. Where begin() or run()
// return false, `out` holds the error and the check returns 1.
template <typename R>
struct Check {
  using clk = std::chrono::steady_clock;

  Check(int ordinal, double timeout_s, R* out) : ordinal(ordinal), timeout_s(timeout_s), out(out) {}

  // `needs_device_memory`: the check allocates from the agent's own pool.
  // `grid` is the result field for the workgroup count, `wgs_per_cu` per CU.
  // `ks` receives one KernelInfo per spec; `kind` names the check in the
  // kernarg-segment message.
  bool begin(bool needs_device_memory, int R::*grid, uint32_t wgs_per_cu, const char* kind,
             std::initializer_list<KernelSpec> specs, KernelInfo* ks) {
    const int n = mi355x_hsa_probe_init();
    if (n < 0) {
      out->hsa_error = n;
      std::snprintf(out->error, sizeof(out->error), "hsa_init: %.140s", H().loaded ? "runtime init failed" : H().error);
      return false;
    }
    if (ordinal < 0 || ordinal >= n) {
      std::snprintf(out->error, sizeof(out->error), "no such GPU agent (count=%d)", n);
      return false;
    }
    if (const double s = in_flight_for(ordinal); s > 0) {
      ag = &g_rt.gpus[ordinal];
      identify();
      out->in_flight_s = s;
      out->hsa_error = -1;
      std::snprintf(out->error, sizeof(out->error),
                    "earlier chip sweep / check still in flight for %.1fs (not completed)", s);
      return finish(), false;
    }
    ag = &g_rt.gpus[ordinal];
    identify();
    uint32_t cus = 0, xcc = 0;
    H().hsa_agent_get_info(ag->agent, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_COMPUTE_UNIT_COUNT), &cus);
    H().hsa_agent_get_info(ag->agent, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_NUM_XCC), &xcc);
    out->cu_count = static_cast<int>(cus);
    out->num_xcc = static_cast<int>(xcc);
    if (cus == 0 || cus > 1024 || !g_rt.has_fine || !g_rt.has_kernarg || (needs_device_memory && !ag->has_coarse)) {
      std::snprintf(out->error, sizeof(out->error), "unexpected agent (cus=%u) or missing memory pool", cus);
      return false;
    }
    out->*grid = static_cast<int>(cus * wgs_per_cu);

    const char* what = "";
    hsa_status_t s = dw.open(*ag, ordinal, &what);
    if (s != HSA_STATUS_SUCCESS) return fail(s, what), false;
    out->kept_queue = dw.borrowed() ? 1 : 0;
    std::string segs;
    bool fits = true;
    for (const KernelSpec& spec : specs) {
      if ((s = dw.symbol(spec.symbol, ks)) != HSA_STATUS_SUCCESS) return fail(s, "kernel symbol"), false;
      segs += (segs.empty() ? "" : "/") + std::to_string(ks->kseg);
      fits = fits && ks->kseg >= spec.args_bytes && ks->kseg <= kKernargBytes;
      ++ks;
    }
    if (!fits) {
      std::snprintf(out->error, sizeof(out->error), "%s kernarg segment%s %s: code object / host ABI mismatch", kind,
                    specs.size() > 1 ? "s" : "", segs.c_str());
      return finish(), false;
    }
    return true;
  }

  // which agent the reply speaks of, as a probe's reply names it (hsa_probe.cpp fill_identity)
  void identify() {
    uint32_t node = 0;
    if (H().hsa_agent_get_info(ag->agent, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_DRIVER_NODE_ID), &node) ==
        HSA_STATUS_SUCCESS)
      out->kfd_node_id = static_cast<int>(node);
    bus_id(*ag, out->pci_bus_id, sizeof(out->pci_bus_id));
  }

  // One dispatch on the check's queue, waited for. Past the deadline, the
  // dispatch and everything it may still write are abandoned to the in-flight
  // registry and `out` says which stage it was.
  bool run(const KernelInfo& k, void* kargs, uint32_t wgs, uint32_t wg_threads, const char* stage, double* us) {
    dw.submit(k, kargs, wgs, wg_threads);
    if (!wait_signal(dw.sig->s, timeout_s)) {
      std::snprintf(out->error, sizeof(out->error), "%s did not complete within %.1fs", stage, timeout_s);
      out->hsa_error = -1;
      dw.abandon(ordinal, bufs, t0);
      return finish(), false;
    }
    *us = dispatch_us(*ag, dw.sig->s);
    return true;
  }

  // the buffers go before the clock stops; a private queue and executable after it
  int finish() {
    bufs.free();
    out->total_us = std::chrono::duration<double, std::micro>(clk::now() - t0).count();
    return out->ok ? 0 : 1;
  }
  int fail(hsa_status_t s, const char* what) {
    set_hsa_error(&out->hsa_error, out->error, sizeof(out->error), s, what);
    return finish();
  }

  const int ordinal;
  const double timeout_s;
  R* const out;
  const clk::time_point t0 = clk::now();
  const Agent* ag = nullptr;
  DeviceWork dw;
  Buffers bufs;  // after dw: freed before a private queue and executable are destroyed
};

std::atomic<uint64_t> g_perf_poison{~0ull};
// --corrupt-datapath: stage < 0 = off
std::mutex g_dp_corrupt_mu;
int g_dp_corrupt[4] = {-1, 0, 0, -1};  // stage, word, bit, ordinal
int g_dpi8_corrupt[4] = {-1, 0, 0, -1};  // --corrupt-datapath-i8, likewise
int g_dpbf_corrupt[4] = {-1, 0, 0, -1};  // --corrupt-datapath-bf16, likewise
int g_dpf8_corrupt[4] = {-1, 0, 0, -1};  // --corrupt-datapath-fp8, likewise
int g_dphf_corrupt[4] = {-1, 0, 0, -1};  // --corrupt-datapath-f16, likewise

}  // namespace
}  // namespace mi355x::hsa_rt

extern "C" int mi355x_hsa_chip_sweep(int ordinal, uint32_t nonce, int iters, double timeout_s,
                                     mi355x_sweep_result* out) {
  *out = mi355x::blank_result<mi355x_sweep_result>(ordinal, nonce);
  out->iters = iters < 1 ? 1 : (iters > 64 ? 64 : iters);
  Check<mi355x_sweep_result> c(ordinal, timeout_s, out);
  KernelInfo k;
  if (!c.begin(true, &mi355x_sweep_result::grid, 1, "sweep", {{"mi355x_chip_sweep.kd", sizeof(mi355x_sweep_args)}}, &k))
    return 1;
  const uint32_t grid = static_cast<uint32_t>(out->grid);
  const size_t rec_bytes = static_cast<size_t>(grid) * MI355X_SWEEP_REC_WORDS * sizeof(uint32_t);
  const size_t tile_bytes = static_cast<size_t>(grid) * MI355X_PROBE_OUT * sizeof(float);
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* tiles = c.bufs.alloc<float>(g_rt.fine, tile_bytes, "alloc tiles", c.ag, "allow tiles");
  auto* arrive = c.bufs.alloc<uint32_t>(c.ag->coarse, 4096, "alloc arrive");
  auto* kargs = c.bufs.alloc<mi355x_sweep_args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  c.bufs.fill(arrive, 0u, 4096 / 4, "zero arrive");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(tiles, 0xFF, tile_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->tiles = tiles;
  kargs->arrive = arrive;
  kargs->nonce = nonce;
  kargs->iters = out->iters;
  kargs->grid = grid;
  kargs->wait_ticks = 2000000;  // 20 ms at the 100 MHz s_memrealtime clock
  if (!c.run(k, kargs, grid, MI355X_SWEEP_THREADS, "chip sweep", &out->kernel_us)) return 1;
  mi355x::sweep_verdict(records, tiles, grid, out);
  return c.finish();
}

extern "C" void mi355x_hsa_perf_poison(uint64_t unit) { g_perf_poison.store(unit, std::memory_order_relaxed); }

extern "C" int mi355x_hsa_perf_check(int ordinal, uint32_t nonce, uint64_t bytes, int mfma_iters, double timeout_s,
                                     mi355x_perf_result* out) {
  *out = mi355x::blank_result<mi355x_perf_result>(ordinal, nonce);
  out->hbm_first_bad = -1;  // a check that ran: no bad unit seen (a reply that never got here keeps 0)
  // 16-byte units, at least one full grid-stride round, at most 64 GiB
  bytes = bytes < (64ull << 20) ? (64ull << 20) : (bytes > (64ull << 30) ? (64ull << 30) : bytes);
  bytes &= ~static_cast<uint64_t>(0xFFFFF);
  out->bytes = bytes;
  out->mfma_iters = mfma_iters < 1 ? 1 : (mfma_iters > (1 << 22) ? (1 << 22) : mfma_iters);
  Check<mi355x_perf_result> c(ordinal, timeout_s, out);
  KernelInfo ks[3];  // fill, check, burn
  if (!c.begin(true, &mi355x_perf_result::mfma_grid, MI355X_BURN_WGS_PER_CU, "perf",
               {{"mi355x_hbm_fill.kd", sizeof(mi355x_hbm_args)},
                {"mi355x_hbm_check.kd", sizeof(mi355x_hbm_args)},
                {"mi355x_mfma_burn.kd", sizeof(mi355x_burn_args)}},
               ks))
    return 1;
  const uint32_t cus = static_cast<uint32_t>(out->cu_count);
  const uint32_t fill_wgs = cus * MI355X_HBM_FILL_WGS_PER_CU;
  const uint32_t check_wgs = cus * MI355X_HBM_CHECK_WGS_PER_CU;
  const uint32_t burn_wgs = static_cast<uint32_t>(out->mfma_grid);
  const size_t rec_bytes = static_cast<size_t>(burn_wgs) * MI355X_PERF_REC_WORDS * sizeof(uint32_t);
  auto* buf = c.bufs.alloc<uint32_t>(c.ag->coarse, bytes, "alloc HBM buffer");
  // device, [0] bad words, [1] bad words of the second pass, [2..3] first bad unit
  auto* counters = c.bufs.alloc<uint32_t>(c.ag->coarse, 4096, "alloc counters");
  auto* h_counters = c.bufs.alloc<uint32_t>(g_rt.fine, 4096, "alloc host counters", c.ag, "allow counters");
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  // 4 slots of kKernargBytes: fill, check, burn, second check
  auto* kargs = c.bufs.alloc<char>(g_rt.kernarg, 4 * kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  c.bufs.fill(counters, 0u, 2, "zero counters");
  c.bufs.fill(counters + 2, 0xFFFFFFFFu, 2, "init first-bad");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(h_counters, mi355x::kPerfCounterFillByte, 16);   // overwritten by the burn kernel's copy
  std::memset(records, 0, rec_bytes);
  std::memset(kargs, 0, 4 * kKernargBytes);
  auto* fa = reinterpret_cast<mi355x_hbm_args*>(kargs);
  auto* ca = reinterpret_cast<mi355x_hbm_args*>(kargs + kKernargBytes);
  auto* ba = reinterpret_cast<mi355x_burn_args*>(kargs + 2 * kKernargBytes);
  auto* c2 = reinterpret_cast<mi355x_hbm_args*>(kargs + 3 * kKernargBytes);
  fa->buf = ca->buf = buf;
  fa->n16 = ca->n16 = bytes / 16;
  fa->bad = ca->bad = counters;
  fa->first_bad = ca->first_bad = reinterpret_cast<uint64_t*>(counters + 2);
  fa->threads = static_cast<uint64_t>(fill_wgs) * MI355X_PERF_THREADS;
  ca->threads = static_cast<uint64_t>(check_wgs) * MI355X_PERF_THREADS;
  fa->poison_unit = g_perf_poison.load(std::memory_order_relaxed);
  ca->poison_unit = ~0ull;
  fa->seed = ca->seed = nonce * 0x01000193u + 0x7F4A7C15u;
  *c2 = *ca;
  c2->bad = counters + 1;  // the second read pass counts on its own
  ba->records = records;
  ba->hbm_counters = counters;
  ba->hbm_counters_host = h_counters;
  ba->nonce = nonce;
  ba->iters = out->mfma_iters;
  // two read passes: the second one gives steady-state read bandwidth (the
  // first still competes with the fill's write-back) and a second look at every word
  if (!c.run(ks[0], fa, fill_wgs, MI355X_PERF_THREADS, "HBM fill", &out->fill_us) ||
      !c.run(ks[1], ca, check_wgs, MI355X_PERF_THREADS, "HBM check", &out->check_us) ||
      !c.run(ks[1], c2, check_wgs, MI355X_PERF_THREADS, "HBM check (2nd pass)", &out->check2_us) ||
      !c.run(ks[2], ba, burn_wgs, MI355X_PERF_THREADS, "MFMA burn", &out->mfma_us))
    return 1;
  mi355x::perf_verdict(records, h_counters, burn_wgs, out);
  return c.finish();
}

extern "C" void mi355x_hsa_datapath_corrupt(int stage, int word, int bit, int ordinal) {
  std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
  g_dp_corrupt[0] = stage;
  g_dp_corrupt[1] = word;
  g_dp_corrupt[2] = bit;
  g_dp_corrupt[3] = ordinal;
}

extern "C" int mi355x_hsa_datapath_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_result* out) {
  *out = mi355x::blank_result<mi355x_datapath_result>(ordinal, nonce);
  Check<mi355x_datapath_result> c(ordinal, timeout_s, out);
  KernelInfo k;
  // no device memory: records, tiles and kernargs all live in host pools
  if (!c.begin(false, &mi355x_datapath_result::grid, 1, "datapath",
               {{"mi355x_mfma_datapath.kd", sizeof(mi355x_datapath_args)}}, &k))
    return 1;
  const uint32_t grid = static_cast<uint32_t>(out->grid);
  const size_t rec_bytes = static_cast<size_t>(grid) * MI355X_DP_REC_WORDS * sizeof(uint32_t);
  const size_t tile_bytes = static_cast<size_t>(grid) * MI355X_DP_WG_WORDS * sizeof(uint32_t);
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* tiles = c.bufs.alloc<uint32_t>(g_rt.fine, tile_bytes, "alloc tiles", c.ag, "allow tiles");
  auto* kargs = c.bufs.alloc<mi355x_datapath_args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(tiles, 0xFF, tile_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->tiles = tiles;
  kargs->nonce = nonce;
  kargs->grid = grid;
  if (!c.run(k, kargs, grid, MI355X_DP_THREADS, "datapath check", &out->kernel_us)) return 1;
  {
    std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
    const int* cr = g_dp_corrupt;
    if (cr[0] >= 0 && cr[0] < MI355X_DP_STAGES && cr[1] >= 0 && cr[1] < MI355X_DP_TILE && cr[2] >= 0 && cr[2] < 32 &&
        (cr[3] < 0 || cr[3] == ordinal))
      tiles[cr[0] * MI355X_DP_TILE + cr[1]] ^= 1u << cr[2];
  }
  mi355x::datapath_verdict(records, tiles, grid, out);
  return c.finish();
}

extern "C" void mi355x_hsa_datapath_i8_corrupt(int stage, int word, int bit, int ordinal) {
  std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
  g_dpi8_corrupt[0] = stage;
  g_dpi8_corrupt[1] = word;
  g_dpi8_corrupt[2] = bit;
  g_dpi8_corrupt[3] = ordinal;
}

extern "C" int mi355x_hsa_datapath_i8_check(int ordinal, uint32_t nonce, double timeout_s,
                                            mi355x_datapath_i8_result* out) {
  *out = mi355x::blank_result<mi355x_datapath_i8_result>(ordinal, nonce);
  Check<mi355x_datapath_i8_result> c(ordinal, timeout_s, out);
  KernelInfo k;
  // no device memory: records, tiles and kernargs all live in host pools
  if (!c.begin(false, &mi355x_datapath_i8_result::grid, 1, "datapath_i8",
               {{"mi355x_mfma_datapath_i8.kd", sizeof(mi355x_datapath_i8_args)}}, &k))
    return 1;
  const uint32_t grid = static_cast<uint32_t>(out->grid);
  const size_t rec_bytes = static_cast<size_t>(grid) * MI355X_DPI8_REC_WORDS * sizeof(uint32_t);
  const size_t tile_bytes = static_cast<size_t>(grid) * MI355X_DPI8_WG_WORDS * sizeof(uint32_t);
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* tiles = c.bufs.alloc<uint32_t>(g_rt.fine, tile_bytes, "alloc tiles", c.ag, "allow tiles");
  auto* kargs =
      c.bufs.alloc<mi355x_datapath_i8_args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(tiles, 0xFF, tile_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->tiles = tiles;
  kargs->nonce = nonce;
  kargs->grid = grid;
  if (!c.run(k, kargs, grid, MI355X_DPI8_THREADS, "datapath i8 check", &out->kernel_us)) return 1;
  {
    std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
    const int* cr = g_dpi8_corrupt;
    if (cr[0] >= 0 && cr[0] < MI355X_DPI8_STAGES && cr[1] >= 0 &&
        cr[1] < static_cast<int>(dpi8_dim(cr[0]) * dpi8_dim(cr[0])) && cr[2] >= 0 && cr[2] < 32 &&
        (cr[3] < 0 || cr[3] == ordinal))
      tiles[dpi8_tile_offset(cr[0]) + cr[1]] ^= 1u << cr[2];
  }
  mi355x::datapath_i8_verdict(records, tiles, grid, out);
  return c.finish();
}

extern "C" void mi355x_hsa_datapath_bf16_corrupt(int stage, int word, int bit, int ordinal) {
  std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
  g_dpbf_corrupt[0] = stage;
  g_dpbf_corrupt[1] = word;
  g_dpbf_corrupt[2] = bit;
  g_dpbf_corrupt[3] = ordinal;
}

extern "C" int mi355x_hsa_datapath_bf16_check(int ordinal, uint32_t nonce, double timeout_s,
                                            mi355x_datapath_bf16_result* out) {
  *out = mi355x::blank_result<mi355x_datapath_bf16_result>(ordinal, nonce);
  Check<mi355x_datapath_bf16_result> c(ordinal, timeout_s, out);
  KernelInfo k;
  // no device memory: records, tiles and kernargs all live in host pools
  if (!c.begin(false, &mi355x_datapath_bf16_result::grid, 1, "datapath_bf16",
               {{"mi355x_mfma_datapath_bf16.kd", sizeof(mi355x_datapath_bf16_args)}}, &k))
    return 1;
  const uint32_t grid = static_cast<uint32_t>(out->grid);
  const size_t rec_bytes = static_cast<size_t>(grid) * MI355X_DPBF_REC_WORDS * sizeof(uint32_t);
  const size_t tile_bytes = static_cast<size_t>(grid) * MI355X_DPBF_WG_WORDS * sizeof(uint32_t);
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* tiles = c.bufs.alloc<uint32_t>(g_rt.fine, tile_bytes, "alloc tiles", c.ag, "allow tiles");
  auto* kargs =
      c.bufs.alloc<mi355x_datapath_bf16_args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(tiles, 0xFF, tile_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->tiles = tiles;
  kargs->nonce = nonce;
  kargs->grid = grid;
  if (!c.run(k, kargs, grid, MI355X_DPBF_THREADS, "datapath bf16 check", &out->kernel_us)) return 1;
  {
    std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
    const int* cr = g_dpbf_corrupt;
    if (cr[0] >= 0 && cr[0] < MI355X_DPBF_STAGES && cr[1] >= 0 &&
        cr[1] < static_cast<int>(dpbf_dim(cr[0]) * dpbf_dim(cr[0])) && cr[2] >= 0 && cr[2] < 32 &&
        (cr[3] < 0 || cr[3] == ordinal))
      tiles[dpbf_tile_offset(cr[0]) + cr[1]] ^= 1u << cr[2];
  }
  mi355x::datapath_bf16_verdict(records, tiles, grid, out);
  return c.finish();
}

extern "C" void mi355x_hsa_datapath_fp8_corrupt(int stage, int word, int bit, int ordinal) {
  std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
  g_dpf8_corrupt[0] = stage;
  g_dpf8_corrupt[1] = word;
  g_dpf8_corrupt[2] = bit;
  g_dpf8_corrupt[3] = ordinal;
}

extern "C" int mi355x_hsa_datapath_fp8_check(int ordinal, uint32_t nonce, double timeout_s,
                                           mi355x_datapath_fp8_result* out) {
  *out = mi355x::blank_result<mi355x_datapath_fp8_result>(ordinal, nonce);
  Check<mi355x_datapath_fp8_result> c(ordinal, timeout_s, out);
  KernelInfo k;
  // no device memory: records, tiles and kernargs all live in host pools
  if (!c.begin(false, &mi355x_datapath_fp8_result::grid, 1, "datapath_fp8",
               {{"mi355x_mfma_datapath_fp8.kd", sizeof(mi355x_datapath_fp8_args)}}, &k))
    return 1;
  const uint32_t grid = static_cast<uint32_t>(out->grid);
  const size_t rec_bytes = static_cast<size_t>(grid) * MI355X_DPF8_REC_WORDS * sizeof(uint32_t);
  const size_t tile_bytes = static_cast<size_t>(grid) * MI355X_DPF8_WG_WORDS * sizeof(uint32_t);
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* tiles = c.bufs.alloc<uint32_t>(g_rt.fine, tile_bytes, "alloc tiles", c.ag, "allow tiles");
  auto* kargs =
      c.bufs.alloc<mi355x_datapath_fp8_args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(tiles, 0xFF, tile_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->tiles = tiles;
  kargs->nonce = nonce;
  kargs->grid = grid;
  if (!c.run(k, kargs, grid, MI355X_DPF8_THREADS, "datapath fp8 check", &out->kernel_us)) return 1;
  {
    std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
    const int* cr = g_dpf8_corrupt;
    if (cr[0] >= 0 && cr[0] < MI355X_DPF8_STAGES && cr[1] >= 0 &&
        cr[1] < static_cast<int>(dpf8_dim(cr[0]) * dpf8_dim(cr[0])) && cr[2] >= 0 && cr[2] < 32 &&
        (cr[3] < 0 || cr[3] == ordinal))
      tiles[dpf8_tile_offset(cr[0]) + cr[1]] ^= 1u << cr[2];
  }
  mi355x::datapath_fp8_verdict(records, tiles, grid, out);
  return c.finish();
}

extern "C" void mi355x_hsa_datapath_f16_corrupt(int stage, int word, int bit, int ordinal) {
  std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
  g_dphf_corrupt[0] = stage;
  g_dphf_corrupt[1] = word;
  g_dphf_corrupt[2] = bit;
  g_dphf_corrupt[3] = ordinal;
}

extern "C" int mi355x_hsa_datapath_f16_check(int ordinal, uint32_t nonce, double timeout_s,
                                           mi355x_datapath_f16_result* out) {
  *out = mi355x::blank_result<mi355x_datapath_f16_result>(ordinal, nonce);
  Check<mi355x_datapath_f16_result> c(ordinal, timeout_s, out);
  KernelInfo k;
  // no device memory: records, tiles and kernargs all live in host pools
  if (!c.begin(false, &mi355x_datapath_f16_result::grid, 1, "datapath_f16",
               {{"mi355x_mfma_datapath_f16.kd", sizeof(mi355x_datapath_f16_args)}}, &k))
    return 1;
  const uint32_t grid = static_cast<uint32_t>(out->grid);
  const size_t rec_bytes = static_cast<size_t>(grid) * MI355X_DPHF_REC_WORDS * sizeof(uint32_t);
  const size_t tile_bytes = static_cast<size_t>(grid) * MI355X_DPHF_WG_WORDS * sizeof(uint32_t);
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* tiles = c.bufs.alloc<uint32_t>(g_rt.fine, tile_bytes, "alloc tiles", c.ag, "allow tiles");
  auto* kargs =
      c.bufs.alloc<mi355x_datapath_f16_args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(tiles, 0xFF, tile_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->tiles = tiles;
  kargs->nonce = nonce;
  kargs->grid = grid;
  if (!c.run(k, kargs, grid, MI355X_DPHF_THREADS, "datapath f16 check", &out->kernel_us)) return 1;
  {
    std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
    const int* cr = g_dphf_corrupt;
    if (cr[0] >= 0 && cr[0] < MI355X_DPHF_STAGES && cr[1] >= 0 &&
        cr[1] < static_cast<int>(dphf_dim(cr[0]) * dphf_dim(cr[0])) && cr[2] >= 0 && cr[2] < 32 &&
        (cr[3] < 0 || cr[3] == ordinal))
      tiles[dphf_tile_offset(cr[0]) + cr[1]] ^= 1u << cr[2];
  }
  mi355x::datapath_f16_verdict(records, tiles, grid, out);
  return c.finish();
}
