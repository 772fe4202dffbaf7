// The full-chip sweep (mi355x_hsa_chip_sweep: every CU of every XCD runs the
// MFMA tile and reports where it ran), the throughput check
// (mi355x_hsa_perf_check: HBM write / read over a verified pattern, sustained
// bf16 MFMA rate, per-XCD clocks) and the MFMA datapath check
// (mi355x_hsa_datapath_check: full-width operands, bit-exact) and its int8
// and bf16 siblings (mi355x_hsa_datapath_i8_check, mi355x_hsa_datapath_bf16_check:
// 128-bit operands; mi355x_hsa_datapath_fp8_check: fp8 and MX-scaled operands;
// mi355x_hsa_datapath_f16_check: f16 operands, the legacy 64-bit forms too;
// mi355x_hsa_datapath_f64_check: f64 operands and accumulators;
// mi355x_hsa_datapath_f6f4_check: fp6 / fp4 MX-scaled operands;
// mi355x_hsa_datapath_sparse_check: the 2:4 sparse forms, v_smfmac_*;
// mi355x_hsa_datapath_gemm_check: a bf16 GEMM out of HBM through LDS;
// mi355x_hsa_datapath_splitk_check: split-K partials summed by L2 atomics;
// mi355x_hsa_datapath_attn_check: a flash-attention loop, MFMA to softmax to MFMA;
// mi355x_hsa_datapath_mxgemm_check: an MXFP4 GEMM, scaled-MFMA chains out of HBM;
// mi355x_hsa_datapath_mxquant_check: MFMA, on-device MX quantisation, scaled MFMA), all on the
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
#include "datapath_f64_verify.h"
#include "datapath_f6f4_verify.h"
#include "datapath_fp8_verify.h"
#include "datapath_i8_verify.h"
#include "datapath_gemm_verify.h"
#include "datapath_sparse_verify.h"
#include "datapath_splitk_verify.h"
#include "datapath_attn_verify.h"
#include "datapath_mxgemm_verify.h"
#include "datapath_mxquant_verify.h"
#include "datapath_verify.h"
#include "hsa_runtime.h"
#include "probe_json.h"
#include "probe_kinds.h"
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
// --corrupt-datapath*: per kind (a row of probe_kinds.h) stage, word, bit, ordinal; stage < 0 = off
std::mutex g_dp_corrupt_mu;
struct DpCorrupt {
  int v[4] = {-1, 0, 0, -1};
};
DpCorrupt g_dp_corrupt[mi355x::kProbeKindCount];

// the kind's injection; g_dp_corrupt_mu held
int* dp_corrupt(const char* kind) { return g_dp_corrupt[mi355x::probe_kind_index(kind)].v; }

void set_dp_corrupt(const char* kind, int stage, int word, int bit, int ordinal) {
  std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
  int* c = dp_corrupt(kind);
  c[0] = stage;
  c[1] = word;
  c[2] = bit;
  c[3] = ordinal;
}

// A register-only datapath check, described by its traits
// (datapath_verdict_common.h): one kernel, one workgroup per CU, each writing a
// record and wave 0's tiles into host memory, then the shared verdict.
template <typename T>
int register_datapath_check(int ordinal, uint32_t nonce, double timeout_s, typename T::Result* out) {
  using R = typename T::Result;
  using Args = typename T::Args;
  *out = mi355x::blank_result<R>(ordinal, nonce);
  Check<R> c(ordinal, timeout_s, out);
  KernelInfo k;
  // no device memory: records, tiles and kernargs all live in host pools
  if (!c.begin(false, &R::grid, 1, T::kKind, {{T::kSymbol, sizeof(Args)}}, &k)) return 1;
  const uint32_t grid = static_cast<uint32_t>(out->grid);
  const size_t rec_bytes = static_cast<size_t>(grid) * T::kRecWords * sizeof(uint32_t);
  const size_t tile_bytes = static_cast<size_t>(grid) * T::kWgWords * sizeof(uint32_t);
  auto* records = c.bufs.template alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* tiles = c.bufs.template alloc<uint32_t>(g_rt.fine, tile_bytes, "alloc tiles", c.ag, "allow tiles");
  auto* kargs = c.bufs.template alloc<Args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(tiles, 0xFF, tile_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->tiles = tiles;
  kargs->nonce = nonce;
  kargs->grid = grid;
  if (!c.run(k, kargs, grid, T::kThreads, T::kDispatch, &out->kernel_us)) return 1;
  {
    // workgroup 0's tiles: the word is numbered within its stage
    std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
    const int* cr = dp_corrupt(T::kKind);
    if (cr[0] >= 0 && cr[0] < static_cast<int>(T::kStages) && cr[1] >= 0 &&
        cr[1] < static_cast<int>(T::tiles(cr[0]) * T::tile_words(cr[0])) && cr[2] >= 0 && cr[2] < 32 &&
        (cr[3] < 0 || cr[3] == ordinal))
      tiles[T::tile_offset(cr[0]) + cr[1]] ^= 1u << cr[2];
  }
  mi355x::datapath_register_verdict<T>(records, tiles, grid, out);
  return c.finish();
}

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

// the eight register-only datapath checks and the eleven kinds' fault injection (liveness_probe.h)
extern "C" int mi355x_hsa_datapath_check(int ordinal, uint32_t nonce, double timeout_s, mi355x_datapath_result* out) {
  return register_datapath_check<mi355x::DatapathF32Traits>(ordinal, nonce, timeout_s, out);
}
extern "C" int mi355x_hsa_datapath_i8_check(int ordinal, uint32_t nonce, double timeout_s,
                                            mi355x_datapath_i8_result* out) {
  return register_datapath_check<mi355x::DatapathI8Traits>(ordinal, nonce, timeout_s, out);
}
extern "C" int mi355x_hsa_datapath_bf16_check(int ordinal, uint32_t nonce, double timeout_s,
                                              mi355x_datapath_bf16_result* out) {
  return register_datapath_check<mi355x::DatapathBf16Traits>(ordinal, nonce, timeout_s, out);
}
extern "C" int mi355x_hsa_datapath_fp8_check(int ordinal, uint32_t nonce, double timeout_s,
                                             mi355x_datapath_fp8_result* out) {
  return register_datapath_check<mi355x::DatapathFp8Traits>(ordinal, nonce, timeout_s, out);
}
extern "C" int mi355x_hsa_datapath_f16_check(int ordinal, uint32_t nonce, double timeout_s,
                                             mi355x_datapath_f16_result* out) {
  return register_datapath_check<mi355x::DatapathF16Traits>(ordinal, nonce, timeout_s, out);
}
extern "C" int mi355x_hsa_datapath_f64_check(int ordinal, uint32_t nonce, double timeout_s,
                                             mi355x_datapath_f64_result* out) {
  return register_datapath_check<mi355x::DatapathF64Traits>(ordinal, nonce, timeout_s, out);
}
extern "C" int mi355x_hsa_datapath_f6f4_check(int ordinal, uint32_t nonce, double timeout_s,
                                              mi355x_datapath_f6f4_result* out) {
  return register_datapath_check<mi355x::DatapathF6f4Traits>(ordinal, nonce, timeout_s, out);
}
extern "C" int mi355x_hsa_datapath_sparse_check(int ordinal, uint32_t nonce, double timeout_s,
                                                mi355x_datapath_sparse_result* out) {
  return register_datapath_check<mi355x::DatapathSparseTraits>(ordinal, nonce, timeout_s, out);
}
extern "C" void mi355x_hsa_datapath_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath", stage, word, bit, ordinal);
}
extern "C" void mi355x_hsa_datapath_i8_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_i8", stage, word, bit, ordinal);
}
extern "C" void mi355x_hsa_datapath_bf16_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_bf16", stage, word, bit, ordinal);
}
extern "C" void mi355x_hsa_datapath_fp8_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_fp8", stage, word, bit, ordinal);
}
extern "C" void mi355x_hsa_datapath_f16_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_f16", stage, word, bit, ordinal);
}
extern "C" void mi355x_hsa_datapath_f64_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_f64", stage, word, bit, ordinal);
}
extern "C" void mi355x_hsa_datapath_f6f4_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_f6f4", stage, word, bit, ordinal);
}
extern "C" void mi355x_hsa_datapath_sparse_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_sparse", stage, word, bit, ordinal);
}
extern "C" void mi355x_hsa_datapath_gemm_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_gemm", stage, word, bit, ordinal);
}
extern "C" void mi355x_hsa_datapath_splitk_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_splitk", stage, word, bit, ordinal);
}
extern "C" void mi355x_hsa_datapath_attn_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_attn", stage, word, bit, ordinal);
}

extern "C" int mi355x_hsa_datapath_gemm_check(int ordinal, uint32_t nonce, double timeout_s,
                                              mi355x_datapath_gemm_result* out) {
  *out = mi355x::blank_result<mi355x_datapath_gemm_result>(ordinal, nonce);
  out->ksteps = MI355X_DPGM_KSTEPS;
  Check<mi355x_datapath_gemm_result> c(ordinal, timeout_s, out);
  KernelInfo ks[2];  // fill, gemm
  // the operands live in device memory; records, D tiles and kernargs in host pools
  if (!c.begin(true, &mi355x_datapath_gemm_result::grid, 1, "datapath_gemm",
               {{"mi355x_gemm_fill.kd", sizeof(mi355x_datapath_gemm_args)},
                {"mi355x_mfma_datapath_gemm.kd", sizeof(mi355x_datapath_gemm_args)}},
               ks))
    return 1;
  const uint32_t grid = static_cast<uint32_t>(out->grid);
  const size_t K = static_cast<size_t>(MI355X_DPGM_KSTEPS) * MI355X_DPGM_KSTEP;
  const size_t rec_bytes = static_cast<size_t>(grid) * MI355X_DPGM_REC_WORDS * sizeof(uint32_t);
  const size_t tile_bytes = static_cast<size_t>(grid) * MI355X_DPGM_WG_WORDS * sizeof(uint32_t);
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* tiles = c.bufs.alloc<uint32_t>(g_rt.fine, tile_bytes, "alloc tiles", c.ag, "allow tiles");
  // written by mi355x_gemm_fill, whole, before the GEMM reads them: no runtime fill or copy (ROCr would open a queue)
  auto* a = c.bufs.alloc<uint16_t>(c.ag->coarse, grid * MI355X_DPGM_TILE * K * sizeof(uint16_t), "alloc A");
  auto* b = c.bufs.alloc<uint16_t>(c.ag->coarse, K * MI355X_DPGM_TILE * sizeof(uint16_t), "alloc B");
  auto* kargs =
      c.bufs.alloc<mi355x_datapath_gemm_args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(tiles, 0xFF, tile_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->tiles = tiles;
  kargs->a = a;
  kargs->b = b;
  kargs->nonce = nonce;
  kargs->grid = grid;
  kargs->ksteps = MI355X_DPGM_KSTEPS;
  if (!c.run(ks[0], kargs, grid, MI355X_DPGM_THREADS, "datapath gemm fill", &out->fill_us) ||
      !c.run(ks[1], kargs, grid, MI355X_DPGM_THREADS, "datapath gemm check", &out->kernel_us))
    return 1;
  {
    std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
    const int* cr = dp_corrupt("datapath_gemm");
    const int words = cr[0] == 2 ? MI355X_DPGM_WG_WORDS : 8;
    if (cr[0] >= 0 && cr[0] < MI355X_DPGM_STAGES && cr[1] >= 0 && cr[1] < words && cr[2] >= 0 && cr[2] < 32 &&
        (cr[3] < 0 || cr[3] == ordinal))
      (cr[0] == 2 ? tiles[cr[1]] : records[dpgm_fold_slot(cr[0], cr[1])]) ^= 1u << cr[2];
  }
  const auto t_verify = std::chrono::steady_clock::now();
  mi355x::datapath_gemm_verdict(records, tiles, grid, MI355X_DPGM_KSTEPS, out);
  out->verify_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_verify).count();
  return c.finish();
}

extern "C" int mi355x_hsa_datapath_splitk_check(int ordinal, uint32_t nonce, double timeout_s,
                                                mi355x_datapath_splitk_result* out) {
  *out = mi355x::blank_result<mi355x_datapath_splitk_result>(ordinal, nonce);
  out->splits = MI355X_DPSK_SPLITS;
  out->ksteps = MI355X_DPSK_KSTEPS;
  Check<mi355x_datapath_splitk_result> c(ordinal, timeout_s, out);
  KernelInfo ks[3];  // fill, split-K GEMM, drain
  // the operands, D and the ledgers live in device memory; records, the drained copies and kernargs in host pools
  if (!c.begin(true, &mi355x_datapath_splitk_result::grid, 1, "datapath_splitk",
               {{"mi355x_splitk_fill.kd", sizeof(mi355x_datapath_splitk_args)},
                {"mi355x_mfma_datapath_splitk.kd", sizeof(mi355x_datapath_splitk_args)},
                {"mi355x_splitk_drain.kd", sizeof(mi355x_datapath_splitk_args)}},
               ks))
    return 1;
  // a tile per 8 CUs, so that its 8 contributors are in flight together with everyone else's
  const uint32_t tiles = std::max(1u, static_cast<uint32_t>(out->cu_count) / MI355X_DPSK_CUS_PER_TILE);
  const uint32_t grid = tiles * MI355X_DPSK_SPLITS;
  out->tiles = static_cast<int>(tiles);
  out->grid = static_cast<int>(grid);
  const size_t K = static_cast<size_t>(MI355X_DPSK_SPLITS) * MI355X_DPSK_KSTEPS * MI355X_DPGM_KSTEP;
  const size_t rec_bytes = static_cast<size_t>(grid) * MI355X_DPSK_REC_WORDS * sizeof(uint32_t);
  const size_t d_bytes = static_cast<size_t>(tiles) * MI355X_DPSK_TILE_WORDS * sizeof(uint32_t);
  const size_t led_bytes = static_cast<size_t>(tiles) * MI355X_DPSK_LEDGER_WORDS * sizeof(uint32_t);
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* out_d = c.bufs.alloc<uint32_t>(g_rt.fine, d_bytes, "alloc tiles", c.ag, "allow tiles");
  auto* out_led = c.bufs.alloc<uint32_t>(g_rt.fine, led_bytes, "alloc ledgers", c.ag, "allow ledgers");
  // written by mi355x_splitk_fill, whole, before the GEMM touches them, and read back by mi355x_splitk_drain: no
  // runtime fill or copy (ROCr would open a queue)
  auto* a = c.bufs.alloc<uint16_t>(c.ag->coarse, tiles * MI355X_DPGM_TILE * K * sizeof(uint16_t), "alloc A");
  auto* b = c.bufs.alloc<uint16_t>(c.ag->coarse, K * MI355X_DPGM_TILE * sizeof(uint16_t), "alloc B");
  auto* d = c.bufs.alloc<float>(c.ag->coarse, d_bytes, "alloc D");
  auto* ledger = c.bufs.alloc<uint32_t>(c.ag->coarse, led_bytes, "alloc ledger");
  auto* kargs =
      c.bufs.alloc<mi355x_datapath_splitk_args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(out_d, 0xFF, d_bytes);
  std::memset(out_led, 0xFF, led_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->out_d = out_d;
  kargs->out_ledger = out_led;
  kargs->a = a;
  kargs->b = b;
  kargs->d = d;
  kargs->ledger = ledger;
  kargs->nonce = nonce;
  kargs->tiles = tiles;
  kargs->splits = MI355X_DPSK_SPLITS;
  kargs->ksteps = MI355X_DPSK_KSTEPS;
  if (!c.run(ks[0], kargs, grid, MI355X_DPSK_THREADS, "datapath splitk fill", &out->fill_us) ||
      !c.run(ks[1], kargs, grid, MI355X_DPSK_THREADS, "datapath splitk check", &out->kernel_us) ||
      !c.run(ks[2], kargs, tiles, MI355X_DPSK_THREADS, "datapath splitk drain", &out->drain_us))
    return 1;
  {
    std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
    const int* cr = dp_corrupt("datapath_splitk");
    const int words = static_cast<int>(cr[0] == 2 ? tiles * MI355X_DPSK_TILE_WORDS
                                       : cr[0] == 3 ? tiles * MI355X_DPSK_LEDGER_WORDS : grid * 8);
    if (cr[0] >= 0 && cr[0] < MI355X_DPSK_STAGES && cr[1] >= 0 && cr[1] < words && cr[2] >= 0 && cr[2] < 32 &&
        (cr[3] < 0 || cr[3] == ordinal))
      (cr[0] == 2   ? out_d[cr[1]]
       : cr[0] == 3 ? out_led[cr[1]]
                    : records[(cr[1] / 8) * MI355X_DPSK_REC_WORDS + dpsk_fold_slot(cr[0], cr[1] % 8)]) ^= 1u << cr[2];
  }
  const auto t_verify = std::chrono::steady_clock::now();
  mi355x::datapath_splitk_verdict(records, out_d, out_led, tiles, MI355X_DPSK_SPLITS, MI355X_DPSK_KSTEPS, out);
  out->verify_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_verify).count();
  return c.finish();
}

extern "C" int mi355x_hsa_datapath_attn_check(int ordinal, uint32_t nonce, double timeout_s,
                                              mi355x_datapath_attn_result* out) {
  *out = mi355x::blank_result<mi355x_datapath_attn_result>(ordinal, nonce);
  out->qblocks = MI355X_DPAT_QBLOCKS;
  out->kblocks = MI355X_DPAT_KBLOCKS;
  Check<mi355x_datapath_attn_result> c(ordinal, timeout_s, out);
  KernelInfo ks[2];  // fill, attention
  // the operands live in device memory; records, m / l, O and kernargs in host pools
  if (!c.begin(true, &mi355x_datapath_attn_result::grid, 1, "datapath_attn",
               {{"mi355x_attn_fill.kd", sizeof(mi355x_datapath_attn_args)},
                {"mi355x_mfma_datapath_attn.kd", sizeof(mi355x_datapath_attn_args)}},
               ks))
    return 1;
  // a head per 4 CUs: its 4 workgroups, one a CU, read the same K and V through L2
  const uint32_t heads = std::max(1u, static_cast<uint32_t>(out->cu_count) / MI355X_DPAT_CUS_PER_HEAD);
  const uint32_t grid = heads * MI355X_DPAT_QBLOCKS;
  out->heads = static_cast<int>(heads);
  out->grid = static_cast<int>(grid);
  const size_t rec_bytes = static_cast<size_t>(grid) * MI355X_DPAT_REC_WORDS * sizeof(uint32_t);
  const size_t ml_bytes = static_cast<size_t>(grid) * MI355X_DPAT_ML_WORDS * sizeof(uint32_t);
  const size_t o_bytes = static_cast<size_t>(grid) * MI355X_DPAT_O_WORDS * sizeof(uint32_t);
  const size_t q_bytes = static_cast<size_t>(grid) * MI355X_DPAT_QBLOCK * MI355X_DPAT_D * sizeof(uint16_t);
  const size_t kv_bytes =
      static_cast<size_t>(heads) * MI355X_DPAT_KBLOCKS * MI355X_DPAT_KBLOCK * MI355X_DPAT_D * sizeof(uint16_t);
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* ml = c.bufs.alloc<uint32_t>(g_rt.fine, ml_bytes, "alloc m / l", c.ag, "allow m / l");
  auto* o = c.bufs.alloc<uint32_t>(g_rt.fine, o_bytes, "alloc O", c.ag, "allow O");
  // written by mi355x_attn_fill, whole, before the attention kernel reads them: no runtime fill (ROCr would open a queue)
  auto* q = c.bufs.alloc<uint16_t>(c.ag->coarse, q_bytes, "alloc Q");
  auto* k = c.bufs.alloc<uint16_t>(c.ag->coarse, kv_bytes, "alloc K");
  auto* v = c.bufs.alloc<uint16_t>(c.ag->coarse, kv_bytes, "alloc V");
  auto* kargs =
      c.bufs.alloc<mi355x_datapath_attn_args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(ml, 0xFF, ml_bytes);
  std::memset(o, 0xFF, o_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->ml = ml;
  kargs->o = o;
  kargs->q = q;
  kargs->k = k;
  kargs->v = v;
  kargs->nonce = nonce;
  kargs->heads = heads;
  kargs->qblocks = MI355X_DPAT_QBLOCKS;
  kargs->kblocks = MI355X_DPAT_KBLOCKS;
  if (!c.run(ks[0], kargs, grid, MI355X_DPAT_THREADS, "datapath attn fill", &out->fill_us) ||
      !c.run(ks[1], kargs, grid, MI355X_DPAT_THREADS, "datapath attn check", &out->kernel_us))
    return 1;
  {
    std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
    const int* cr = dp_corrupt("datapath_attn");
    const int words = static_cast<int>(cr[0] == 2 ? grid * MI355X_DPAT_ML_WORDS
                                       : cr[0] == 3 ? grid * MI355X_DPAT_O_WORDS : grid * 8);
    if (cr[0] >= 0 && cr[0] < MI355X_DPAT_STAGES && cr[1] >= 0 && cr[1] < words && cr[2] >= 0 && cr[2] < 32 &&
        (cr[3] < 0 || cr[3] == ordinal))
      (cr[0] == 2   ? ml[cr[1]]
       : cr[0] == 3 ? o[cr[1]]
                    : records[(cr[1] / 8) * MI355X_DPAT_REC_WORDS + dpat_fold_slot(cr[0], cr[1] % 8)]) ^= 1u << cr[2];
  }
  const auto t_verify = std::chrono::steady_clock::now();
  mi355x::datapath_attn_verdict(records, ml, o, heads, MI355X_DPAT_QBLOCKS, MI355X_DPAT_KBLOCKS, out);
  out->verify_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_verify).count();
  return c.finish();
}

extern "C" void mi355x_hsa_datapath_mxgemm_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_mxgemm", stage, word, bit, ordinal);
}

extern "C" int mi355x_hsa_datapath_mxgemm_check(int ordinal, uint32_t nonce, double timeout_s,
                                                mi355x_datapath_mxgemm_result* out) {
  *out = mi355x::blank_result<mi355x_datapath_mxgemm_result>(ordinal, nonce);
  out->ksteps = MI355X_DPMX_KSTEPS;
  Check<mi355x_datapath_mxgemm_result> c(ordinal, timeout_s, out);
  KernelInfo ks[2];  // fill, gemm
  // the operands and scales live in device memory; records, D tiles and kernargs in host pools
  if (!c.begin(true, &mi355x_datapath_mxgemm_result::grid, 1, "datapath_mxgemm",
               {{"mi355x_mxgemm_fill.kd", sizeof(mi355x_datapath_mxgemm_args)},
                {"mi355x_mfma_datapath_mxgemm.kd", sizeof(mi355x_datapath_mxgemm_args)}},
               ks))
    return 1;
  const uint32_t grid = static_cast<uint32_t>(out->grid);
  if (!dpmx_sizes_ok(grid, MI355X_DPMX_KSTEPS)) {
    std::snprintf(out->error, sizeof(out->error), "datapath mxgemm check: %u workgroups", grid);
    return c.finish();
  }
  const size_t K = static_cast<size_t>(MI355X_DPMX_KSTEPS) * MI355X_DPMX_KSTEP;
  const size_t rec_bytes = static_cast<size_t>(grid) * MI355X_DPMX_REC_WORDS * sizeof(uint32_t);
  const size_t tile_bytes = static_cast<size_t>(grid) * MI355X_DPMX_WG_WORDS * sizeof(uint32_t);
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* tiles = c.bufs.alloc<uint32_t>(g_rt.fine, tile_bytes, "alloc tiles", c.ag, "allow tiles");
  // written by mi355x_mxgemm_fill, whole, before the GEMM reads them: no runtime fill or copy (ROCr would open a queue)
  auto* a = c.bufs.alloc<uint8_t>(c.ag->coarse, grid * MI355X_DPMX_TILE * K / 2, "alloc A");
  auto* b = c.bufs.alloc<uint8_t>(c.ag->coarse, MI355X_DPMX_TILE * K / 2, "alloc B");
  auto* sa = c.bufs.alloc<uint8_t>(c.ag->coarse, grid * MI355X_DPMX_TILE * K / 32, "alloc A scales");
  auto* sb = c.bufs.alloc<uint8_t>(c.ag->coarse, MI355X_DPMX_TILE * K / 32, "alloc B scales");
  auto* kargs =
      c.bufs.alloc<mi355x_datapath_mxgemm_args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(tiles, 0xFF, tile_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->tiles = tiles;
  kargs->a = a;
  kargs->b = b;
  kargs->sa = sa;
  kargs->sb = sb;
  kargs->nonce = nonce;
  kargs->grid = grid;
  kargs->ksteps = MI355X_DPMX_KSTEPS;
  if (!c.run(ks[0], kargs, grid, MI355X_DPMX_THREADS, "datapath mxgemm fill", &out->fill_us) ||
      !c.run(ks[1], kargs, grid, MI355X_DPMX_THREADS, "datapath mxgemm check", &out->kernel_us))
    return 1;
  {
    std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
    const int* cr = dp_corrupt("datapath_mxgemm");
    const int words = static_cast<int>(cr[0] == 3 ? grid * MI355X_DPMX_WG_WORDS : grid * 16);
    if (cr[0] >= 0 && cr[0] < MI355X_DPMX_STAGES && cr[1] >= 0 && cr[1] < words && (cr[0] == 3 || cr[1] % 16 < 8) &&
        cr[2] >= 0 && cr[2] < 32 && (cr[3] < 0 || cr[3] == ordinal))
      (cr[0] == 3 ? tiles[cr[1]]
                  : records[(cr[1] / 16) * MI355X_DPMX_REC_WORDS + dpmx_fold_slot(cr[0], cr[1] % 16)]) ^= 1u << cr[2];
  }
  const auto t_verify = std::chrono::steady_clock::now();
  mi355x::datapath_mxgemm_verdict(records, tiles, grid, MI355X_DPMX_KSTEPS, out);
  out->verify_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_verify).count();
  return c.finish();
}

extern "C" void mi355x_hsa_datapath_mxquant_corrupt(int stage, int word, int bit, int ordinal) {
  set_dp_corrupt("datapath_mxquant", stage, word, bit, ordinal);
}

extern "C" int mi355x_hsa_datapath_mxquant_check(int ordinal, uint32_t nonce, double timeout_s,
                                                 mi355x_datapath_mxquant_result* out) {
  *out = mi355x::blank_result<mi355x_datapath_mxquant_result>(ordinal, nonce);
  out->hsteps = MI355X_DPMQ_HSTEPS;
  Check<mi355x_datapath_mxquant_result> c(ordinal, timeout_s, out);
  KernelInfo ks[2];  // fill, the MLP tile
  // the operands live in device memory; records, the quantised images, Y tiles and kernargs in host pools
  if (!c.begin(true, &mi355x_datapath_mxquant_result::grid, 1, "datapath_mxquant",
               {{"mi355x_mxquant_fill.kd", sizeof(mi355x_datapath_mxquant_args)},
                {"mi355x_mfma_datapath_mxquant.kd", sizeof(mi355x_datapath_mxquant_args)}},
               ks))
    return 1;
  const uint32_t grid = static_cast<uint32_t>(out->grid);
  if (!dpmq_sizes_ok(grid, MI355X_DPMQ_HSTEPS)) {
    std::snprintf(out->error, sizeof(out->error), "datapath mxquant check: %u workgroups", grid);
    return c.finish();
  }
  const size_t hidden = static_cast<size_t>(MI355X_DPMQ_HSTEPS) * MI355X_DPMQ_TILE;
  const uint32_t img_words = MI355X_DPMQ_IMG_WORDS(MI355X_DPMQ_HSTEPS);
  const size_t rec_bytes = static_cast<size_t>(grid) * MI355X_DPMQ_REC_WORDS * sizeof(uint32_t);
  const size_t img_bytes = static_cast<size_t>(grid) * img_words * sizeof(uint32_t);
  const size_t tile_bytes = static_cast<size_t>(grid) * MI355X_DPMQ_WG_WORDS * sizeof(uint32_t);
  auto* records = c.bufs.alloc<uint32_t>(g_rt.fine, rec_bytes, "alloc records", c.ag, "allow records");
  auto* image = c.bufs.alloc<uint32_t>(g_rt.fine, img_bytes, "alloc image", c.ag, "allow image");
  auto* tiles = c.bufs.alloc<uint32_t>(g_rt.fine, tile_bytes, "alloc tiles", c.ag, "allow tiles");
  // written by mi355x_mxquant_fill, whole, before the MLP tile reads them: no runtime fill or copy (ROCr would open a queue)
  auto* x = c.bufs.alloc<uint16_t>(c.ag->coarse, static_cast<size_t>(grid) * MI355X_DPMQ_TILE * MI355X_DPMQ_TILE * 2, "alloc X");
  auto* w1 = c.bufs.alloc<uint16_t>(c.ag->coarse, hidden * MI355X_DPMQ_TILE * 2, "alloc W1");
  auto* w2 = c.bufs.alloc<uint8_t>(c.ag->coarse, MI355X_DPMQ_TILE * hidden / 2, "alloc W2");
  auto* sb = c.bufs.alloc<uint8_t>(c.ag->coarse, MI355X_DPMQ_TILE * hidden / 32, "alloc W2 scales");
  auto* kargs =
      c.bufs.alloc<mi355x_datapath_mxquant_args>(g_rt.kernarg, kKernargBytes, "alloc kernarg", c.ag, "allow kernarg");
  if (!c.bufs.ok()) return c.fail(c.bufs.status, c.bufs.what);
  std::memset(records, 0, rec_bytes);
  std::memset(image, 0xFF, img_bytes);
  std::memset(tiles, 0xFF, tile_bytes);
  std::memset(kargs, 0, kKernargBytes);
  kargs->records = records;
  kargs->tiles = tiles;
  kargs->image = image;
  kargs->x = x;
  kargs->w1 = w1;
  kargs->w2 = w2;
  kargs->sb = sb;
  kargs->nonce = nonce;
  kargs->grid = grid;
  kargs->hsteps = MI355X_DPMQ_HSTEPS;
  if (!c.run(ks[0], kargs, grid, MI355X_DPMQ_THREADS, "datapath mxquant fill", &out->fill_us) ||
      !c.run(ks[1], kargs, grid, MI355X_DPMQ_THREADS, "datapath mxquant check", &out->kernel_us))
    return 1;
  {
    std::lock_guard<std::mutex> lk(g_dp_corrupt_mu);
    const int* cr = dp_corrupt("datapath_mxquant");
    const uint32_t per_wg = cr[0] == 3 ? MI355X_DPMQ_WG_WORDS : cr[0] == 2 ? img_words : 16u;
    if (cr[0] >= 0 && cr[0] < MI355X_DPMQ_STAGES && cr[1] >= 0 && static_cast<uint32_t>(cr[1]) < grid * per_wg &&
        (cr[0] != 0 || cr[1] % 16 < 8) && cr[2] >= 0 && cr[2] < 32 && (cr[3] < 0 || cr[3] == ordinal))
      (cr[0] == 3   ? tiles[cr[1]]
       : cr[0] == 2 ? image[cr[1]]
                    : records[(cr[1] / 16) * MI355X_DPMQ_REC_WORDS + dpmq_fold_slot(cr[0], cr[1] % 16)]) ^= 1u << cr[2];
  }
  const auto t_verify = std::chrono::steady_clock::now();
  mi355x::datapath_mxquant_verdict(records, image, tiles, grid, MI355X_DPMQ_HSTEPS, out);
  out->verify_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_verify).count();
  return c.finish();
}
