// The JSON the probe prints: a device's object for the liveness probe, a chip
// sweep, a throughput check and the four datapath checks, the server's hello,
// and the lines around the devices, --serve and one-shot (shared by
// probe_main.cpp and the contract CLIs under native/tests, so a test sees
// exactly the line the prober parses), and the blank result each check starts
// from. Strings grow as needed: a long
// escaped `error` next to wide numbers is never cut.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>

#include "mi355x/liveness_probe.h"

namespace mi355x {

inline std::string json_escape(const char* s) {
  std::string o;
  for (; *s; ++s) {
    char c = *s;
    if (c == '"' || c == '\\') {
      o += '\\';
      o += c;
    } else if (static_cast<unsigned char>(c) < 0x20) {
      char b[8];
      std::snprintf(b, sizeof(b), "\\u%04x", c);
      o += b;
    } else {
      o += c;
    }
  }
  return o;
}

// printf into a string of whatever length the output needs
__attribute__((format(printf, 1, 2))) inline std::string json_format(const char* fmt, ...) {
  va_list ap, ap2;
  va_start(ap, fmt);
  va_copy(ap2, ap);
  const int n = std::vsnprintf(nullptr, 0, fmt, ap);
  va_end(ap);
  std::string o(n > 0 ? static_cast<size_t>(n) : 0, '\0');
  if (n > 0) std::vsnprintf(&o[0], o.size() + 1, fmt, ap2);
  va_end(ap2);
  return o;
}

// The result of a check on `ordinal` before anything is known: all zero but
// what the type defines otherwise -- the datapath results' first_bad_* = -1
// ("none"), the four checks' kfd_node_id = -1 (with pci_bus_id "": the reply
// never reached a device). hbm_first_bad of the throughput result stays 0 here: a reply that
// never reached the runtime carries 0, mi355x_hsa_perf_check sets its own -1.
template <typename R>
R blank_result(int ordinal, uint32_t nonce) {
  R r{};
  r.ordinal = ordinal;
  r.nonce = nonce;
  if constexpr (std::is_same_v<R, mi355x_datapath_result> || std::is_same_v<R, mi355x_datapath_i8_result> ||
                std::is_same_v<R, mi355x_datapath_fp8_result> || std::is_same_v<R, mi355x_datapath_f16_result>)
    r.first_bad_wg = r.first_bad_stage = r.first_bad_word = -1;
  if constexpr (!std::is_same_v<R, mi355x_probe_result>) r.kfd_node_id = -1;  // a check that names no agent
  return r;
}

inline std::string sweep_json(const mi355x_sweep_result& r) {
  std::string per = "[";
  for (int i = 0; i < 16 && i < (r.num_xcc > 0 ? r.num_xcc : 8); ++i) {
    if (i) per += ",";
    per += std::to_string(r.wgs_per_xcc[i]);
  }
  per += "]";
  return json_format(
      "{\"ordinal\":%d,\"ok\":%s,\"hsa_error\":%d,\"nonce\":%u,\"iters\":%d,\"grid\":%d,"
      "\"cu_count\":%d,\"num_xcc\":%d,\"records_ok\":%d,\"mfma_bad\":%u,\"lds_bad\":%u,"
      "\"tile_bad\":%u,\"cus_covered\":%d,\"xccs_covered\":%d,\"all_resident\":%s,"
      "\"wgs_per_xcc\":%s,\"kernel_us\":%.2f,\"arrival_spread_us\":%.2f,\"total_us\":%.1f,"
      "\"in_flight_s\":%.2f,\"kept_queue\":%s,\"kfd_node_id\":%d,\"pci_bus_id\":\"%s\",\"error\":\"%s\"}",
      r.ordinal, r.ok ? "true" : "false", r.hsa_error, r.nonce, r.iters, r.grid, r.cu_count, r.num_xcc, r.records_ok,
      r.mfma_bad, r.lds_bad, r.tile_bad, r.cus_covered, r.xccs_covered, r.all_resident ? "true" : "false", per.c_str(),
      r.kernel_us, r.arrival_spread_us, r.total_us, r.in_flight_s, r.kept_queue ? "true" : "false", r.kfd_node_id,
      json_escape(r.pci_bus_id).c_str(), json_escape(r.error).c_str());
}

inline std::string perf_json(const mi355x_perf_result& r) {
  std::string per = "[";
  for (int i = 0; i < 16 && i < (r.num_xcc > 0 ? r.num_xcc : 8); ++i)
    per += json_format("%s%.0f", i ? "," : "", r.xcd_clock_mhz[i]);
  per += "]";
  return json_format(
      "{\"ordinal\":%d,\"ok\":%s,\"hsa_error\":%d,\"nonce\":%u,\"bytes\":%llu,\"cu_count\":%d,"
      "\"num_xcc\":%d,\"fill_us\":%.1f,\"check_us\":%.1f,\"check2_us\":%.1f,\"hbm_write_gbps\":%.1f,"
      "\"hbm_read_gbps\":%.1f,\"hbm_bad_words\":%llu,\"hbm_bad_words_pass2\":%llu,\"hbm_first_bad\":%lld,"
      "\"mfma_iters\":%d,\"mfma_grid\":%d,"
      "\"mfma_records_ok\":%d,\"mfma_checksum_mismatch\":%d,\"mfma_xccs\":%d,\"mfma_us\":%.1f,"
      "\"mfma_tflops\":%.1f,\"clock_mhz_min\":%.0f,\"clock_mhz_median\":%.0f,\"clock_mhz_max\":%.0f,"
      "\"xcd_clock_mhz\":%s,\"total_us\":%.1f,\"in_flight_s\":%.2f,\"kept_queue\":%s,\"kfd_node_id\":%d,"
      "\"pci_bus_id\":\"%s\",\"error\":\"%s\"}",
      r.ordinal, r.ok ? "true" : "false", r.hsa_error, r.nonce, static_cast<unsigned long long>(r.bytes), r.cu_count,
      r.num_xcc, r.fill_us, r.check_us, r.check2_us, r.hbm_write_gbps, r.hbm_read_gbps,
      static_cast<unsigned long long>(r.hbm_bad_words), static_cast<unsigned long long>(r.hbm_bad_words_pass2),
      static_cast<long long>(r.hbm_first_bad), r.mfma_iters, r.mfma_grid, r.mfma_records_ok, r.mfma_checksum_mismatch,
      r.mfma_xccs, r.mfma_us, r.mfma_tflops, r.clock_mhz_min, r.clock_mhz_median, r.clock_mhz_max, per.c_str(),
      r.total_us, r.in_flight_s, r.kept_queue ? "true" : "false", r.kfd_node_id,
      json_escape(r.pci_bus_id).c_str(), json_escape(r.error).c_str());
}

inline std::string datapath_json(const mi355x_datapath_result& r) {
  return json_format(
      "{\"ordinal\":%d,\"ok\":%s,\"hsa_error\":%d,\"nonce\":%u,\"grid\":%d,\"cu_count\":%d,\"num_xcc\":%d,"
      "\"records_ok\":%d,\"mfma_bad\":%u,\"stage_bad\":[%u,%u,%u,%u],\"tile_bad\":%u,"
      "\"first_bad_wg\":%d,\"first_bad_stage\":%d,\"first_bad_word\":%d,\"first_bad_got\":%u,"
      "\"first_bad_want\":%u,\"first_bad_xor\":%u,\"cus_covered\":%d,\"simds_covered\":%d,\"xccs_covered\":%d,"
      "\"kernel_us\":%.2f,\"total_us\":%.1f,\"in_flight_s\":%.2f,\"kept_queue\":%s,\"kfd_node_id\":%d,"
      "\"pci_bus_id\":\"%s\",\"error\":\"%s\"}",
      r.ordinal, r.ok ? "true" : "false", r.hsa_error, r.nonce, r.grid, r.cu_count, r.num_xcc, r.records_ok,
      r.mfma_bad, r.stage_bad[0], r.stage_bad[1], r.stage_bad[2], r.stage_bad[3], r.tile_bad, r.first_bad_wg,
      r.first_bad_stage, r.first_bad_word, r.first_bad_got, r.first_bad_want, r.first_bad_xor, r.cus_covered,
      r.simds_covered, r.xccs_covered, r.kernel_us, r.total_us, r.in_flight_s, r.kept_queue ? "true" : "false", r.kfd_node_id,
      json_escape(r.pci_bus_id).c_str(), json_escape(r.error).c_str());
}

inline std::string datapath_i8_json(const mi355x_datapath_i8_result& r) {
  return json_format(
      "{\"ordinal\":%d,\"ok\":%s,\"hsa_error\":%d,\"nonce\":%u,\"grid\":%d,\"cu_count\":%d,\"num_xcc\":%d,"
      "\"records_ok\":%d,\"mfma_bad\":%u,\"stage_bad\":[%u,%u,%u,%u,%u],\"tile_bad\":%u,"
      "\"first_bad_wg\":%d,\"first_bad_stage\":%d,\"first_bad_word\":%d,\"first_bad_got\":%u,"
      "\"first_bad_want\":%u,\"first_bad_xor\":%u,\"cus_covered\":%d,\"simds_covered\":%d,\"xccs_covered\":%d,"
      "\"kernel_us\":%.2f,\"total_us\":%.1f,\"in_flight_s\":%.2f,\"kept_queue\":%s,\"kfd_node_id\":%d,"
      "\"pci_bus_id\":\"%s\",\"error\":\"%s\"}",
      r.ordinal, r.ok ? "true" : "false", r.hsa_error, r.nonce, r.grid, r.cu_count, r.num_xcc, r.records_ok,
      r.mfma_bad, r.stage_bad[0], r.stage_bad[1], r.stage_bad[2], r.stage_bad[3], r.stage_bad[4], r.tile_bad,
      r.first_bad_wg, r.first_bad_stage, r.first_bad_word, r.first_bad_got, r.first_bad_want, r.first_bad_xor,
      r.cus_covered, r.simds_covered, r.xccs_covered, r.kernel_us, r.total_us, r.in_flight_s,
      r.kept_queue ? "true" : "false", r.kfd_node_id,
      json_escape(r.pci_bus_id).c_str(), json_escape(r.error).c_str());
}

// the bf16 check's result is the int8 check's (liveness_probe.h): the same line
inline std::string datapath_bf16_json(const mi355x_datapath_bf16_result& r) { return datapath_i8_json(r); }

// the fp8 check's line: the int8 check's with eight stage counts
inline std::string datapath_fp8_json(const mi355x_datapath_fp8_result& r) {
  return json_format(
      "{\"ordinal\":%d,\"ok\":%s,\"hsa_error\":%d,\"nonce\":%u,\"grid\":%d,\"cu_count\":%d,\"num_xcc\":%d,"
      "\"records_ok\":%d,\"mfma_bad\":%u,\"stage_bad\":[%u,%u,%u,%u,%u,%u,%u,%u],\"tile_bad\":%u,"
      "\"first_bad_wg\":%d,\"first_bad_stage\":%d,\"first_bad_word\":%d,\"first_bad_got\":%u,"
      "\"first_bad_want\":%u,\"first_bad_xor\":%u,\"cus_covered\":%d,\"simds_covered\":%d,\"xccs_covered\":%d,"
      "\"kernel_us\":%.2f,\"total_us\":%.1f,\"in_flight_s\":%.2f,\"kept_queue\":%s,\"kfd_node_id\":%d,"
      "\"pci_bus_id\":\"%s\",\"error\":\"%s\"}",
      r.ordinal, r.ok ? "true" : "false", r.hsa_error, r.nonce, r.grid, r.cu_count, r.num_xcc, r.records_ok,
      r.mfma_bad, r.stage_bad[0], r.stage_bad[1], r.stage_bad[2], r.stage_bad[3], r.stage_bad[4], r.stage_bad[5],
      r.stage_bad[6], r.stage_bad[7], r.tile_bad, r.first_bad_wg, r.first_bad_stage, r.first_bad_word,
      r.first_bad_got, r.first_bad_want, r.first_bad_xor, r.cus_covered, r.simds_covered, r.xccs_covered,
      r.kernel_us, r.total_us, r.in_flight_s, r.kept_queue ? "true" : "false", r.kfd_node_id,
      json_escape(r.pci_bus_id).c_str(), json_escape(r.error).c_str());
}

// the f16 check's line: the int8 check's with seven stage counts
inline std::string datapath_f16_json(const mi355x_datapath_f16_result& r) {
  return json_format(
      "{\"ordinal\":%d,\"ok\":%s,\"hsa_error\":%d,\"nonce\":%u,\"grid\":%d,\"cu_count\":%d,\"num_xcc\":%d,"
      "\"records_ok\":%d,\"mfma_bad\":%u,\"stage_bad\":[%u,%u,%u,%u,%u,%u,%u],\"tile_bad\":%u,"
      "\"first_bad_wg\":%d,\"first_bad_stage\":%d,\"first_bad_word\":%d,\"first_bad_got\":%u,"
      "\"first_bad_want\":%u,\"first_bad_xor\":%u,\"cus_covered\":%d,\"simds_covered\":%d,\"xccs_covered\":%d,"
      "\"kernel_us\":%.2f,\"total_us\":%.1f,\"in_flight_s\":%.2f,\"kept_queue\":%s,\"kfd_node_id\":%d,"
      "\"pci_bus_id\":\"%s\",\"error\":\"%s\"}",
      r.ordinal, r.ok ? "true" : "false", r.hsa_error, r.nonce, r.grid, r.cu_count, r.num_xcc, r.records_ok,
      r.mfma_bad, r.stage_bad[0], r.stage_bad[1], r.stage_bad[2], r.stage_bad[3], r.stage_bad[4], r.stage_bad[5],
      r.stage_bad[6], r.tile_bad, r.first_bad_wg, r.first_bad_stage, r.first_bad_word,
      r.first_bad_got, r.first_bad_want, r.first_bad_xor, r.cus_covered, r.simds_covered, r.xccs_covered,
      r.kernel_us, r.total_us, r.in_flight_s, r.kept_queue ? "true" : "false", r.kfd_node_id,
      json_escape(r.pci_bus_id).c_str(), json_escape(r.error).c_str());
}

// phase_us of one device: HSA build = code object, queue, buffers, dispatch;
// HIP build = hipSetDevice + identity, the stream's queue, buffers + events, dispatch
inline std::string device_json(const mi355x_probe_result& r, bool hsa_build) {
  const std::string phases =
      hsa_build ? json_format("\"code_object\":%.1f,\"queue\":%.1f,\"buffers\":%.1f,\"dispatch_wait\":%.1f",
                              r.phase_us[0], r.phase_us[1], r.phase_us[2], r.phase_us[3])
                : json_format("\"device\":%.1f,\"stream\":%.1f,\"buffers\":%.1f,\"dispatch_wait\":%.1f", r.phase_us[0],
                              r.phase_us[1], r.phase_us[2], r.phase_us[3]);
  return json_format(
      "{\"ordinal\":%d,\"ok\":%s,\"hip_error\":%d,\"mismatches\":%d,\"nonce\":%u,\"xcc_id\":%u,"
      "\"hw_id\":%u,\"iters\":%d,\"dispatches\":%d,\"kfd_node_id\":%d,\"runtime\":\"%s\","
      "\"kernel_us\":%.3f,\"setup_us\":%.3f,\"total_us\":%.3f,"
      "\"phase_us\":{%s},"
      "\"pci_bus_id\":\"%s\","
      "\"arch\":\"%s\",\"name\":\"%s\",\"uuid\":\"%s\",\"pci_domain\":%d,\"pci_bus\":%d,"
      "\"pci_device\":%d,\"cu_count\":%d,\"total_mem\":%llu,\"late\":%s,\"pending_s\":%.3f,\"error\":\"%s\"}",
      r.ordinal, r.ok ? "true" : "false", r.hip_error, r.mismatches, r.nonce, r.xcc_id, r.hw_id, r.iters,
      r.dispatches, r.kfd_node_id, r.runtime, r.kernel_us, r.setup_us, r.total_us, phases.c_str(),
      json_escape(r.pci_bus_id).c_str(), json_escape(r.arch).c_str(), json_escape(r.name).c_str(),
      json_escape(r.uuid).c_str(), r.pci_domain, r.pci_bus, r.pci_device, r.cu_count,
      static_cast<unsigned long long>(r.total_mem), r.late ? "true" : "false", r.pending_s,
      json_escape(r.error).c_str());
}

// ---- --serve: the hello line and what goes around a reply's devices ----------
// `n`: the runtime's GPU count, negative when it did not start
inline std::string serve_hello_json(int n, bool concurrent, uint64_t t_start_ns, uint64_t t_runtime_ns) {
  return json_format(
      "{\"serve\":true,\"ok\":%s,\"hip_device_count\":%d,\"concurrent\":%s,\"deadlines\":true,"
      "\"t_start_ns\":%llu,\"t_runtime_ns\":%llu}",
      n >= 0 ? "true" : "false", n < 0 ? 0 : n, concurrent ? "true" : "false",
      static_cast<unsigned long long>(t_start_ns), static_cast<unsigned long long>(t_runtime_ns));
}

// "id" only for a tagged request
inline std::string id_field(bool tagged, unsigned long long id) {
  return tagged ? "\"id\":" + std::to_string(id) + "," : std::string();
}

// `devices`: the JSON array of the device objects. Only a datapath reply
// carries its kind's key: the other replies stay as they were.
inline std::string serve_reply_json(bool tagged, unsigned long long id, const std::string& kind, bool ok, int n,
                                    uint64_t t_ready_ns, const std::string& devices) {
  const std::string head = json_format(
      "{%s\"ok\":%s,\"hip_device_count\":%d,\"sweep\":%s,\"perf\":%s,\"t_ready_ns\":%llu,", id_field(tagged, id).c_str(),
      ok ? "true" : "false", n, kind == "sweep" ? "true" : "false", kind == "perf" ? "true" : "false",
      static_cast<unsigned long long>(t_ready_ns));
  const char* key = kind == "datapath" ? "\"datapath\":true," : kind == "datapath_i8"   ? "\"datapath_i8\":true,"
                    : kind == "datapath_bf16" ? "\"datapath_bf16\":true,"
                    : kind == "datapath_fp8"  ? "\"datapath_fp8\":true,"
                    : kind == "datapath_f16"  ? "\"datapath_f16\":true,"
                                              : "";
  return head + key + "\"devices\":" + devices + "}";
}

// the answer to a line outside the request grammar; the server goes on
inline std::string bad_request_json(bool tagged, unsigned long long id) {
  return "{" + id_field(tagged, id) + "\"ok\":false,\"error\":\"bad request\",\"devices\":[]}";
}

// ---- one-shot: the whole document (no trailing newline) -----------------------
// `code`: the runtime's start-up error; `init_profile`: JSON or "null"
inline std::string runtime_init_failed_json(int code, uint64_t t_start_ns, const std::string& init_profile) {
  return json_format(
      "{\"ok\":false,\"hip_device_count\":0,\"error\":\"GPU runtime init failed (%d)\",\"devices\":[],"
      "\"t_start_ns\":%llu,\"t_ready_ns\":0,\"init_profile\":%s}",
      code, static_cast<unsigned long long>(t_start_ns), init_profile.c_str());
}

// --sweep / --perf / --datapath / --datapath-i8 / --datapath-bf16 / --datapath-fp8 / --datapath-f16
inline std::string oneshot_check_json(const std::string& kind, bool ok, int n, uint64_t t_start_ns,
                                      uint64_t t_runtime_ns, uint64_t t_ready_ns, const std::string& devices) {
  return json_format(
      "{\"ok\":%s,\"%s\":true,\"hip_device_count\":%d,\"t_start_ns\":%llu,\"t_runtime_ns\":%llu,"
      "\"t_ready_ns\":%llu,\"devices\":%s}",
      ok ? "true" : "false", kind.c_str(), n, static_cast<unsigned long long>(t_start_ns),
      static_cast<unsigned long long>(t_runtime_ns), static_cast<unsigned long long>(t_ready_ns), devices.c_str());
}

// the liveness probe (or --identify); what it measured of its own start-up
struct OneshotProbeTimes {
  uint64_t t_start_ns, t_runtime_ns, t_ready_ns;
  double cpu_ms_runtime, cpu_user_ms_runtime, cpu_ms_ready;
  long long read_syscalls_runtime;
  double init_us[5];  // dlopen, kfd_open, hsa_init, agents, pools
};

// `init_profile`, `view`: JSON or "null"
inline std::string oneshot_probe_json(bool ok, int n, bool identify, const OneshotProbeTimes& t,
                                      const std::string& init_profile, const std::string& view,
                                      const std::string& devices) {
  return json_format(
      "{\"ok\":%s,\"hip_device_count\":%d,\"identify\":%s,\"t_start_ns\":%llu,\"t_runtime_ns\":%llu,"
      "\"t_ready_ns\":%llu,\"cpu_ms_runtime\":%.2f,\"cpu_user_ms_runtime\":%.2f,\"cpu_ms_ready\":%.2f,\"read_syscalls_runtime\":%lld,"
      "\"init_us\":{\"dlopen\":%.1f,\"kfd_open\":%.1f,\"hsa_init\":%.1f,\"agents\":%.1f,\"pools\":%.1f},\"init_profile\":%s,"
      "\"view\":%s,\"devices\":%s}",
      ok ? "true" : "false", n, identify ? "true" : "false", static_cast<unsigned long long>(t.t_start_ns),
      static_cast<unsigned long long>(t.t_runtime_ns), static_cast<unsigned long long>(t.t_ready_ns), t.cpu_ms_runtime,
      t.cpu_user_ms_runtime, t.cpu_ms_ready, t.read_syscalls_runtime, t.init_us[0], t.init_us[1], t.init_us[2],
      t.init_us[3], t.init_us[4], init_profile.c_str(), view.c_str(), devices.c_str());
}

}  // namespace mi355x
