// The JSON objects the probe prints for a chip sweep, a throughput check and the
// two datapath checks (shared by probe_main.cpp and the contract CLIs under
// native/tests, so a test sees exactly the line the prober parses), and the
// blank result each of them starts from. Strings grow as needed: a long
// escaped `error` next to wide numbers is never cut.
#pragma once

#include <cstdarg>
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
// ("none"). hbm_first_bad of the throughput result stays 0 here: a reply that
// never reached the runtime carries 0, mi355x_hsa_perf_check sets its own -1.
template <typename R>
R blank_result(int ordinal, uint32_t nonce) {
  R r{};
  r.ordinal = ordinal;
  r.nonce = nonce;
  if constexpr (std::is_same_v<R, mi355x_datapath_result> || std::is_same_v<R, mi355x_datapath_i8_result>)
    r.first_bad_wg = r.first_bad_stage = r.first_bad_word = -1;
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
      "\"in_flight_s\":%.2f,\"kept_queue\":%s,\"error\":\"%s\"}",
      r.ordinal, r.ok ? "true" : "false", r.hsa_error, r.nonce, r.iters, r.grid, r.cu_count, r.num_xcc, r.records_ok,
      r.mfma_bad, r.lds_bad, r.tile_bad, r.cus_covered, r.xccs_covered, r.all_resident ? "true" : "false", per.c_str(),
      r.kernel_us, r.arrival_spread_us, r.total_us, r.in_flight_s, r.kept_queue ? "true" : "false",
      json_escape(r.error).c_str());
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
      "\"xcd_clock_mhz\":%s,\"total_us\":%.1f,\"in_flight_s\":%.2f,\"kept_queue\":%s,\"error\":\"%s\"}",
      r.ordinal, r.ok ? "true" : "false", r.hsa_error, r.nonce, static_cast<unsigned long long>(r.bytes), r.cu_count,
      r.num_xcc, r.fill_us, r.check_us, r.check2_us, r.hbm_write_gbps, r.hbm_read_gbps,
      static_cast<unsigned long long>(r.hbm_bad_words), static_cast<unsigned long long>(r.hbm_bad_words_pass2),
      static_cast<long long>(r.hbm_first_bad), r.mfma_iters, r.mfma_grid, r.mfma_records_ok, r.mfma_checksum_mismatch,
      r.mfma_xccs, r.mfma_us, r.mfma_tflops, r.clock_mhz_min, r.clock_mhz_median, r.clock_mhz_max, per.c_str(),
      r.total_us, r.in_flight_s, r.kept_queue ? "true" : "false", json_escape(r.error).c_str());
}

inline std::string datapath_json(const mi355x_datapath_result& r) {
  return json_format(
      "{\"ordinal\":%d,\"ok\":%s,\"hsa_error\":%d,\"nonce\":%u,\"grid\":%d,\"cu_count\":%d,\"num_xcc\":%d,"
      "\"records_ok\":%d,\"mfma_bad\":%u,\"stage_bad\":[%u,%u,%u,%u],\"tile_bad\":%u,"
      "\"first_bad_wg\":%d,\"first_bad_stage\":%d,\"first_bad_word\":%d,\"first_bad_got\":%u,"
      "\"first_bad_want\":%u,\"first_bad_xor\":%u,\"cus_covered\":%d,\"simds_covered\":%d,\"xccs_covered\":%d,"
      "\"kernel_us\":%.2f,\"total_us\":%.1f,\"in_flight_s\":%.2f,\"kept_queue\":%s,\"error\":\"%s\"}",
      r.ordinal, r.ok ? "true" : "false", r.hsa_error, r.nonce, r.grid, r.cu_count, r.num_xcc, r.records_ok,
      r.mfma_bad, r.stage_bad[0], r.stage_bad[1], r.stage_bad[2], r.stage_bad[3], r.tile_bad, r.first_bad_wg,
      r.first_bad_stage, r.first_bad_word, r.first_bad_got, r.first_bad_want, r.first_bad_xor, r.cus_covered,
      r.simds_covered, r.xccs_covered, r.kernel_us, r.total_us, r.in_flight_s, r.kept_queue ? "true" : "false",
      json_escape(r.error).c_str());
}

inline std::string datapath_i8_json(const mi355x_datapath_i8_result& r) {
  return json_format(
      "{\"ordinal\":%d,\"ok\":%s,\"hsa_error\":%d,\"nonce\":%u,\"grid\":%d,\"cu_count\":%d,\"num_xcc\":%d,"
      "\"records_ok\":%d,\"mfma_bad\":%u,\"stage_bad\":[%u,%u,%u,%u,%u],\"tile_bad\":%u,"
      "\"first_bad_wg\":%d,\"first_bad_stage\":%d,\"first_bad_word\":%d,\"first_bad_got\":%u,"
      "\"first_bad_want\":%u,\"first_bad_xor\":%u,\"cus_covered\":%d,\"simds_covered\":%d,\"xccs_covered\":%d,"
      "\"kernel_us\":%.2f,\"total_us\":%.1f,\"in_flight_s\":%.2f,\"kept_queue\":%s,\"error\":\"%s\"}",
      r.ordinal, r.ok ? "true" : "false", r.hsa_error, r.nonce, r.grid, r.cu_count, r.num_xcc, r.records_ok,
      r.mfma_bad, r.stage_bad[0], r.stage_bad[1], r.stage_bad[2], r.stage_bad[3], r.stage_bad[4], r.tile_bad,
      r.first_bad_wg, r.first_bad_stage, r.first_bad_word, r.first_bad_got, r.first_bad_want, r.first_bad_xor,
      r.cus_covered, r.simds_covered, r.xccs_covered, r.kernel_us, r.total_us, r.in_flight_s,
      r.kept_queue ? "true" : "false", json_escape(r.error).c_str());
}

}  // namespace mi355x
