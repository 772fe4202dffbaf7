// The datapath check kinds of mi355x-liveness-probe, one row each: the checks
// whose request is `<wire> <timeout_s> <devices>` and whose one-shot flag is
// --datapath<suffix> (with --corrupt-datapath<suffix> beside it). The request
// grammar (probe_request.h), the reply's kind key (probe_json.h), the probe's
// flags, usage text and dispatch (probe_main.cpp), the prober's one-shot flag
// and request head (liveness_prober.cpp) and the daemon's "needs -liveness"
// checks (daemon/flags.cpp) all read this table. Host only, no dependencies.
//
// The order is the probe's precedence when several kind flags are given (the
// first row wins) and the order of the usage text.
#pragma once

#include <cstring>
#include <string>

namespace mi355x {

struct ProbeKind {
  const char* wire;    // the request verb, the reply's key and ServeRequest::kind
  const char* suffix;  // "" or "-f16": --datapath-f16, --corrupt-datapath-f16
};

inline constexpr ProbeKind kProbeKinds[] = {
    {"datapath", ""},
    {"datapath_i8", "-i8"},
    {"datapath_bf16", "-bf16"},
    {"datapath_fp8", "-fp8"},
    {"datapath_f16", "-f16"},
    {"datapath_f64", "-f64"},
    {"datapath_f6f4", "-f6f4"},
    {"datapath_sparse", "-sparse"},
    {"datapath_gemm", "-gemm"},
    {"datapath_splitk", "-splitk"},
    {"datapath_attn", "-attn"},
    {"datapath_mxgemm", "-mxgemm"},
    {"datapath_mxquant", "-mxquant"},
};
inline constexpr int kProbeKindCount = static_cast<int>(sizeof(kProbeKinds) / sizeof(kProbeKinds[0]));

// the row's index for the first `n` characters of `wire`, -1 when they name no row
inline int probe_kind_index(const char* wire, size_t n) {
  for (int i = 0; i < kProbeKindCount; ++i)
    if (std::strlen(kProbeKinds[i].wire) == n && std::memcmp(kProbeKinds[i].wire, wire, n) == 0) return i;
  return -1;
}
inline int probe_kind_index(const std::string& wire) { return probe_kind_index(wire.data(), wire.size()); }

inline std::string probe_kind_flag(const ProbeKind& k) { return std::string("--datapath") + k.suffix; }
inline std::string probe_kind_corrupt_flag(const ProbeKind& k) { return std::string("--corrupt-datapath") + k.suffix; }

}  // namespace mi355x
