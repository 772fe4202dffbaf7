// The request grammar of `mi355x-liveness-probe --serve` (shared by
// probe_main.cpp and native/tests/probe_contract_cli.cpp, so a host test
// parses a line exactly as the server does):
//     [@<id> ]probe <iters> <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]sweep <iters> <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]perf <mfma_iters> <timeout_s> <mib> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]datapath <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]datapath_i8 <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]datapath_bf16 <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]datapath_fp8 <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
//     [@<id> ]datapath_f16 <timeout_s> <ordinal>:<nonce>[:<deadline_s>] ...
// A device's own deadline (> 0) replaces the request's timeout for that device.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace mi355x {

struct ServeRequest {
  bool tagged = false;
  unsigned long long id = 0;
  std::string kind;  // probe | sweep | perf | datapath | datapath_i8 | datapath_bf16 | datapath_fp8 | datapath_f16
  int iters = 0;
  double timeout_s = 0;
  unsigned long long perf_mib = 0;
  std::vector<int> ords;
  std::vector<uint32_t> nonces;
  std::vector<double> timeouts;  // per device
};

// a line as read from stdin, without its end-of-line characters
inline void strip_eol(std::string* line) {
  while (!line->empty() && (line->back() == '\n' || line->back() == '\r')) line->pop_back();
}

// False for a line outside the grammar; r->tagged and r->id are then what was
// read of the tag (the bad-request reply carries the id of a well-formed tag).
// The device list may be empty. Text left over after it (a malformed device
// token, anything but blanks behind the last device) refuses the whole line:
// no request is answered for a part of its devices.
inline bool parse_request(const std::string& line, ServeRequest* r) {
  const char* p = line.c_str();
  if (*p == '@') {
    char* end = nullptr;
    const unsigned long long id = std::strtoull(p + 1, &end, 10);
    if (end == p + 1 || *end != ' ') return false;
    r->id = id;
    r->tagged = true;
    p = end + 1;
  }
  int consumed = 0;
  bool parsed = false;
  if (std::strncmp(p, "perf ", 5) == 0) {
    r->kind = "perf";
    parsed = std::sscanf(p, "perf %d %lf %llu %n", &r->iters, &r->timeout_s, &r->perf_mib, &consumed) >= 3;
  } else if (std::strncmp(p, "datapath_i8 ", 12) == 0) {
    r->kind = "datapath_i8";
    parsed = std::sscanf(p, "datapath_i8 %lf %n", &r->timeout_s, &consumed) >= 1;
  } else if (std::strncmp(p, "datapath_bf16 ", 14) == 0) {
    r->kind = "datapath_bf16";
    parsed = std::sscanf(p, "datapath_bf16 %lf %n", &r->timeout_s, &consumed) >= 1;
  } else if (std::strncmp(p, "datapath_fp8 ", 13) == 0) {
    r->kind = "datapath_fp8";
    parsed = std::sscanf(p, "datapath_fp8 %lf %n", &r->timeout_s, &consumed) >= 1;
  } else if (std::strncmp(p, "datapath_f16 ", 13) == 0) {
    r->kind = "datapath_f16";
    parsed = std::sscanf(p, "datapath_f16 %lf %n", &r->timeout_s, &consumed) >= 1;
  } else if (std::strncmp(p, "datapath ", 9) == 0) {
    r->kind = "datapath";
    parsed = std::sscanf(p, "datapath %lf %n", &r->timeout_s, &consumed) >= 1;
  } else if (std::strncmp(p, "sweep ", 6) == 0) {
    r->kind = "sweep";
    parsed = std::sscanf(p, "sweep %d %lf %n", &r->iters, &r->timeout_s, &consumed) >= 2;
  } else if (std::strncmp(p, "probe ", 6) == 0) {
    r->kind = "probe";
    parsed = std::sscanf(p, "probe %d %lf %n", &r->iters, &r->timeout_s, &consumed) >= 2;
  }
  if (!parsed || consumed == 0) return false;
  p += consumed;
  while (*p) {
    char* end = nullptr;
    const long o = std::strtol(p, &end, 10);
    if (end == p || *end != ':') return false;
    p = end + 1;
    const unsigned long nc = std::strtoul(p, &end, 0);
    if (end == p) return false;
    p = end;
    double dl = r->timeout_s;
    if (*p == ':') {
      const double v = std::strtod(p + 1, &end);
      if (end == p + 1) return false;
      if (v > 0) dl = v;
      p = end;
    }
    r->ords.push_back(static_cast<int>(o));
    r->nonces.push_back(static_cast<uint32_t>(nc));
    r->timeouts.push_back(dl);
    while (*p == ' ') ++p;
  }
  return true;
}

}  // namespace mi355x
