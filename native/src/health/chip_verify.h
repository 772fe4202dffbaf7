// The verdicts of the full-chip sweep and of the throughput check: what the
// host decides from the records the kernels wrote (shared by hsa_chip.cpp and
// native/tests/kernel_contract_cli.cpp). Host only, no HSA: the caller owns
// the dispatch and hands over plain memory.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "liveness_kernel.h"
#include "mi355x/liveness_probe.h"
#include "probe_verify.h"

namespace mi355x {

// the host-visible counter words are filled with this byte before the burn
// kernel copies the device counters over them
constexpr int kPerfCounterFillByte = 0xA5;

// upper median: sorted[n / 2]
inline double median_of(std::vector<double> v) {
  if (v.empty()) return 0;
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

// `records`: grid * MI355X_SWEEP_REC_WORDS words, `tiles`: grid *
// MI355X_PROBE_OUT floats, as mi355x_chip_sweep left them. The caller has set
// out->nonce, out->iters and out->num_xcc; every verdict field must be zero.
inline void sweep_verdict(const uint32_t* records, const float* tiles, uint32_t grid, mi355x_sweep_result* out) {
  const uint32_t nonce = out->nonce;
  std::vector<uint32_t> keys;
  keys.reserve(grid);
  uint64_t tmin = UINT64_MAX, tmax = 0;
  uint32_t xmask = 0;
  bool all_res = true;
  for (uint32_t w = 0; w < grid; ++w) {
    const uint32_t* r = records + static_cast<size_t>(w) * MI355X_SWEEP_REC_WORDS;
    const bool present = r[MI355X_REC_MAGIC] == MI355X_SWEEP_MAGIC && r[MI355X_REC_WG] == w &&
                         r[MI355X_REC_NONCE] == (nonce ^ w);
    if (!present) continue;
    out->mfma_bad += r[MI355X_REC_MFMA_BAD];
    out->lds_bad += r[MI355X_REC_LDS_BAD];
    const uint32_t x = r[MI355X_REC_XCC] & 0xF;
    xmask |= 1u << x;
    ++out->wgs_per_xcc[x];
    keys.push_back((x << 16) | ((r[MI355X_REC_HWID] >> 8) & 0xFF));
    all_res = all_res && r[MI355X_REC_ARRIVED] >= grid;
    const uint64_t t = (static_cast<uint64_t>(r[MI355X_REC_T0_HI]) << 32) | r[MI355X_REC_T0_LO];
    tmin = t < tmin ? t : tmin;
    tmax = t > tmax ? t : tmax;
    // wave 0's tile against the host reference
    const uint32_t nw = sweep_nonce(nonce, w, 0);
    uint32_t tb = 0;
    const float* tile = tiles + static_cast<size_t>(w) * MI355X_PROBE_OUT;
    for (int i = 0; i < MI355X_PROBE_M; ++i)
      for (int j = 0; j < MI355X_PROBE_N; ++j) {
        float dot = 0.f;
        for (int k = 0; k < MI355X_PROBE_K; ++k) dot += probe_a(i, k, nw) * probe_b(k, j, nw);
        const float e = probe_c(i, j, nw) + static_cast<float>(out->iters) * dot;
        tb += !same_bits(tile[i * MI355X_PROBE_N + j], e);
      }
    out->tile_bad += tb;
    if (r[MI355X_REC_MFMA_BAD] == 0 && r[MI355X_REC_LDS_BAD] == 0 && tb == 0) ++out->records_ok;
  }
  std::sort(keys.begin(), keys.end());
  out->cus_covered = static_cast<int>(std::unique(keys.begin(), keys.end()) - keys.begin());
  out->xccs_covered = __builtin_popcount(xmask);
  out->all_resident = all_res && out->records_ok == static_cast<int>(grid);
  if (tmax >= tmin && tmin != UINT64_MAX) out->arrival_spread_us = static_cast<double>(tmax - tmin) / 100.0;
  out->ok = out->records_ok == static_cast<int>(grid) && (out->num_xcc <= 0 || out->xccs_covered == out->num_xcc);
  if (!out->ok)
    std::snprintf(out->error, sizeof(out->error),
                  "%d/%d workgroups correct (mfma_bad=%u lds_bad=%u tile_bad=%u), %d/%d XCDs ran", out->records_ok,
                  grid, out->mfma_bad, out->lds_bad, out->tile_bad, out->xccs_covered, out->num_xcc);
}

// `records`: burn_wgs * MI355X_PERF_REC_WORDS words as mi355x_mfma_burn left
// them, `counters`: the host copy of the HBM check's words ([0] / [1] bad words
// of the two read passes, [2..3] first bad unit). The caller has set
// out->nonce, bytes, num_xcc, mfma_iters, fill_us, check_us, check2_us and
// mfma_us; every verdict field must be zero.
inline void perf_verdict(const uint32_t* records, const uint32_t counters[4], uint32_t burn_wgs,
                         mi355x_perf_result* out) {
  const uint32_t nonce = out->nonce;
  const uint64_t bytes = out->bytes;
  out->hbm_bad_words = counters[0] > counters[1] ? counters[0] : counters[1];
  out->hbm_bad_words_pass2 = counters[1];
  const uint64_t first = (static_cast<uint64_t>(counters[3]) << 32) | counters[2];
  // a unit the buffer does not have is no unit: the words were never written
  // by the kernels (the host's fill, or anything else)
  const bool first_is_unit = first < bytes / 16;
  const bool counters_unwritten = first != ~0ull && !first_is_unit;
  out->hbm_first_bad = first_is_unit ? static_cast<int64_t>(first) : -1;
  if (out->fill_us > 0) out->hbm_write_gbps = static_cast<double>(bytes) / (out->fill_us * 1e3);
  // the faster read pass that has a time at all
  double best_check = out->check_us;
  if (out->check2_us > 0 && (best_check <= 0 || out->check2_us < best_check)) best_check = out->check2_us;
  if (best_check > 0) out->hbm_read_gbps = static_cast<double>(bytes) / (best_check * 1e3);
  const double flops = 2.0 * 32 * 32 * 16 * 2.0 * static_cast<double>(out->mfma_iters) * (MI355X_PERF_THREADS / 64) *
                       static_cast<double>(burn_wgs);
  if (out->mfma_us > 0) out->mfma_tflops = flops / (out->mfma_us * 1e6);
  std::vector<double> clocks;
  std::vector<std::vector<double>> per_xcd(16);
  uint32_t ref = 0;
  bool have_ref = false, ref_finite = true;
  uint32_t xmask = 0;
  for (uint32_t wg = 0; wg < burn_wgs; ++wg) {
    const uint32_t* r = records + static_cast<size_t>(wg) * MI355X_PERF_REC_WORDS;
    if (r[MI355X_PREC_MAGIC] != MI355X_PERF_MAGIC || r[MI355X_PREC_WG] != wg || r[MI355X_PREC_NONCE] != (nonce ^ wg))
      continue;
    ++out->mfma_records_ok;
    for (int v = 0; v < MI355X_PERF_THREADS / 64; ++v) {
      if (!have_ref) {
        ref = r[MI355X_PREC_SUM + v];
        have_ref = true;
        // operands below 1 and at most 2^22 iterations: a correct checksum is
        // finite, so identical NaN / Inf words everywhere are no agreement
        ref_finite = (ref & 0x7F800000u) != 0x7F800000u;
        if (!ref_finite) ++out->mfma_checksum_mismatch;
      } else if (!ref_finite || r[MI355X_PREC_SUM + v] != ref) {
        ++out->mfma_checksum_mismatch;
      }
    }
    const uint64_t rt0 = (static_cast<uint64_t>(r[MI355X_PREC_RT0_HI]) << 32) | r[MI355X_PREC_RT0_LO];
    const uint64_t rt1 = (static_cast<uint64_t>(r[MI355X_PREC_RT1_HI]) << 32) | r[MI355X_PREC_RT1_LO];
    const uint64_t cyc = (static_cast<uint64_t>(r[MI355X_PREC_CYC_HI]) << 32) | r[MI355X_PREC_CYC_LO];
    const uint32_t x = r[MI355X_PREC_XCC] & 0xF;
    xmask |= 1u << x;
    if (rt1 > rt0) {
      const double mhz = static_cast<double>(cyc) / (static_cast<double>(rt1 - rt0) / 100.0);  // ticks per us
      clocks.push_back(mhz);
      per_xcd[x].push_back(mhz);
    }
  }
  out->mfma_xccs = __builtin_popcount(xmask);
  if (!clocks.empty()) {
    out->clock_mhz_min = *std::min_element(clocks.begin(), clocks.end());
    out->clock_mhz_max = *std::max_element(clocks.begin(), clocks.end());
    out->clock_mhz_median = median_of(clocks);
  }
  for (int x = 0; x < 16; ++x) out->xcd_clock_mhz[x] = median_of(per_xcd[x]);
  out->ok = out->hbm_bad_words == 0 && out->mfma_checksum_mismatch == 0 &&
            out->mfma_records_ok == static_cast<int>(burn_wgs) &&
            (out->num_xcc <= 0 || out->mfma_xccs == out->num_xcc);
  if (!out->ok)
    std::snprintf(out->error, sizeof(out->error),
                  "hbm_bad_words=%llu first_bad_unit=%lld mfma records %d/%u checksum mismatches %d, %d/%d XCDs ran%s",
                  static_cast<unsigned long long>(out->hbm_bad_words), static_cast<long long>(out->hbm_first_bad),
                  out->mfma_records_ok, burn_wgs, out->mfma_checksum_mismatch, out->mfma_xccs, out->num_xcc,
                  counters_unwritten ? "; HBM counters were not copied" : "");
}

}  // namespace mi355x
