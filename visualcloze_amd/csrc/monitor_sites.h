// The sites of the Flux handle's numerics monitor (vc_flux_set_monitor) and the arithmetic of its log: which residual stream is tap /
// site number what, how many bytes a log takes and where the VcStat of (evaluation, site, sample) lies.  Host code only, nothing from
// HIP: flux_engine.hip (through flux_rules.h) uses it for the taps (vc_flux_set_tap) and the monitor alike - ONE enumeration -, tests/c_abi/monitor_check.cpp
// runs it alone under the sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/vcloze_hip.h"

// monitor.hip's scan kernel uses the same ordering rule on the device
#if defined(__HIPCC__)
#define VCMON_HD __host__ __device__
#else
#define VCMON_HD
#endif

namespace vcmon {

// ---- the taps: img_in, txt_in, then (img, txt) of every double block, then every single block
inline int tap_count(int depth, int depth_single) { return 2 + 2 * depth + depth_single; }
inline int tap_img_in() { return 0; }
inline int tap_txt_in() { return 1; }
inline int tap_double(int i, bool txt) { return 2 + 2 * i + (txt ? 1 : 0); }
inline int tap_single(int depth, int i) { return 2 + 2 * depth + i; }
// the name of tap `tap` -> buf (at most len - 1 characters, terminated); false past the end or on an empty buffer
inline bool tap_name(int depth, int depth_single, int tap, char* buf, int len) {
  if (!buf || len <= 0 || tap < 0 || tap >= tap_count(depth, depth_single)) return false;
  if (tap == 0) snprintf(buf, (size_t)len, "img_in");
  else if (tap == 1) snprintf(buf, (size_t)len, "txt_in");
  else if (tap < 2 + 2 * depth) snprintf(buf, (size_t)len, "double.%d.%s", (tap - 2) / 2, (tap - 2) % 2 ? "txt" : "img");
  else snprintf(buf, (size_t)len, "single.%d", tap - 2 - 2 * depth);
  return true;
}

// ---- the monitor's sites: level 1 = "v", "x"; level 2 = those, then every tap under its tap name, in tap order
constexpr int SITE_V = 0, SITE_X = 1, FIRST_TAP_SITE = 2;
inline int site_count(int level, int depth, int depth_single) {
  return level <= 0 ? 0 : level == 1 ? FIRST_TAP_SITE : FIRST_TAP_SITE + tap_count(depth, depth_single);
}
inline int site_of_tap(int tap) { return FIRST_TAP_SITE + tap; }
inline bool site_name(int level, int depth, int depth_single, int site, char* buf, int len) {
  if (!buf || len <= 0 || site < 0 || site >= site_count(level, depth, depth_single)) return false;
  if (site == SITE_V) snprintf(buf, (size_t)len, "v");
  else if (site == SITE_X) snprintf(buf, (size_t)len, "x");
  else return tap_name(depth, depth_single, site - FIRST_TAP_SITE, buf, len);
  return true;
}

// the order in which an evaluation WRITES its sites (what vc_flux_monitor_report calls first): the tap sites, then v, then x
VCMON_HD inline int site_rank(int site, int n_sites) { return site >= FIRST_TAP_SITE ? site - FIRST_TAP_SITE : n_sites - FIRST_TAP_SITE + site; }
VCMON_HD inline int site_at_rank(int rank, int n_sites) { return rank < n_sites - FIRST_TAP_SITE ? rank + FIRST_TAP_SITE : rank - (n_sites - FIRST_TAP_SITE); }

// ---- the log: [capacity_evals][n_sites][B] of VcStat; -1 for anything outside it (or sizes that are not positive).  The engine hands
// vc_tensor_stats log_index(0, site, 0) as the base of a site and log_row_stride as its out_stride; the kernel adds row * stride + b
inline int64_t log_row_stride(int n_sites, int B) { return (int64_t)n_sites * B; }
inline int64_t log_index(int64_t eval, int site, int b, int64_t capacity_evals, int n_sites, int B) {
  if (capacity_evals <= 0 || n_sites <= 0 || B <= 0 || eval < 0 || eval >= capacity_evals || site < 0 || site >= n_sites || b < 0 || b >= B)
    return -1;
  return eval * log_row_stride(n_sites, B) + (int64_t)site * B + b;
}
inline int64_t log_bytes(int64_t capacity_evals, int n_sites, int B) {
  if (capacity_evals <= 0 || n_sites <= 0 || B <= 0) return -1;
  return capacity_evals * n_sites * B * (int64_t)sizeof(VcStat);
}
// the block partials of ONE vc_tensor_stats launch over B samples (its launches are ordered on one stream and share it)
inline int64_t scratch_bytes(int B) { return B <= 0 ? -1 : (int64_t)B * 4 * VC_MONITOR_MAX_BLOCKS * (int64_t)sizeof(float); }
// a linear index of the log -> (evaluation, site, sample)
inline void log_split(int64_t index, int n_sites, int B, int32_t* eval, int32_t* site, int32_t* b) {
  *b = (int32_t)(index % B);
  *site = (int32_t)(index / B % n_sites);
  *eval = (int32_t)(index / B / n_sites);
}

}  // namespace vcmon
