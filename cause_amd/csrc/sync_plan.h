// sync_plan.h -- the host half of cw_version / cw_delta (sync.hip): the checks
// of a cw_sync_batch and the choice of route.  Pure functions of their
// arguments; compiles without HIP (tests/sync_plan.cpp runs them under the
// sanitizers).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "causeweave_sync.h"

namespace cw {

constexpr uint32_t SY_WAVE_CAP = CW_SYNC_WAVE_CAP;  // most nodes of a document on the wave route
constexpr uint32_t SY_WG_CAP = 0xFFFFu;             // ... on the workgroup route (LW_MAXDOC's bound)
constexpr uint64_t SY_MAX_DOCS = 1ull << 22;        // documents of a call: one 1,024-thread workgroup each in one dispatch

enum SyRoute { SY_ROUTE_WAVE = 0, SY_ROUTE_WG = 1, SY_ROUTE_GENERAL = 2 };

struct SyShape {
  uint64_t D = 0, N = 0, largest = 0;  // documents, nodes, the largest document
};

// The route of a call: by its largest document and the two context options.
inline SyRoute sync_route(uint64_t largest, uint32_t opt_wave, uint32_t opt_fused) {
  if (!opt_fused || largest > SY_WG_CAP) return SY_ROUTE_GENERAL;
  if (!opt_wave || largest > SY_WAVE_CAP) return SY_ROUTE_WG;
  return SY_ROUTE_WAVE;
}

// The batch's own fields.  0 and *shape filled in, or -1 and the reason in err.
inline int sync_check_batch(const cw_sync_batch *b, SyShape *shape, char *err, size_t cap) {
  if (!b) return snprintf(err, cap, "null batch/result"), -1;
  if (b->site_bits < 1 || b->site_bits > 10) return snprintf(err, cap, "site_bits %u outside 1..10", b->site_bits), -1;
  if (b->site_shift > 63 || b->ts_shift > 63) return snprintf(err, cap, "bad key layout"), -1;
  const uint64_t *off = b->doc_offsets, D = b->n_docs;
  if (!off) return snprintf(err, cap, "doc_offsets is required (host memory)"), -1;
  if (off[0] != 0) return snprintf(err, cap, "doc_offsets[0] must be 0"), -1;
  if (D >= (0xFFFFFFFFull >> b->site_bits) + 1 || (D << b->site_bits) >= 0xFFFFFFFFull)
    return snprintf(err, cap, "batch too large: %llu documents of %u site ranks (limit 2^32-1 table words)",
                    (unsigned long long)D, 1u << b->site_bits), -1;
  if (D >= SY_MAX_DOCS)
    return snprintf(err, cap, "batch too large: %llu documents (limit 2^22-1 in one dispatch)", (unsigned long long)D), -1;
  uint64_t mx = 0;
  for (uint64_t d = 0; d < D; d++) {
    if (off[d + 1] < off[d]) return snprintf(err, cap, "doc_offsets not monotone"), -1;
    const uint64_t n = off[d + 1] - off[d];
    if (n > mx) mx = n;
  }
  if (off[D] >= 0xFFFFFFFFull)
    return snprintf(err, cap, "batch too large: N=%llu (limit 2^32-1)", (unsigned long long)off[D]), -1;
  if (off[D] && !b->id_key) return snprintf(err, cap, "null id_key"), -1;
  shape->D = D;
  shape->N = off[D];
  shape->largest = mx;
  return 0;
}

// A gathered output is there exactly when its input column is.
inline int sync_check_pairing(const cw_sync_batch *b, const cw_delta_result *r, char *err, size_t cap) {
  if ((b->cause == nullptr) != (r->delta_cause == nullptr))
    return snprintf(err, cap, "cause and delta_cause go together"), -1;
  if ((b->kind == nullptr) != (r->delta_kind == nullptr))
    return snprintf(err, cap, "kind and delta_kind go together"), -1;
  if ((b->cause_is_id == nullptr) != (r->delta_cause_is_id == nullptr))
    return snprintf(err, cap, "cause_is_id and delta_cause_is_id go together"), -1;
  return 0;
}

}  // namespace cw
