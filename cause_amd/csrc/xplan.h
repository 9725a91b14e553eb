// xplan.h -- where the exact path's synthetic lists lie (exact.hip): the flagged
// documents that take part, split into groups that weave_tail weaves in one
// call each.  A pure function of its arguments; compiles without HIP.
#pragma once
#include <stdint.h>

#include <vector>

namespace cw {

constexpr uint32_t X_NONE = 0xFFFFFFFFu;  // a document that is not on the synthetic path

// Synthetic lists woven together: a batch of small documents, or one document
// on the giant tree.
struct XGroup {
  bool giant;
  uint64_t base;              // first synthetic index (a multiple of 32: its bits start a word)
  std::vector<uint64_t> off;  // the lists' offsets from base (one more entry than lists)
};

struct XPlan {
  std::vector<uint32_t> sb;  // per document: its list's first synthetic index, or X_NONE
  std::vector<XGroup> groups;
  uint64_t NS = 0;  // synthetic indices in all (sb holds their low 32 bits: the caller checks NS)
  size_t max_lists() const {  // the most lists in one group (at least 1)
    size_t m = 1;
    for (const XGroup &g : groups) m = m < g.off.size() - 1 ? g.off.size() - 1 : m;
    return m;
  }
};

// Document f (xoff[f + 1] - xoff[f] = n nodes) takes part when part[f], with
// n + 1 slots (slots2 false: layout 1) or 2n + 1 (layout 2).  Groups, in the
// order they are woven: the small documents without an early node, the small
// ones with one (early[f]), then every document of >= giant_min or >= limit
// slots on its own, in document order.  An empty group is left out.
inline XPlan x_plan(uint32_t F, const uint64_t *xoff, const uint8_t *part, const uint8_t *early,
                    bool slots2, uint32_t giant_min, uint32_t limit) {
  XPlan p;
  p.sb.assign(F, X_NONE);
  const auto slots = [&](uint32_t f) {
    const uint64_t n = xoff[f + 1] - xoff[f];
    return slots2 ? 2 * n + 1 : n + 1;
  };
  std::vector<uint32_t> small[2], big;
  for (uint32_t f = 0; f < F; f++) {
    if (!part[f]) continue;
    if (slots(f) >= giant_min || slots(f) >= limit) big.push_back(f);
    else small[early[f] ? 1 : 0].push_back(f);
  }
  for (const auto &s : small) {
    if (s.empty()) continue;
    p.groups.push_back(XGroup{false, p.NS, {0}});
    XGroup &g = p.groups.back();
    for (uint32_t f : s) {
      p.sb[f] = (uint32_t)(p.NS + g.off.back());
      g.off.push_back(g.off.back() + slots(f));
    }
    p.NS = (p.NS + g.off.back() + 31) & ~31ull;
  }
  for (uint32_t f : big) {
    p.sb[f] = (uint32_t)p.NS;
    p.groups.push_back(XGroup{true, p.NS, {0, slots(f)}});
    p.NS = (p.NS + slots(f) + 31) & ~31ull;
  }
  return p;
}

}  // namespace cw
