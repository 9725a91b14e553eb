// Drives x_plan (cause_amd/csrc/xplan.h), the layout of the exact path's
// synthetic lists, against the two grouping loops exact_weave_flagged held
// before it shared one planner.  Built and run by tests/test_xplan.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "xplan.h"

namespace {

constexpr uint32_t LINK_IDX = 0x1FFFFFFFu;  // cw_internal.h: documents < 2^29 nodes

struct Group {
  bool giant, early;
  uint64_t base;
  std::vector<uint64_t> off;
};

struct Model {
  std::vector<uint32_t> sb;
  std::vector<Group> groups;
  uint64_t NS = 0;
};

// Layout 1 as exact_weave_flagged wrote it (part[f]: the document is not left
// to the serial fold), the uint32_t truncation of the bases included.
Model layout1(uint32_t F, const std::vector<uint64_t> &xoff, const std::vector<uint8_t> &part,
              const std::vector<uint8_t> &h_early, uint32_t giant_min, uint32_t limit) {
  std::vector<Group> groups;
  std::vector<uint32_t> sb(F, cw::X_NONE);
  uint64_t NS = 0;
  {
    std::vector<uint32_t> small[2], big;
    for (uint32_t f = 0; f < F; f++) {
      const uint64_t n = xoff[f + 1] - xoff[f];
      if (!part[f]) continue;
      if (n + 1 >= giant_min || n + 1 >= limit) big.push_back(f);
      else small[h_early[f] ? 1 : 0].push_back(f);
    }
    for (int e = 0; e < 2; e++) {
      if (small[e].empty()) continue;
      Group g{false, e == 1, NS, {0}};
      for (uint32_t f : small[e]) {
        sb[f] = (uint32_t)(NS + g.off.back());
        g.off.push_back(g.off.back() + (xoff[f + 1] - xoff[f]) + 1);
      }
      NS = (NS + g.off.back() + 31) & ~31ull;
      groups.push_back(std::move(g));
    }
    for (uint32_t f : big) {
      const uint64_t n = xoff[f + 1] - xoff[f];
      sb[f] = (uint32_t)NS;
      groups.push_back(Group{true, h_early[f] != 0, NS, {0, n + 1}});
      NS = (NS + n + 1 + 31) & ~31ull;
    }
  }
  return {sb, groups, NS};
}

// Layout 2 as exact_weave_flagged wrote it (x2[f]: the document has an early
// node and takes the anchor rounds).
Model layout2(uint32_t F, const std::vector<uint64_t> &xoff, const std::vector<uint8_t> &x2,
              uint32_t giant_min, uint32_t limit) {
  std::vector<uint32_t> sb2(F, cw::X_NONE);
  std::vector<Group> groups2;
  uint64_t NS2 = 0;
  {
    std::vector<uint32_t> small2, big2;
    for (uint32_t f = 0; f < F; f++) {
      if (!x2[f]) continue;
      const uint64_t n = xoff[f + 1] - xoff[f];
      if (2 * n + 1 >= giant_min || 2 * n + 1 >= limit) big2.push_back(f);
      else small2.push_back(f);
    }
    if (!small2.empty()) {
      Group g{false, true, NS2, {0}};
      for (uint32_t f : small2) {
        sb2[f] = (uint32_t)(NS2 + g.off.back());
        g.off.push_back(g.off.back() + 2 * (xoff[f + 1] - xoff[f]) + 1);
      }
      NS2 = (NS2 + g.off.back() + 31) & ~31ull;
      groups2.push_back(std::move(g));
    }
    for (uint32_t f : big2) {
      const uint64_t n = xoff[f + 1] - xoff[f];
      sb2[f] = (uint32_t)NS2;
      groups2.push_back(Group{true, true, NS2, {0, 2 * n + 1}});
      NS2 = (NS2 + 2 * n + 1 + 31) & ~31ull;
    }
  }
  return {sb2, groups2, NS2};
}

int failures = 0;
unsigned long cases = 0;
#define CHECK(x, ...)                                   \
  do {                                                  \
    if (!(x)) {                                         \
      if (failures++ < 10) {                            \
        fprintf(stderr, "line %d: %s: ", __LINE__, #x); \
        fprintf(stderr, __VA_ARGS__);                   \
        fprintf(stderr, "\n");                          \
      }                                                 \
    }                                                   \
  } while (0)

void same(const char *what, unsigned long id, const cw::XPlan &p, const Model &m, uint32_t F,
          const std::vector<uint8_t> &part) {
  CHECK(p.NS == m.NS, "%s %lu: NS %llu, before %llu", what, id, (unsigned long long)p.NS,
        (unsigned long long)m.NS);
  CHECK(p.sb == m.sb, "%s %lu: the bases differ", what, id);
  CHECK(p.groups.size() == m.groups.size(), "%s %lu: %zu groups, before %zu", what, id, p.groups.size(),
        m.groups.size());
  size_t lists = 1;
  for (size_t k = 0; k < p.groups.size() && k < m.groups.size(); k++) {
    const cw::XGroup &g = p.groups[k];
    CHECK(g.giant == m.groups[k].giant && g.base == m.groups[k].base && g.off == m.groups[k].off,
          "%s %lu: group %zu differs", what, id, k);
    CHECK(g.base % 32 == 0, "%s %lu: group %zu starts at %llu", what, id, k, (unsigned long long)g.base);
    CHECK(g.off.size() >= 2 && g.off[0] == 0, "%s %lu: group %zu is empty", what, id, k);
    CHECK(!g.giant || g.off.size() == 2, "%s %lu: giant group %zu holds %zu lists", what, id, k,
          g.off.size() - 1);
    lists = lists < g.off.size() - 1 ? g.off.size() - 1 : lists;
  }
  CHECK(p.max_lists() == lists, "%s %lu: max_lists %zu, the groups hold %zu", what, id, p.max_lists(), lists);
  for (uint32_t f = 0; f < F; f++)
    CHECK((p.sb[f] == cw::X_NONE) == !part[f] || p.NS > 0xFFFFFFFEull, "%s %lu: document %u", what, id, f);
}

// One size list: both layouts, with the given flags.
void run(unsigned long id, const std::vector<uint64_t> &sizes, const std::vector<uint8_t> &part,
         const std::vector<uint8_t> &early, uint32_t giant_min, uint32_t limit) {
  const uint32_t F = (uint32_t)sizes.size();
  std::vector<uint64_t> xoff(1, 0);
  for (uint64_t n : sizes) xoff.push_back(xoff.back() + n);
  same("layout 1", id, cw::x_plan(F, xoff.data(), part.data(), early.data(), false, giant_min, limit),
       layout1(F, xoff, part, early, giant_min, limit), F, part);
  // layout 2: the documents of layout 1 with an early node, every one early
  std::vector<uint8_t> x2(F);
  for (uint32_t f = 0; f < F; f++) x2[f] = part[f] && early[f];
  same("layout 2", id, cw::x_plan(F, xoff.data(), x2.data(), x2.data(), true, giant_min, limit),
       layout2(F, xoff, x2, giant_min, limit), F, x2);
  cases++;
}

// A size list under every flag pattern that matters: all take part or none,
// all early or none, and mixed.
void run_flags(unsigned long id, const std::vector<uint64_t> &sizes, uint32_t giant_min, uint32_t limit) {
  const size_t F = sizes.size();
  std::vector<uint8_t> zero(F, 0), one(F, 1), alt(F), alt3(F);
  for (size_t f = 0; f < F; f++) alt[f] = f & 1, alt3[f] = f % 3 != 0;
  run(id, sizes, one, one, giant_min, limit);
  run(id, sizes, one, zero, giant_min, limit);
  run(id, sizes, zero, one, giant_min, limit);
  run(id, sizes, one, alt, giant_min, limit);
  run(id, sizes, alt3, alt, giant_min, limit);
  run(id, sizes, alt, alt3, giant_min, limit);
}

}  // namespace

int main() {
  unsigned long id = 0;
  // F = 1, sizes on both sides of every boundary: n + 1 and 2n + 1 against
  // giant_min and giant_min - 1 (4,096 and 4,097: 2n + 1 is odd), against the
  // document limit, and giant_min = 0
  const std::vector<uint64_t> edge = {1,      2,      30,     31,     32,     33,       2046,     2047,
                                      2048,   2049,   4093,   4094,   4095,   4096,     4097,     4098,
                                      0x0FFFFFFEull, 0x0FFFFFFFull, 0x10000000ull, 0x1FFFFFFDull,
                                      0x1FFFFFFEull, 0x1FFFFFFFull};
  for (uint32_t gm : {0u, 1u, 4095u, 4096u, 4097u, 4098u, 0xFFFFFFFFu})
    for (uint32_t lim : {LINK_IDX - 1, LINK_IDX, 0xFFFFFFFFu}) {
      for (uint64_t n : edge) run_flags(id++, {n}, gm, lim);
      // the same sizes side by side (small ones share a group, the rest follow)
      run_flags(id++, std::vector<uint64_t>(edge.begin(), edge.begin() + 16), gm, lim);
      run_flags(id++, {4094, 4095, 4096, 2047, 2048, 4095, 7, 4094}, gm, lim);
    }
  // group sizes on both sides of a multiple of 32 (k lists of n + 1 slots)
  for (uint64_t total = 60; total <= 68; total++)
    for (uint64_t k : {1, 2, 3}) {
      std::vector<uint64_t> sizes(k, 1);
      sizes[0] = total - (k - 1) * 2 - 1;  // slots: sum (n + 1) = total
      run_flags(id++, sizes, 1u << 16, LINK_IDX);
      sizes.push_back(70000);  // and a giant one behind them
      run_flags(id++, sizes, 1u << 16, LINK_IDX);
    }
  // sums that pass 0xFFFFFFF0 - 16: the caller refuses these by NS and must
  // see the same NS (and the same truncated bases) as before
  for (uint64_t last : {0x0FFFFFC0ull, 0x0FFFFFD0ull, 0x0FFFFFDFull, 0x0FFFFFE0ull, 0x0FFFFFFFull, 0x1FFFFFFEull}) {
    const std::vector<uint64_t> sizes = {0x1FFFFFFEull, 0x1FFFFFFEull, 0x1FFFFFFEull, 0x1FFFFFFEull,
                                         0x1FFFFFFEull, 0x1FFFFFFEull, 0x1FFFFFFEull, 100,
                                         last};
    for (uint32_t gm : {1u << 16, 0xFFFFFFFFu})
      for (uint32_t lim : {LINK_IDX, 0xFFFFFFFFu}) run_flags(id++, sizes, gm, lim);
  }
  {
    std::vector<uint64_t> sizes(40, 0x1FFFFFFEull);  // far past 2^32
    run_flags(id++, sizes, 1u << 16, LINK_IDX);
    run_flags(id++, sizes, 0xFFFFFFFFu, 0xFFFFFFFFu);
  }
  // seeded random lists
  std::mt19937_64 rng(20261020);
  for (int it = 0; it < 4000; it++) {
    const uint32_t F = 1 + (uint32_t)(rng() % (it % 50 == 0 ? 300 : 12));
    const uint32_t gm = it % 7 == 0 ? 0u : it % 7 == 1 ? 0xFFFFFFFFu : 16u << (rng() % 10);
    std::vector<uint64_t> sizes(F);
    std::vector<uint8_t> part(F), early(F);
    for (uint32_t f = 0; f < F; f++) {
      const uint64_t r = rng();
      sizes[f] = 1 + ((r >> 8) % 4 == 0 ? (r >> 16) % (2ull * gm + 70) : (r >> 16) % 97);
      if (it % 97 == 0 && f % 5 == 0) sizes[f] = LINK_IDX - 3 + (r >> 40) % 6;
      part[f] = (r & 7) != 0;
      early[f] = (r >> 3 & 3) == 0;
    }
    run(id++, sizes, part, early, gm, it % 11 == 0 ? 0xFFFFFFFFu : LINK_IDX);
  }
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("%lu size lists, both layouts\nok\n", cases);
  return 0;
}
