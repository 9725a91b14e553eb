// Drives lb_step (cause_amd/csrc/lookback.h), the rule that says when a
// stage's look-back words are cleared, through its corner cases on the CPU.
// Built and run by tests/test_lookback_epoch.py.
//
// The rule, as the three stages each wrote it before they shared it
// (weave_maps_packed, map_union_fused, list_union_fused):
//
//   if (++epoch >= 0xFFFF || lb != last_lb || words > last_words) {
//     clear `words` words;  epoch = 1;  last_lb = lb;  last_words = words;
//   }
//   launch with epoch
#include <cstdint>
#include <cstdio>
#include <set>

#include "lookback.h"

namespace {

struct Model {  // the rule above, word for word
  uint32_t epoch = 0, last_words = 0;
  const void *last_lb = nullptr;
  bool call(const void *lb, uint32_t words, uint32_t *ep) {
    bool clear = false;
    if (++epoch >= 0xFFFF || lb != last_lb || words > last_words) {
      clear = true;
      epoch = 1;
      last_lb = lb;
      last_words = words;
    }
    *ep = epoch;
    return clear;
  }
};

int failures = 0;
#define CHECK(x, ...)                               \
  do {                                              \
    if (!(x)) {                                     \
      if (failures++ < 10) {                        \
        fprintf(stderr, "line %d: %s: ", __LINE__, #x); \
        fprintf(stderr, __VA_ARGS__);               \
        fprintf(stderr, "\n");                      \
      }                                             \
    }                                               \
  } while (0)

struct Driver {
  cw::LookBack st;
  Model model;
  std::set<uint32_t> live;  // epochs handed out since the last clear
  unsigned long calls = 0, clears = 0;
  bool one_epoch = true;  // every call so far took one epoch: the model applies
  bool call(const void *buf, uint32_t words, uint32_t epochs = 1) {
    const cw::LbStep s = cw::lb_step(st, buf, words, epochs);
    one_epoch = one_epoch && epochs == 1;
    if (one_epoch) {
      uint32_t want;
      const bool want_clear = model.call(buf, words, &want);
      CHECK(s.clear == want_clear, "call %lu: clear %d, the rule says %d", calls, (int)s.clear, (int)want_clear);
      CHECK(s.first == want, "call %lu: epoch %u, the rule says %u", calls, s.first, want);
    }
    if (s.clear) {
      live.clear();
      clears++;
      CHECK(s.next.buf == buf && s.next.words == words, "call %lu: a clear records the buffer and its words", calls);
    } else {
      CHECK(s.next.buf == st.buf && s.next.words == st.words, "call %lu: the record changed without a clear", calls);
      CHECK(buf == st.buf && words <= st.words, "call %lu: words never cleared are read", calls);
    }
    for (uint32_t e = s.first; e < s.first + epochs; e++) {
      CHECK(e >= 1 && e <= 0xFFFE, "call %lu: epoch %u outside 1 .. 0xFFFE", calls, e);
      CHECK(live.insert(e).second, "call %lu: epoch %u used twice between two clears", calls, e);
    }
    CHECK(s.next.epoch == s.first + epochs - 1, "call %lu: the last epoch is not recorded", calls);
    st = s.next;
    calls++;
    return s.clear;
  }
};

}  // namespace

int main() {
  static unsigned long long buf_a[4], buf_b[4];
  {
    Driver d;
    CHECK(d.call(buf_a, 100), "first use clears");
    CHECK(!d.call(buf_a, 100), "the same call again does not");
    CHECK(!d.call(buf_a, 40), "fewer words do not");
    CHECK(d.call(buf_b, 40), "a moved buffer clears");
    CHECK(!d.call(buf_b, 40), "and settles");
    CHECK(d.call(buf_b, 41), "more words than were cleared clear");
    CHECK(d.call(buf_b, 100), "(the record is the cleared count, not the buffer's size)");
    CHECK(!d.call(buf_b, 100), "and settles");
    // across the wrap, twice
    const unsigned long before = d.clears;
    for (int i = 0; i < 2 * 65600; i++) d.call(buf_b, 100);
    CHECK(d.clears - before == 2, "2 x 65,600 calls: %lu clears", d.clears - before);
    printf("one epoch a call: %lu calls, %lu clears\n", d.calls, d.clears);
  }
  {
    // the wrap with changes of buffer and size mixed in
    Driver d;
    for (int i = 0; i < 65600; i++)
      d.call(i % 20011 == 20010 ? (const void *)buf_a : (const void *)buf_b, i % 9973 == 0 ? 200 : 150 - i % 7);
    printf("mixed: %lu calls, %lu clears\n", d.calls, d.clears);
  }
  for (uint32_t n : {2u, 3u, 7u, 64u}) {  // several epochs a call: the same invariants
    Driver d;
    for (int i = 0; i < 65600; i++) d.call(buf_a, 10, i % 5 == 4 ? 1 : n);
    CHECK(d.clears >= 2, "%u epochs a call: %lu clears", n, d.clears);
  }
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
