// lookback.h -- the decoupled look-back that numbers the output of a one-kernel
// stage (k_map_pack's key weaves, k_map_union's and k_list_union's merged
// nodes): workgroup i publishes its count in word i, then sums the words of its
// predecessors.  The host half (LookBack, lb_step) compiles without HIP.
#pragma once
#include <stdint.h>

namespace cw {

// look-back word: flags (2 bits) | the call's epoch (16 bits, LB_EPOCH) | count.
// LB_AGG: the count of workgroup i alone; LB_INC: the counts of 0 .. i.  A word
// of an earlier call reads as "not published yet", so the words need no
// clearing before each call (lb_step says when they do).
constexpr unsigned long long LB_AGG = 1ull << 62, LB_INC = 2ull << 62;
constexpr uint32_t LB_EPOCH = 46;

// A stage's look-back words between calls: the buffer, how many of its words
// have been cleared, the last epoch used.
struct LookBack {
  const void *buf = nullptr;
  uint32_t words = 0, epoch = 0;
};

struct LbStep {
  LookBack next;   // the state after this call
  uint32_t first;  // this call's epochs are first .. first + epochs - 1, in 1 .. 0xFFFE
  bool clear;      // the call's `words` words are zeroed first
};

// A call takes new epochs; the words are cleared only when the epochs would
// reach 0xFFFF, the buffer moved, or the call needs more words than were
// cleared.  A pure function of its arguments.
inline LbStep lb_step(const LookBack &s, const void *buf, uint32_t words, uint32_t epochs) {
  if (s.epoch + epochs >= 0xFFFFu || buf != s.buf || words > s.words)
    return {LookBack{buf, words, epochs}, 1u, true};
  return {LookBack{s.buf, s.words, s.epoch + epochs}, s.epoch + 1, false};
}

#ifdef __HIPCC__
// The atomics are relaxed: the 64-bit word is the whole message, flag and
// count, so there are no acquire / release fences around it.

// One thread: workgroup i's count (for i == 0 that is the inclusive word).
__device__ __forceinline__ void lb_publish(unsigned long long *lb, uint32_t i, uint32_t epoch,
                                           uint32_t count) {
  const unsigned long long w = (i == 0 ? LB_INC : LB_AGG) | ((unsigned long long)epoch << LB_EPOCH) | count;
  __hip_atomic_store(lb + i, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The first wave, all 64 lanes: the sum of the counts of workgroups 0 .. i-1
// (wave-uniform); for i > 0 it then stores workgroup i's inclusive word.  One
// window of 64 predecessors a round trip, back to the nearest inclusive word
// (earlier workgroups are dispatched first and publish before they look back,
// so the wait always ends).  Four windows a round trip lost against one.
__device__ __forceinline__ uint32_t lb_exclusive(unsigned long long *lb, uint32_t i, uint32_t epoch,
                                                 uint32_t count) {
  if (i == 0) return 0;
  const unsigned long long ep = (unsigned long long)epoch << LB_EPOCH;
  const uint32_t lane = threadIdx.x;  // (the first wave: < 64)
  uint32_t base = 0;
  for (int64_t q0 = (int64_t)i - 1;;) {
    const int64_t q = q0 - lane;  // lane 0 = the nearest predecessor
    unsigned long long v = q >= 0 ? __hip_atomic_load(lb + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                  : (LB_INC | ep);
    if (((v >> LB_EPOCH) & 0xFFFFull) != epoch) v = 0;  // an earlier call's word
    const uint64_t inc = __ballot((v >> 62) == 2), none = __ballot((v >> 62) == 0);
    const uint32_t first = inc ? (uint32_t)__builtin_ctzll(inc) : 64u;  // nearest inclusive
    const uint64_t need = first >= 63 ? ~0ull : ((2ull << first) - 1);
    if (none & need) {  // a workgroup in this window has not published yet
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    uint32_t x = lane <= first ? (uint32_t)v : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    base += x;
    if (first < 64) break;
    q0 -= 64;
  }
  if (lane == 0)
    __hip_atomic_store(lb + i, LB_INC | ep | (unsigned long long)(base + count), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  return base;
}
#endif

}  // namespace cw
