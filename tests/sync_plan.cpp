// The host half of cw_version / cw_delta (cause_amd/csrc/sync_plan.h) on the CPU:
// every check of a cw_sync_batch, the NULL pairing of the gathered columns and
// the choice of route.  Offsets live in exactly sized heap arrays, so that a
// check that reads past n_docs + 1 entries is caught by the address sanitizer
// tests/test_sync_plan.py builds this with.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "sync_plan.h"

using namespace cw;

static int failures = 0;
#define EXPECT(x)                                              \
  do {                                                         \
    if (!(x)) {                                                \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);   \
      failures++;                                              \
    }                                                          \
  } while (0)

static cw_sync_batch batch(const std::vector<uint64_t> &off, const uint64_t *id, uint32_t site_bits) {
  cw_sync_batch b;
  memset(&b, 0, sizeof b);
  b.n_docs = off.size() - 1;
  b.doc_offsets = off.data();
  b.id_key = id;
  b.ts_shift = 20;
  b.site_shift = 16;
  b.site_bits = site_bits;
  return b;
}

static bool refused(const cw_sync_batch *b, const char *why) {
  char err[256] = "";
  SyShape sh;
  sh.D = sh.N = sh.largest = 12345;
  const int rc = sync_check_batch(b, &sh, err, sizeof err);
  const bool ok = rc == -1 && strstr(err, why) && sh.D == 12345 && sh.N == 12345 && sh.largest == 12345;
  if (!ok) printf("  rc %d, err \"%s\", wanted \"%s\"\n", rc, err, why);
  return ok;
}

int main() {
  char err[256];
  SyShape sh;
  uint64_t ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};

  {  // a good batch: empty documents at the front, in the middle and at the end
    std::vector<uint64_t> off{0, 0, 3, 3, 8, 8};
    cw_sync_batch b = batch(off, ids, 4);
    EXPECT(sync_check_batch(&b, &sh, err, sizeof err) == 0);
    EXPECT(sh.D == 5 && sh.N == 8 && sh.largest == 5);
  }
  {  // D = 0, and documents without nodes and without ids
    std::vector<uint64_t> off{0};
    cw_sync_batch b = batch(off, nullptr, 1);
    EXPECT(sync_check_batch(&b, &sh, err, sizeof err) == 0 && sh.D == 0 && sh.N == 0 && sh.largest == 0);
    std::vector<uint64_t> off3{0, 0, 0, 0};
    b = batch(off3, nullptr, 10);
    EXPECT(sync_check_batch(&b, &sh, err, sizeof err) == 0 && sh.D == 3 && sh.N == 0);
  }
  {  // every refusal
    std::vector<uint64_t> off{0, 3, 8};
    cw_sync_batch b = batch(off, ids, 4);
    EXPECT(refused(nullptr, "null batch"));
    b.site_bits = 0;
    EXPECT(refused(&b, "site_bits"));
    b.site_bits = 11;
    EXPECT(refused(&b, "site_bits"));
    b.site_bits = 4;
    b.site_shift = 64;
    EXPECT(refused(&b, "key layout"));
    b.site_shift = 16;
    b.ts_shift = 64;
    EXPECT(refused(&b, "key layout"));
    b.ts_shift = 63;
    EXPECT(sync_check_batch(&b, &sh, err, sizeof err) == 0);
    b.doc_offsets = nullptr;
    EXPECT(refused(&b, "doc_offsets is required"));
    b.doc_offsets = off.data();
    b.id_key = nullptr;
    EXPECT(refused(&b, "null id_key"));
    std::vector<uint64_t> one{1, 3, 8}, down{0, 5, 3}, big{0, 0xFFFFFFFFull}, fits{0, 0xFFFFFFFEull};
    b = batch(one, ids, 4);
    EXPECT(refused(&b, "must be 0"));
    b = batch(down, ids, 4);
    EXPECT(refused(&b, "not monotone"));
    b = batch(big, ids, 4);
    EXPECT(refused(&b, "batch too large: N="));
    b = batch(fits, ids, 4);
    EXPECT(sync_check_batch(&b, &sh, err, sizeof err) == 0 && sh.N == 0xFFFFFFFEull);
    // n_docs << site_bits >= 2^32 - 1 is refused before any offset past the first is read
    std::vector<uint64_t> z{0};
    for (uint32_t sb = 1; sb <= 10; sb++) {
      b = batch(z, nullptr, sb);
      b.n_docs = (0xFFFFFFFFull >> sb) + 1;
      EXPECT(refused(&b, "documents of"));
      b.n_docs = ~0ull >> 3;
      EXPECT(refused(&b, "documents of"));
    }
    b = batch(z, nullptr, 1);
    b.n_docs = ~0ull;
    EXPECT(refused(&b, "documents of"));
    // ... and so are 2^22 documents: a workgroup a document must fit one dispatch
    b.n_docs = SY_MAX_DOCS;
    EXPECT(SY_MAX_DOCS * 1024 == 1ull << 32 && refused(&b, "in one dispatch"));
    // ... and the largest table that fits passes the check
    std::vector<uint64_t> wide((0xFFFFFFFEull >> 10) + 1, 0);
    b = batch(wide, nullptr, 10);
    EXPECT(sync_check_batch(&b, &sh, err, sizeof err) == 0 && (sh.D << 10) < 0xFFFFFFFFull);
  }
  {  // a gathered output is there exactly when its input column is
    std::vector<uint64_t> off{0, 8};
    uint64_t ca[8], oca[8];
    uint8_t kd[8], okd[8], ci[8], oci[8];
    for (int mask = 0; mask < 64; mask++) {
      cw_sync_batch b = batch(off, ids, 4);
      cw_delta_result r;
      memset(&r, 0, sizeof r);
      b.cause = mask & 1 ? ca : nullptr;
      r.delta_cause = mask & 2 ? oca : nullptr;
      b.kind = mask & 4 ? kd : nullptr;
      r.delta_kind = mask & 8 ? okd : nullptr;
      b.cause_is_id = mask & 16 ? ci : nullptr;
      r.delta_cause_is_id = mask & 32 ? oci : nullptr;
      const bool paired = !(mask & 1) == !(mask & 2) && !(mask & 4) == !(mask & 8) && !(mask & 16) == !(mask & 32);
      EXPECT((sync_check_pairing(&b, &r, err, sizeof err) == 0) == paired);
    }
  }
  {  // routes: every size at which the route changes, under every pair of options
    EXPECT(SY_WAVE_CAP == CW_SYNC_WAVE_CAP && SY_WG_CAP == 65535);
    const uint64_t sizes[] = {0, 1, 63, 64, 65, SY_WAVE_CAP - 1, SY_WAVE_CAP, SY_WAVE_CAP + 1, 1023, 1024, 1025,
                              SY_WG_CAP - 1, SY_WG_CAP, (uint64_t)SY_WG_CAP + 1, 0xFFFFFFFEull};
    for (uint64_t n : sizes) {
      const SyRoute want = n <= SY_WAVE_CAP ? SY_ROUTE_WAVE : n <= SY_WG_CAP ? SY_ROUTE_WG : SY_ROUTE_GENERAL;
      EXPECT(sync_route(n, 1, 1) == want);
      EXPECT(sync_route(n, 0, 1) == (want == SY_ROUTE_WAVE ? SY_ROUTE_WG : want));
      EXPECT(sync_route(n, 1, 0) == SY_ROUTE_GENERAL && sync_route(n, 0, 0) == SY_ROUTE_GENERAL);
    }
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
