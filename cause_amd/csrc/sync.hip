// sync.hip -- cw_version and cw_delta (include/causeweave_sync.h): the per-site
// heads of every document and the nodes above a peer's heads.  Included by
// causeweave.hip after listweft.hip (lookback.h, block_exscan).  Both read ids
// only; sync_plan.h holds the checks and the choice of route.
//
// Version.  ver[(d << site_bits) | r] = the largest id of site rank r in
// document d, yarn_len = how many, max_ts[d] = the largest id >> ts_shift.
//   wave / workgroup route: k_sync_version<NT, G>, G threads a document (a wave,
//     four documents a workgroup of 256; or a workgroup of 1,024).  The site
//     row (8 B maximum + 4 B count a rank) sits in LDS per document, zeroed,
//     filled by LDS atomics from one pass over the ids, written out whole.  LDS
//     at site_bits = 10: 12 KiB a document, 48 KiB a workgroup on the wave
//     route (three workgroups a CU), 12 KiB on the workgroup route; the row is
//     dynamic LDS, sized by site_bits (768 B a workgroup at site_bits = 4).
//   tiled route: k_sync_version_tiled, fixed tiles of SY_TILE node positions.  A
//     tile takes the documents it crosses one after the other: row in LDS, then
//     64-bit global atomicMax / atomicAdd of its nonzero words onto the table
//     the call zeroed.  Max and count do not depend on the order.
//
// Delta.  A node is in the delta iff id > have[its site rank].
//   wave / workgroup route: k_sync_delta<NT, G, BW>: the have row in LDS, each
//     wave ballots the flags of 64 consecutive nodes into a bitmap word, a block
//     scan of the popcounts, the workgroup's count published and its first
//     output position found by look-back (lookback.h), then the payloads of the
//     delta nodes only gathered to their final places.  With `ahead` the same
//     pass makes the version row in LDS and counts the ranks with have > ver.
//     LDS at site_bits = 10: rows 16 KiB a document; bitmap and prefix 12 KiB
//     (workgroup route) or 192 B (wave route).
//   general route: k_sync_delta_gen, a workgroup per document: a count pass,
//     scan_counts, a write pass.

constexpr uint32_t SY_WAVE_NT = 256;                           // the wave route's workgroup: four documents
constexpr uint32_t SY_WAVE_WORDS = (SY_WAVE_CAP + 63) / 64;    // bitmap words of one of them
constexpr uint32_t SY_WG_NT = 1024;
constexpr uint32_t SY_WG_WORDS = (SY_WG_CAP + 64) / 64;        // 1,024
constexpr uint32_t SY_TILE = 8192, SY_TILE_NT = 256;
static_assert(SY_WG_CAP == LW_MAXDOC, "the workgroup route's bound is the list weft's");

struct SyIn {
  const uint64_t *id;
  const uint32_t *off;  // device [D+1]
  uint32_t D, N, ts_shift, site_shift, site_bits;
};

struct SyDelta {
  const uint64_t *have;  // [D << site_bits]
  const uint64_t *cause;
  const uint8_t *kind, *cii;
  uint32_t *o_src;
  uint64_t *o_id, *o_cause;
  uint8_t *o_kind, *o_cii;
  uint32_t *ahead;  // [D] or nullptr
  uint64_t *o_off;  // device [D+1] (the fused routes)
};

__device__ __forceinline__ uint64_t sy_wave_max(uint64_t m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t y = __shfl_xor((unsigned long long)m, o, 64);
    m = y > m ? y : m;
  }
  return m;
}

__device__ __forceinline__ void sy_lds_max(uint64_t *p, uint64_t x) {
  atomicMax(reinterpret_cast<unsigned long long *>(p), (unsigned long long)x);  // (no returned value)
}

template <uint32_t NT, uint32_t G>
__global__ __launch_bounds__(NT) void k_sync_version(SyIn in, uint64_t *ver, uint32_t *ylen, uint64_t *max_ts) {
  constexpr uint32_t DG = NT / G, U = 4;
  extern __shared__ uint64_t sy_rows[];  // DG rows of S maxima, then DG rows of S counts
  __shared__ uint64_t gmax[DG];
  const uint32_t tid = threadIdx.x, g = tid / G, gl = tid % G;
  const uint32_t S = 1u << in.site_bits, smask = S - 1, shift = in.site_shift;
  const uint32_t d = blockIdx.x * DG + g;
  const bool active = d < in.D;
  uint64_t *const mx = sy_rows + (size_t)g * S;
  uint32_t *const cn = reinterpret_cast<uint32_t *>(sy_rows + (size_t)DG * S) + (size_t)g * S;
  for (uint32_t r = gl; r < S; r += G) {
    mx[r] = 0;
    cn[r] = 0;
  }
  if (gl == 0) gmax[g] = 0;
  __syncthreads();
  if (active) {
    const uint32_t b0 = in.off[d], n = in.off[d + 1] - b0;
    const uint64_t *const ids = in.id + b0;
    uint64_t m = 0;
    for (uint32_t i0 = gl; i0 < n; i0 += U * G) {
      uint64_t x[U];
#pragma unroll
      for (uint32_t u = 0; u < U; u++) {
        const uint32_t i = i0 + u * G;
        x[u] = i < n ? ids[i] : 0ull;
      }
#pragma unroll
      for (uint32_t u = 0; u < U; u++) {
        if (i0 + u * G >= n) continue;
        const uint32_t site = (uint32_t)(x[u] >> shift) & smask;
        sy_lds_max(&mx[site], x[u]);
        atomicAdd(&cn[site], 1u);
        m = x[u] > m ? x[u] : m;
      }
    }
    m = sy_wave_max(m);
    if ((tid & 63) == 0 && m) sy_lds_max(&gmax[g], m);
  }
  __syncthreads();
  if (active) {
    const uint64_t row = (uint64_t)d << in.site_bits;
    for (uint32_t r = gl; r < S; r += G) {
      ver[row + r] = mx[r];
      if (ylen) ylen[row + r] = cn[r];
    }
    if (gl == 0 && max_ts) max_ts[d] = gmax[g] >> in.ts_shift;
  }
}

// (ver, ylen and max_ts are zero when the kernel starts)
__global__ __launch_bounds__(SY_TILE_NT) void k_sync_version_tiled(SyIn in, uint64_t *ver, uint32_t *ylen,
                                                                  uint64_t *max_ts) {
  __shared__ uint64_t mx[1024];
  __shared__ uint32_t cn[1024];
  __shared__ uint64_t smax;
  const uint32_t tid = threadIdx.x;
  const uint32_t S = 1u << in.site_bits, smask = S - 1, shift = in.site_shift;
  const uint64_t t0 = (uint64_t)blockIdx.x * SY_TILE, t1 = t0 + SY_TILE < in.N ? t0 + SY_TILE : in.N;
  uint64_t pos = t0;
  while (pos < t1) {  // (uniform over the workgroup)
    // the document of position pos: off[d] <= pos < off[d + 1] (off[D] = N > pos)
    uint32_t lo = 0, hi = in.D;
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (in.off[mid] <= pos) lo = mid; else hi = mid;
    }
    const uint32_t d = lo;
    const uint64_t de = in.off[d + 1], e = de < t1 ? de : t1;
    for (uint32_t r = tid; r < S; r += SY_TILE_NT) {
      mx[r] = 0;
      cn[r] = 0;
    }
    if (tid == 0) smax = 0;
    __syncthreads();
    uint64_t m = 0;
    for (uint64_t i = pos + tid; i < e; i += SY_TILE_NT) {
      const uint64_t x = in.id[i];
      const uint32_t site = (uint32_t)(x >> shift) & smask;
      sy_lds_max(&mx[site], x);
      atomicAdd(&cn[site], 1u);
      m = x > m ? x : m;
    }
    m = sy_wave_max(m);
    if ((tid & 63) == 0 && m) sy_lds_max(&smax, m);
    __syncthreads();
    const uint64_t row = (uint64_t)d << in.site_bits;
    for (uint32_t r = tid; r < S; r += SY_TILE_NT) {
      if (!cn[r]) continue;
      if (mx[r]) atomicMax(reinterpret_cast<unsigned long long *>(ver + row + r), (unsigned long long)mx[r]);
      if (ylen) atomicAdd(ylen + row + r, cn[r]);
    }
    if (tid == 0 && max_ts && (smax >> in.ts_shift))
      atomicMax(reinterpret_cast<unsigned long long *>(max_ts + d), (unsigned long long)(smax >> in.ts_shift));
    __syncthreads();  // (the rows are zeroed again)
    pos = e;
  }
}

// The delta node at doc-local index i of the document that starts at b0 -> output slot o.
__device__ __forceinline__ void sy_gather(const SyIn &in, const SyDelta &a, uint32_t b0, uint32_t i, uint32_t o) {
  a.o_src[o] = i;
  if (a.o_id) a.o_id[o] = in.id[b0 + i];
  if (a.o_cause) a.o_cause[o] = a.cause[b0 + i];
  if (a.o_kind) a.o_kind[o] = a.kind[b0 + i];
  if (a.o_cii) a.o_cii[o] = a.cii[b0 + i];
}

// G threads a document, BW bitmap words a document (G * passes >= 64 * BW).
template <uint32_t NT, uint32_t G, uint32_t BW>
__global__ __launch_bounds__(NT) void k_sync_delta(SyIn in, SyDelta a, unsigned long long *lb, uint32_t epoch) {
  constexpr uint32_t DG = NT / G, W = DG * BW, GW = G / 64, U = 4;
  static_assert(W <= NT, "one bitmap word a thread in the scan");
  extern __shared__ uint64_t sy_rows[];  // DG have rows of S words, then (ahead) DG version rows
  __shared__ uint64_t bitmap[W];
  __shared__ uint32_t prefix[W];
  __shared__ uint32_t wtot[NT / 64];
  __shared__ uint32_t s_n[DG], s_ahead[DG];
  __shared__ uint32_t s_base;
  const uint32_t tid = threadIdx.x, lane = tid & 63, g = tid / G, gl = tid % G, wg = gl >> 6;
  const uint32_t S = 1u << in.site_bits, smask = S - 1, shift = in.site_shift;
  const uint32_t d = blockIdx.x * DG + g;
  const bool active = d < in.D, want_ahead = a.ahead != nullptr;
  const uint32_t b0 = active ? in.off[d] : 0u, n = active ? in.off[d + 1] - b0 : 0u;
  const uint32_t nwords = (n + 63) >> 6;
  const uint64_t *const ids = in.id + b0;
  uint64_t *const hv = sy_rows + (size_t)g * S;
  uint64_t *const mx = sy_rows + (size_t)(DG + g) * S;  // (only with ahead)
  // 1. the have row
  for (uint32_t r = gl; r < S; r += G) {
    hv[r] = active ? a.have[((uint64_t)d << in.site_bits) + r] : 0ull;
    if (want_ahead) mx[r] = 0;
  }
  if (gl == 0) {
    s_n[g] = n;
    s_ahead[g] = 0;
  }
  __syncthreads();

  // 2. the delta bitmap: wave wg of the document takes its words wg, wg + GW, ...
  for (uint32_t w0 = wg; w0 < nwords; w0 += U * GW) {
    uint64_t x[U];
#pragma unroll
    for (uint32_t u = 0; u < U; u++) {
      const uint32_t i = ((w0 + u * GW) << 6) + lane;
      x[u] = i < n ? ids[i] : 0ull;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; u++) {
      const uint32_t word = w0 + u * GW, i = (word << 6) + lane;
      bool in_delta = false;
      if (i < n) {
        const uint32_t site = (uint32_t)(x[u] >> shift) & smask;
        in_delta = x[u] > hv[site];
        if (want_ahead) sy_lds_max(&mx[site], x[u]);
      }
      const uint64_t m = __ballot(in_delta);
      if (lane == 0 && word < nwords) bitmap[g * BW + word] = m;
    }
  }
  __syncthreads();

  // 3. delta nodes before each bitmap word of the workgroup, in document order
  uint32_t pc = 0, tot;
  if (tid < W && (tid % BW) < ((s_n[tid / BW] + 63) >> 6)) pc = (uint32_t)__popcll(bitmap[tid]);
  const uint32_t ex = block_exscan<NT>(pc, wtot, &tot);
  if (tid < W) prefix[tid] = ex;
  if (want_ahead && active) {
    uint32_t k = 0;
    for (uint32_t r = gl; r < S; r += G) k += hv[r] > mx[r] ? 1u : 0u;
    if (k) atomicAdd(&s_ahead[g], k);
  }

  // 4. publish the workgroup's count, then sum the predecessors' (one wave)
  if (tid == 0) lb_publish(lb, blockIdx.x, epoch, tot);
  if (tid < 64) {
    const uint32_t b = lb_exclusive(lb, blockIdx.x, epoch, tot);
    if (tid == 0) s_base = b;
  }
  __syncthreads();  // (prefix[] and s_ahead[] are complete here as well)
  if (!active) return;
  const uint32_t base = s_base;

  // 5. the delta nodes at their final places (i & 63 == lane: G is a multiple of 64)
  const uint64_t below = (1ull << lane) - 1;
  for (uint32_t i = gl; i < n; i += G) {
    const uint64_t bits = bitmap[g * BW + (i >> 6)];
    if (!((bits >> lane) & 1ull)) continue;
    sy_gather(in, a, b0, i, base + prefix[g * BW + (i >> 6)] + (uint32_t)__popcll(bits & below));
  }
  if (gl == 0) {
    a.o_off[d] = (uint64_t)base + prefix[g * BW];
    if (d == in.D - 1) a.o_off[in.D] = (uint64_t)base + tot;
    if (want_ahead) a.ahead[d] = s_ahead[g];
  }
}

// The general route, a workgroup per document.  pass 0: cnt[d]; pass 1: the
// delta nodes from koff[d] on.
__global__ __launch_bounds__(1024) void k_sync_delta_gen(SyIn in, SyDelta a, int pass, uint32_t *cnt,
                                                        const uint32_t *koff) {
  __shared__ uint64_t hv[1024];
  __shared__ uint32_t wtot[16];
  const uint32_t d = blockIdx.x, tid = threadIdx.x;
  const uint32_t S = 1u << in.site_bits, smask = S - 1, shift = in.site_shift;
  const uint32_t b0 = in.off[d], n = in.off[d + 1] - b0;
  if (tid < S) hv[tid] = a.have[((uint64_t)d << in.site_bits) + tid];
  __syncthreads();
  uint32_t run = pass ? koff[d] : 0u;
  for (uint64_t i0 = 0; i0 < n; i0 += 1024) {
    const uint64_t i = i0 + tid;
    bool in_delta = false;
    if (i < n) {
      const uint64_t x = in.id[b0 + i];
      in_delta = x > hv[(uint32_t)(x >> shift) & smask];
    }
    uint32_t tot;
    const uint32_t pos = run + block_exscan<1024>(in_delta ? 1u : 0u, wtot, &tot);
    if (pass && in_delta) sy_gather(in, a, b0, (uint32_t)i, pos);
    run += tot;
  }
  if (!pass && tid == 0) cnt[d] = run;
}

// ahead[d] (zero when the kernel starts) += the ranks of d with have > ver.
__global__ __launch_bounds__(256) void k_sync_ahead(const uint64_t *have, const uint64_t *ver, uint64_t words,
                                                   uint32_t site_bits, uint32_t *ahead) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < words && have[e] > ver[e]) atomicAdd(&ahead[e >> site_bits], 1u);
}

namespace {

// After the checks: the ids (uploaded for a host call, which leaves the stream
// idle) and the layout on the device.
int sync_prepare(cw_ctx *c, const cw_sync_batch *b, bool dev, const SyShape &sh, SyIn *in) {
  HIPCHK(c, hipSetDevice(c->device));
  *in = SyIn{b->id_key, nullptr, (uint32_t)sh.D, (uint32_t)sh.N, b->ts_shift, b->site_shift, b->site_bits};
  if (!sh.D) return 0;
  if (!dev) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (upload(c, "sy_id", b->id_key, (size_t)sh.N * 8, &in->id)) return -1;
  }
  const char *name = "sy_off";
  bool miss;
  return device_layout(c, c->sync.docs, sh.D, b->doc_offsets, nullptr, &name, nullptr, &in->off, &miss);
}

size_t sy_row_bytes(uint32_t docs, uint32_t site_bits, uint32_t per_rank) {
  return (size_t)docs * per_rank << site_bits;
}

// ver / ylen / max_ts (device; ylen and max_ts optional) of a batch with D > 0.
int sync_version_run(cw_ctx *c, const SyShape &sh, const SyIn &in, SyRoute route, uint64_t *ver, uint32_t *ylen,
                     uint64_t *max_ts) {
  const uint64_t D = sh.D, N = sh.N, words = D << in.site_bits;
  // per node its id; per rank its maximum and count out; per document its two offsets and max_ts
  const double bytes = (double)N * 8 + (double)words * (ylen ? 12 : 8) + (double)D * (max_ts ? 16 : 8);
  if (route == SY_ROUTE_GENERAL || N == 0) {
    HIPCHK(c, hipMemsetAsync(ver, 0, words * 8, c->stream));
    if (ylen) HIPCHK(c, hipMemsetAsync(ylen, 0, words * 4, c->stream));
    if (max_ts) HIPCHK(c, hipMemsetAsync(max_ts, 0, D * 8, c->stream));
    if (N == 0) return 0;
    const uint64_t tiles = (N + SY_TILE - 1) / SY_TILE;
    if (!grid_ok(tiles, SY_TILE_NT)) return fail(c, "batch too large for one dispatch");
    {
      // ... the table zeroed first, and its nonzero words read and written again by the atomics
      Launch L(c, "sync_ver_tiled", bytes + (double)words * (ylen ? 12 : 8));
      hipLaunchKernelGGL(k_sync_version_tiled, dim3((uint32_t)tiles), dim3(SY_TILE_NT), 0, c->stream, in, ver, ylen,
                         max_ts);
    }
    return check_launch(c, "sync_ver_tiled");
  }
  if (route == SY_ROUTE_WAVE) {
    constexpr uint32_t DG = SY_WAVE_NT / 64;
    const uint64_t blocks = (D + DG - 1) / DG;
    if (!grid_ok(blocks, SY_WAVE_NT)) return fail(c, "batch too large for one dispatch");
    {
      Launch L(c, "sync_ver_wave", bytes);
      hipLaunchKernelGGL((k_sync_version<SY_WAVE_NT, 64>), dim3((uint32_t)blocks), dim3(SY_WAVE_NT),
                         sy_row_bytes(DG, in.site_bits, 12), c->stream, in, ver, ylen, max_ts);
    }
    return check_launch(c, "sync_ver_wave");
  }
  if (!grid_ok(D, SY_WG_NT)) return fail(c, "batch too large for one dispatch");
  {
    Launch L(c, "sync_ver_wg", bytes);
    hipLaunchKernelGGL((k_sync_version<SY_WG_NT, SY_WG_NT>), dim3((uint32_t)D), dim3(SY_WG_NT),
                       sy_row_bytes(1, in.site_bits, 12), c->stream, in, ver, ylen, max_ts);
  }
  return check_launch(c, "sync_ver_wg");
}

int version_impl(cw_ctx *c, const cw_sync_batch *b, cw_version_result *r, int memspace) {
  if (!b || !r) return fail(c, "null batch/result");
  if (memspace != CW_MEM_HOST && memspace != CW_MEM_DEVICE) return fail(c, "bad memspace");
  const bool dev = memspace == CW_MEM_DEVICE;
  char err[256];
  SyShape sh;
  SyIn in;
  if (sync_check_batch(b, &sh, err, sizeof err)) return fail(c, "%s", err);
  if (sh.D && !r->ver) return fail(c, "ver is required");
  if (sync_prepare(c, b, dev, sh, &in)) return -1;
  const uint64_t D = sh.D, words = D << b->site_bits;
  if (!D) return 0;
  uint64_t *ver = r->ver, *mts = r->max_ts;
  uint32_t *ylen = r->yarn_len;
  if (!dev) {
    ver = scratch_t<uint64_t>(c, "sy_over", words);
    ylen = r->yarn_len ? scratch_t<uint32_t>(c, "sy_oylen", words) : nullptr;
    mts = r->max_ts ? scratch_t<uint64_t>(c, "sy_omax", D) : nullptr;
    if (!ver || (r->yarn_len && !ylen) || (r->max_ts && !mts)) return fail(c, "out of device memory (host-mode staging)");
  }
  if (sync_version_run(c, sh, in, sync_route(sh.largest, c->sync_wave, c->sync_fused), ver, ylen, mts)) return -1;
  if (!dev) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(r->ver, ver, words * 8, hipMemcpyDeviceToHost));
    if (ylen) HIPCHK(c, hipMemcpy(r->yarn_len, ylen, words * 4, hipMemcpyDeviceToHost));
    if (mts) HIPCHK(c, hipMemcpy(r->max_ts, mts, D * 8, hipMemcpyDeviceToHost));
  } else if (!c->async) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return c->prof ? collect_prof(c) : 0;
}

int delta_impl(cw_ctx *c, const cw_sync_batch *b, const uint64_t *have, cw_delta_result *r, int memspace) {
  if (!b || !r) return fail(c, "null batch/result");
  if (!have) return fail(c, "null have");
  if (memspace != CW_MEM_HOST && memspace != CW_MEM_DEVICE) return fail(c, "bad memspace");
  const bool dev = memspace == CW_MEM_DEVICE;
  if (!r->delta_offsets) return fail(c, "delta_offsets is required (host memory)");
  char err[256];
  SyShape sh;
  SyIn in;
  if (sync_check_batch(b, &sh, err, sizeof err) || sync_check_pairing(b, r, err, sizeof err))
    return fail(c, "%s", err);
  if (sh.N && !r->delta_src) return fail(c, "null delta_src");
  if (sync_prepare(c, b, dev, sh, &in)) return -1;
  const uint64_t D = sh.D, N = sh.N, words = D << b->site_bits;
  if (!D || !N) {  // no nodes: no delta; a have word above 0 is ahead of an empty document
    for (uint64_t d = 0; d <= D; d++) r->delta_offsets[d] = 0;
    if (!D || !r->ahead) return 0;
  }
  SyDelta a{have, b->cause, b->kind, b->cause_is_id, r->delta_src, r->delta_id, r->delta_cause, r->delta_kind,
            r->delta_cause_is_id, r->ahead, nullptr};
  if (!dev) {  // uploads (the stream is idle: sync_prepare), and the outputs staged
    if (upload(c, "sy_have", have, (size_t)words * 8, &a.have)) return -1;
    if (a.cause && upload(c, "sy_cause", b->cause, (size_t)N * 8, &a.cause)) return -1;
    if (a.kind && upload(c, "sy_kind", b->kind, (size_t)N, &a.kind)) return -1;
    if (a.cii && upload(c, "sy_cii", b->cause_is_id, (size_t)N, &a.cii)) return -1;
    a.o_src = scratch_t<uint32_t>(c, "sy_osrc", N);
    a.o_id = r->delta_id ? scratch_t<uint64_t>(c, "sy_oid", N) : nullptr;
    a.o_cause = a.cause ? scratch_t<uint64_t>(c, "sy_oca", N) : nullptr;
    a.o_kind = a.kind ? scratch_t<uint8_t>(c, "sy_okd", N) : nullptr;
    a.o_cii = a.cii ? scratch_t<uint8_t>(c, "sy_oci", N) : nullptr;
    a.ahead = r->ahead ? scratch_t<uint32_t>(c, "sy_oahead", D) : nullptr;
    if (!a.o_src || (r->delta_id && !a.o_id) || (a.cause && !a.o_cause) || (a.kind && !a.o_kind) ||
        (a.cii && !a.o_cii) || (r->ahead && !a.ahead))
      return fail(c, "out of device memory (host-mode staging)");
  }
  const SyRoute route = N ? sync_route(sh.largest, c->sync_wave, c->sync_fused) : SY_ROUTE_GENERAL;
  // per delta node: its source index out, and each gathered column in and out
  const double per_delta = 4 + (a.o_id ? 16 : 0) + (a.o_cause ? 16 : 0) + (a.o_kind ? 2 : 0) + (a.o_cii ? 2 : 0);
  uint64_t *ko = r->delta_offsets;
  if (route == SY_ROUTE_GENERAL) {
    if (a.ahead) {  // the version, then the ranks above it
      uint64_t *ver = scratch_t<uint64_t>(c, "sy_ver", words);
      if (!ver) return fail(c, "out of device memory (delta)");
      if (sync_version_run(c, sh, in, SY_ROUTE_GENERAL, ver, nullptr, nullptr)) return -1;
      HIPCHK(c, hipMemsetAsync(a.ahead, 0, D * 4, c->stream));
      const uint64_t blocks = (words + 255) / 256;
      {
        Launch L(c, "sync_ahead", (double)words * 16 + (double)D * 4);
        hipLaunchKernelGGL(k_sync_ahead, dim3((uint32_t)blocks), dim3(256), 0, c->stream, a.have, ver, words,
                           in.site_bits, a.ahead);
      }
      if (check_launch(c, "sync_ahead")) return -1;
    }
    if (N) {
      if (!grid_ok(D, 1024)) return fail(c, "batch too large for one dispatch");
      uint32_t *kcnt = scratch_t<uint32_t>(c, "sy_kcnt", D + 1), *koff = scratch_t<uint32_t>(c, "sy_koff", D + 1);
      if (!kcnt || !koff) return fail(c, "out of device memory (delta)");
      auto pass = [&](const char *stat, int p, double bytes) {
        {
          Launch L(c, stat, bytes);
          hipLaunchKernelGGL(k_sync_delta_gen, dim3((uint32_t)D), dim3(1024), 0, c->stream, in, a, p, kcnt, koff);
        }
        return check_launch(c, stat);
      };
      // per node its id, per rank its have word, per document its offsets and count
      const double bytes = (double)N * 8 + (double)words * 8 + (double)D * 12;
      if (pass("sync_delta_count", 0, bytes)) return -1;
      if (scan_counts(c, kcnt, D, ko, koff)) return -1;
      if (pass("sync_delta_write", 1, bytes + (double)ko[D] * per_delta)) return -1;
    }
  } else {
    const bool wave = route == SY_ROUTE_WAVE;
    constexpr uint32_t DG = SY_WAVE_NT / 64;
    const uint64_t blocks = wave ? (D + DG - 1) / DG : D;
    if (!grid_ok(blocks, wave ? SY_WAVE_NT : SY_WG_NT)) return fail(c, "batch too large for one dispatch");
    a.o_off = scratch_t<uint64_t>(c, "sy_doff", D + 1);
    if (!a.o_off) return fail(c, "out of device memory (delta)");
    uint32_t epoch;
    unsigned long long *lb = lookback_words(c, c->sync.lb, "sy_lb", (uint32_t)blocks, 1, &epoch);
    if (!lb) return -1;
    const uint32_t rows = a.ahead ? 16 : 8;
    const char *stat = wave ? "sync_delta_wave" : "sync_delta_wg";
    size_t rec = NO_REC;
    {
      // per node its id and its bit of the bitmap; per rank its have word; per
      // document its offsets, its delta offset and ahead; the delta nodes join
      // once the count is known
      Launch L(c, stat, (double)N * 8.125 + (double)words * 8 + (double)D * (16 + (a.ahead ? 4 : 0)), nullptr, &rec);
      if (wave)
        hipLaunchKernelGGL((k_sync_delta<SY_WAVE_NT, 64, SY_WAVE_WORDS>), dim3((uint32_t)blocks), dim3(SY_WAVE_NT),
                           sy_row_bytes(DG, in.site_bits, rows), c->stream, in, a, lb, epoch);
      else
        hipLaunchKernelGGL((k_sync_delta<SY_WG_NT, SY_WG_NT, SY_WG_WORDS>), dim3((uint32_t)blocks), dim3(SY_WG_NT),
                           sy_row_bytes(1, in.site_bits, rows), c->stream, in, a, lb, epoch);
    }
    if (check_launch(c, stat)) return -1;
    // the call's one wait: the offsets
    HIPCHK(c, hipMemcpyAsync(ko, a.o_off, (D + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (rec < c->pending.size()) c->pending[rec].bytes += (double)ko[D] * per_delta;
  }
  const uint64_t P = ko[D];
  if (P > N) return fail(c, "internal: delta past N");
  if (!dev) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (P) {
      HIPCHK(c, hipMemcpy(r->delta_src, a.o_src, P * 4, hipMemcpyDeviceToHost));
      if (a.o_id) HIPCHK(c, hipMemcpy(r->delta_id, a.o_id, P * 8, hipMemcpyDeviceToHost));
      if (a.o_cause) HIPCHK(c, hipMemcpy(r->delta_cause, a.o_cause, P * 8, hipMemcpyDeviceToHost));
      if (a.o_kind) HIPCHK(c, hipMemcpy(r->delta_kind, a.o_kind, P, hipMemcpyDeviceToHost));
      if (a.o_cii) HIPCHK(c, hipMemcpy(r->delta_cause_is_id, a.o_cii, P, hipMemcpyDeviceToHost));
    }
    if (a.ahead) HIPCHK(c, hipMemcpy(r->ahead, a.ahead, D * 4, hipMemcpyDeviceToHost));
  } else if (!c->async) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return c->prof ? collect_prof(c) : 0;
}

}  // namespace
