// render.hip -- cw_render_lists / cw_render_maps: the last stage of every
// pipeline, causal-list->edn / causal-list->list / count (list.cljc:57-77) and
// causal-map->edn / causal-map->list / count- (map.cljc:68-73, 94-109) on the
// result arrays of a weave, merge or weft.  Included by causeweave.hip after
// listweft.hip (lookback.h).
//
// One tiled stream compaction with two predicates.  Lists: position g of the
// global weave is emitted iff bit g of visible_bits is set.  Maps: key weave s
// is emitted iff seg_active[s] >= 0.  The output position of g is rank(g), the
// number of emitted positions below g: document boundaries do not enter the
// scan, so one kernel serves one giant list, 10^4 documents of 50,001 nodes
// and 10^6 documents of a few nodes alike.
//
// k_render<KIND, VAL>, a workgroup of RN_NT = 256 threads per tile of RN_TILE =
// 8,192 positions (256 bitmap words, one per thread):
//   1. the tile index from an atomic ticket (one word zeroed per call), not
//      from blockIdx.x: a workgroup that holds ticket t waits only for tickets
//      below t, whose holders already run, whatever the dispatch order;
//   2. the tile's bitmap words into LDS.  Lists: the caller's words, the bits
//      at positions >= N masked off.  Maps: each wave ballots the predicate of
//      64 consecutive key weaves; the words also go to a scratch bitmap, so
//      that k_render_offsets ranks both kinds the same way; seg_coll is
//      checked here (ascending, < n_colls);
//   3. a block scan of the words' popcounts; the tile's count published and
//      its exclusive base taken by the decoupled look-back (lookback.h, the
//      stage's own words and epochs); tile_base[t] kept for k_render_offsets;
//   4. the expansion, position-major: thread i takes positions i, i + 256, ...
//      so weave_perm (seg_active, seg_key, seg_coll) is read with coalesced
//      loads, RN_U of them in flight, and an emitted position's output index is
//      base + prefix[word] + popcount(bits below).  Consecutive emitted
//      positions of a wave have consecutive indices: the stores of
//      rendered_src and of rendered_value (its natural width) coalesce as far
//      as the bitmap is dense.  (A word's bits expanded by the thread that
//      owns the word would read weave_perm at a stride of 128 B a lane.)
//   5. the value gather, the one random access: an emitted position's document
//      is the tile's first one, tile_doc[t] (its two offsets are read once a
//      workgroup), or is searched in doc_off[tile_doc[t] + 1 .. tile_doc[t + 1]]
//      (the documents that meet the tile: one or two at 50,001 nodes, thousands
//      of tiny or empty ones at worst); src is checked against the document's
//      size and an out-of-range one gets value 0.  Maps read seg_coll[s]
//      instead.  A round of RN_U positions runs in phases (index loads,
//      documents, value loads, stores), so the gathers of a round are in
//      flight together instead of one dependent chain a position.
//
// The tile: 256 words = one word a thread, so the block scan is one pass and
// the LDS is 2 KiB; at 256 threads and <= 64 VGPRs eight workgroups share a
// CU (32 waves), which hides the look-back's round trip of one workgroup
// behind the expansion of the others.  8,192 positions make 32 KiB of
// weave_perm a workgroup, 32 positions a thread; a 2 * 10^9-node list has
// 262,144 tiles, and a tile's count (<= 8,192) and every prefix (< 2^32) fit
// the look-back word's 46 count bits.
//
// k_render_offsets, one thread per document boundary: rank(doc_off[d]) =
// tile_base[t] + the set bits of tile t below it (at most 256 words
// re-counted).  Maps: the boundary of collection c is lower_bound(seg_coll, c).

constexpr uint32_t RN_NT = 256;
constexpr uint32_t RN_TILE = RN_NT * 32;  // positions a tile
constexpr uint32_t RN_U = 4;              // loads in flight in the expansion

enum { RN_LIST32 = 0, RN_LIST16 = 1, RN_MAP = 2 };

struct RnArgs {
  uint32_t n;       // positions: N, or n_segs
  uint32_t n_docs;  // documents / collections
  // lists
  const void *perm;      // [n] u32 or u16
  const uint32_t *bits;  // [(n + 31) / 32]
  // maps
  const int64_t *active;     // [n]
  const uint32_t *seg_coll;  // [n]
  const uint64_t *seg_key;   // [n]
  uint32_t *mbits;           // scratch bitmap, [(n + 31) / 32] (written)
  // the value column
  const uint32_t *doc_off;   // device [n_docs + 1]
  const uint32_t *tile_doc;  // device [tiles + 1] (lists)
  const void *value;
  // outputs
  uint32_t *out_src;
  uint64_t *out_key;
  void *out_val;
  // the scan
  uint32_t *tile_base;     // [tiles]
  uint32_t *ctl;           // [0] the ticket, [1] maps: seg_coll out of order
  unsigned long long *lb;  // [tiles]
  uint32_t epoch;
};

template <int VAL>
struct RnVal {
  using T = uint8_t;
};
template <>
struct RnVal<2> {
  using T = uint16_t;
};
template <>
struct RnVal<4> {
  using T = uint32_t;
};
template <>
struct RnVal<8> {
  using T = uint64_t;
};

// (8 workgroups a CU: at most 64 VGPRs)
template <int KIND, int VAL>
__global__ __launch_bounds__(RN_NT, 8) void k_render(RnArgs a) {
  constexpr uint32_t NW = RN_NT / 64;
  using VT = typename RnVal<VAL>::T;
  __shared__ uint32_t words[RN_NT];
  __shared__ uint32_t prefix[RN_NT];
  __shared__ uint32_t wtot[NW];
  __shared__ uint32_t s_tile, s_base;

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  // 1. the ticket
  if (tid == 0) s_tile = atomicAdd(a.ctl, 1u);
  __syncthreads();
  const uint32_t t = s_tile;
  const uint32_t g0 = t * RN_TILE;  // (t < tiles: g0 < n)
  const uint32_t n = a.n;
  const uint32_t cnt = n - g0 < RN_TILE ? n - g0 : RN_TILE;  // positions of this tile

  // 2. the bitmap words
  if (KIND != RN_MAP) {
    uint32_t x = 0;
    const uint32_t p0 = tid * 32;
    if (p0 < cnt) {
      x = a.bits[(g0 >> 5) + tid];
      if (cnt - p0 < 32) x &= (1u << (cnt - p0)) - 1;
    }
    words[tid] = x;
  } else {
#pragma unroll 4
    for (uint32_t it = 0; it < 32; it++) {
      const uint32_t i = it * RN_NT + tid;
      bool on = false;
      if (i < cnt) {
        const uint32_t s = g0 + i;
        on = a.active[s] >= 0;
        const uint32_t c = a.seg_coll[s];
        if (c >= a.n_docs || (s > 0 && a.seg_coll[s - 1] > c)) atomicOr(a.ctl + 1, 1u);  // (no returned value)
      }
      const uint64_t m = __ballot(on);
      if (lane < 2) {
        const uint32_t x = (uint32_t)(m >> (32 * lane));
        const uint32_t w = ((i - lane) >> 5) + lane;  // (i - lane: the wave's first position)
        words[w] = x;
        if (w * 32 < cnt) a.mbits[(g0 >> 5) + w] = x;
      }
    }
  }
  __syncthreads();

  // 3. emitted positions before each word; the tile's base
  uint32_t tot;
  prefix[tid] = block_exscan<RN_NT>((uint32_t)__popc(words[tid]), wtot, &tot);
  if (tid == 0) lb_publish(a.lb, t, a.epoch, tot);
  if (tid < 64) {
    const uint32_t b = lb_exclusive(a.lb, t, a.epoch, tot);
    if (tid == 0) {
      s_base = b;
      a.tile_base[t] = b;
    }
  }
  __syncthreads();  // (prefix[] is complete here as well)
  const uint32_t base = s_base;
  if (!a.out_src && !a.out_key && !VAL) return;  // the count-only call

  // 4. the expansion; 5. the value gather.  Each round in phases -- the index
  // loads of RN_U positions, their documents, their values, the stores -- so
  // that the loads of a phase are in flight together.
  uint32_t dlo = 0, dhi = 0, off0 = 0, off1 = 0;
  if (KIND != RN_MAP && VAL) {  // the tile's first document: most positions' own
    dlo = a.tile_doc[t];
    dhi = a.tile_doc[t + 1];
    off0 = a.doc_off[dlo];
    off1 = a.doc_off[dlo + 1];
  }
  for (uint32_t it0 = 0; it0 < 32 && it0 * RN_NT < cnt; it0 += RN_U) {
    bool on[RN_U];
    uint32_t src[RN_U], coll[RN_U], o[RN_U], b0[RN_U], sz[RN_U];
    uint64_t key[RN_U];
    VT v[RN_U];
#pragma unroll
    for (uint32_t u = 0; u < RN_U; u++) {
      const uint32_t i = (it0 + u) * RN_NT + tid;
      const uint32_t wd = words[i >> 5];
      on[u] = (wd >> (i & 31)) & 1u;  // (0 past the tile's positions)
      o[u] = base + prefix[i >> 5] + (uint32_t)__popc(wd & ((1u << (i & 31)) - 1));
      src[u] = coll[u] = 0;
      key[u] = 0;
      if (on[u]) {
        const uint32_t g = g0 + i;
        if (KIND == RN_LIST32) src[u] = static_cast<const uint32_t *>(a.perm)[g];
        if (KIND == RN_LIST16) src[u] = static_cast<const uint16_t *>(a.perm)[g];
        if (KIND == RN_MAP) {
          // (an active index past 32 bits is out of every collection's range)
          const uint64_t ac = (uint64_t)a.active[g];
          src[u] = ac > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)ac;
          if (a.out_key) key[u] = a.seg_key[g];
          if (VAL) coll[u] = a.seg_coll[g];
        }
      }
    }
    if (VAL) {
#pragma unroll
      for (uint32_t u = 0; u < RN_U; u++) {  // the document's first node and its size
        b0[u] = sz[u] = 0;
        if (!on[u]) continue;
        if (KIND == RN_MAP) {
          if (coll[u] < a.n_docs) {
            b0[u] = a.doc_off[coll[u]];
            const uint32_t b1 = a.doc_off[coll[u] + 1];
            sz[u] = b1 >= b0[u] ? b1 - b0[u] : 0u;
          }
        } else {
          const uint32_t g = g0 + (it0 + u) * RN_NT + tid;
          if (g < off1) {
            b0[u] = off0;
            sz[u] = off1 - off0;
          } else {  // the last document of [dlo + 1, dhi] that starts at or below g
            uint32_t lo = dlo + 1, hi = dhi;
            while (lo < hi) {
              const uint32_t mid = lo + ((hi - lo + 1) >> 1);
              if (a.doc_off[mid] <= g) lo = mid;
              else hi = mid - 1;
            }
            b0[u] = a.doc_off[lo];
            sz[u] = a.doc_off[lo + 1] - b0[u];
          }
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < RN_U; u++) {
        v[u] = 0;
        if (on[u] && src[u] < sz[u]) v[u] = static_cast<const VT *>(a.value)[(uint64_t)b0[u] + src[u]];
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < RN_U; u++) {
      if (!on[u]) continue;
      if (a.out_src) a.out_src[o[u]] = src[u];
      if (KIND == RN_MAP && a.out_key) a.out_key[o[u]] = key[u];
      if (VAL) static_cast<VT *>(a.out_val)[o[u]] = v[u];
    }
  }
}

// One thread per boundary d <= n_docs: out[d] = rank(boundary d), the boundary
// being doc_off[d] (lists) or lower_bound(seg_coll, d) (maps: seg_coll given).
// out[n_docs + 1] = ctl[1] (maps: seg_coll was out of order).
__global__ __launch_bounds__(256) void k_render_offsets(const uint32_t *__restrict__ doc_off,
                                                        const uint32_t *__restrict__ seg_coll,
                                                        const uint32_t *__restrict__ bits,
                                                        const uint32_t *__restrict__ tile_base, uint32_t n,
                                                        uint32_t n_docs, const uint32_t *__restrict__ ctl,
                                                        uint64_t *__restrict__ out) {
  const uint32_t d = blockIdx.x * 256 + threadIdx.x;
  if (d > n_docs) return;
  if (d == 0) out[n_docs + 1] = ctl[1];
  uint32_t g;
  if (seg_coll) {
    uint32_t lo = 0, hi = n;  // the first s with seg_coll[s] >= d
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (seg_coll[mid] < d) lo = mid + 1;
      else hi = mid;
    }
    g = lo;
  } else {
    g = doc_off[d];
    if (g > n) g = n;
  }
  if (n == 0) {
    out[d] = 0;
    return;
  }
  const uint32_t tiles = (n + RN_TILE - 1) / RN_TILE;
  const uint32_t t = g / RN_TILE < tiles ? g / RN_TILE : tiles - 1;
  // (g <= n: every bit counted lies below n)
  const uint32_t w0 = t * (RN_TILE / 32), w1 = g >> 5;
  uint32_t r = tile_base[t];
  uint32_t w = w0;
  for (; w + 4 <= w1; w += 4) {
    const uint32_t x0 = bits[w], x1 = bits[w + 1], x2 = bits[w + 2], x3 = bits[w + 3];
    r += __popc(x0) + __popc(x1) + __popc(x2) + __popc(x3);
  }
  for (; w < w1; w++) r += __popc(bits[w]);
  if (g & 31) r += __popc(bits[w1] & ((1u << (g & 31)) - 1));
  out[d] = r;
}

namespace {

// What render_impl needs of either call, every array in device memory.
struct RnHost {
  int kind;             // RN_LIST32 / RN_LIST16 / RN_MAP
  uint32_t value_size;  // 0, 1, 2, 4, 8
  uint64_t n, n_docs;
  RnArgs a;             // (tile_base, ctl, lb, epoch, mbits, tile_doc: filled in by render_impl)
  const uint64_t *off;  // HOST [n_docs + 1] or nullptr (maps without a value column)
  uint64_t *out_off;    // HOST [n_docs + 1]
};

template <int KIND>
void render_launch(cw_ctx *c, const RnHost &h, uint32_t tiles) {
  const dim3 g(tiles), b(RN_NT);
  switch (h.value_size) {
    case 0: hipLaunchKernelGGL((k_render<KIND, 0>), g, b, 0, c->stream, h.a); break;
    case 1: hipLaunchKernelGGL((k_render<KIND, 1>), g, b, 0, c->stream, h.a); break;
    case 2: hipLaunchKernelGGL((k_render<KIND, 2>), g, b, 0, c->stream, h.a); break;
    case 4: hipLaunchKernelGGL((k_render<KIND, 4>), g, b, 0, c->stream, h.a); break;
    default: hipLaunchKernelGGL((k_render<KIND, 8>), g, b, 0, c->stream, h.a); break;
  }
}

// The layout on the device, cached in the context while the offsets repeat:
// doc_off (u32[D + 1]) and, for lists, tile_doc[t] = the last document that
// starts at or below position t * RN_TILE (u32[tiles + 1]).
int render_layout(cw_ctx *c, DevLayout &ly, const char *n_off, const char *n_td, const uint64_t *off,
                  uint64_t D, uint32_t tiles, bool want_td, const uint32_t **doff, const uint32_t **tdoc) {
  uint32_t *q = want_td ? scratch_t<uint32_t>(c, n_td, (size_t)tiles + 1) : nullptr;
  if (want_td && !q) return fail(c, "out of device memory (render offsets)");
  bool miss;
  if (device_layout(c, ly, D, off, nullptr, &n_off, q, doff, &miss)) return -1;
  if (miss && want_td) {
    std::vector<uint32_t> h_td((size_t)tiles + 1);
    uint64_t d = 0;
    for (uint32_t t = 0; t <= tiles; t++) {
      const uint64_t g = (uint64_t)t * RN_TILE;
      while (d + 1 < D && off[d + 1] <= g) d++;
      h_td[t] = (uint32_t)d;
    }
    if (hipMemcpy(q, h_td.data(), h_td.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
      ly.off.clear();
      return fail(c, "hipMemcpy (%s)", n_td);
    }
  }
  *tdoc = q;
  return 0;
}

// The two kernels and the one wait: the offsets (and, for maps, the order
// word) come back in one copy.  Returns 0, -1 on error; *bad_order (maps).
int render_impl(cw_ctx *c, RnHost &h, bool *bad_order) {
  const bool maps = h.kind == RN_MAP;
  const uint64_t D = h.n_docs, n = h.n;
  auto &rs = c->render;
  *bad_order = false;
  if (n == 0) {
    for (uint64_t d = 0; d <= D; d++) h.out_off[d] = 0;
    return 0;
  }
  const uint32_t tiles = (uint32_t)((n + RN_TILE - 1) / RN_TILE);
  if (!grid_ok(tiles, RN_NT) || !grid_ok((D + 256) / 256, 256)) return fail(c, "batch too large for one dispatch");
  const bool val = h.value_size != 0;
  // (lists: k_render_offsets reads doc_off as well, and tile_doc goes along whether
  // or not this call has a value column, so that calls with and without one
  // share the cached layout)
  if (!maps || val) {
    if (render_layout(c, maps ? rs.maps : rs.lists, maps ? "rn_moff" : "rn_off", "rn_tdoc", h.off, D, tiles,
                      !maps, &h.a.doc_off, &h.a.tile_doc))
      return -1;
  }
  uint32_t *tb = scratch_t<uint32_t>(c, "rn_tbase", tiles), *ctl = scratch_t<uint32_t>(c, "rn_ctl", 4);
  uint64_t *d_off = scratch_t<uint64_t>(c, "rn_ooff", D + 2);
  uint32_t *mb = maps ? scratch_t<uint32_t>(c, "rn_mbits", (n + 31) / 32) : nullptr;
  if (!tb || !ctl || !d_off || (maps && !mb)) return fail(c, "out of device memory (render)");
  uint32_t epoch;
  unsigned long long *lb = lookback_words(c, rs.lb, "rn_lb", tiles, 1, &epoch);
  if (!lb) return -1;
  HIPCHK(c, hipMemsetAsync(ctl, 0, 16, c->stream));  // the ticket and the order word
  h.a.n = (uint32_t)n;
  h.a.n_docs = (uint32_t)D;
  h.a.mbits = mb;
  h.a.tile_base = tb;
  h.a.ctl = ctl;
  h.a.lb = lb;
  h.a.epoch = epoch;
  const char *stat = maps ? "render_maps" : "render_lists";
  size_t rec = NO_REC;
  {
    // per position its bit (lists) or its active word, collection and, with
    // entry_key, key (maps: the bit is written instead); the emitted nodes'
    // share joins once the count is known
    const double per = maps ? 12.0 + 0.125 : 0.125;
    Launch L(c, stat, (double)n * per, nullptr, &rec);
    if (h.kind == RN_LIST32) render_launch<RN_LIST32>(c, h, tiles);
    else if (h.kind == RN_LIST16) render_launch<RN_LIST16>(c, h, tiles);
    else render_launch<RN_MAP>(c, h, tiles);
  }
  if (check_launch(c, stat)) return -1;
  {
    // a boundary's offset word in (lists), its tile's base and on average
    // half a tile of bitmap words; 8 B out
    Launch L(c, "render_offsets", (double)(D + 1) * (16.0 + RN_TILE / 16.0));
    hipLaunchKernelGGL(k_render_offsets, dim3((uint32_t)((D + 256) / 256)), dim3(256), 0, c->stream,
                       maps ? nullptr : h.a.doc_off, maps ? h.a.seg_coll : nullptr, maps ? mb : h.a.bits, tb,
                       (uint32_t)n, (uint32_t)D, ctl, d_off);
  }
  if (check_launch(c, "render_offsets")) return -1;
  // the call's one device-to-host copy and its one wait
  std::vector<uint64_t> tmp;
  uint64_t *dst = h.out_off;
  if (maps) {
    tmp.resize(D + 2);
    dst = tmp.data();
  }
  HIPCHK(c, hipMemcpyAsync(dst, d_off, (D + 1 + (maps ? 1 : 0)) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (maps) {
    if (tmp[D + 1]) {
      *bad_order = true;
      return 0;
    }
    memcpy(h.out_off, tmp.data(), (D + 1) * 8);
  }
  if (rec < c->pending.size()) {
    // per emitted node: its perm word in (4 or 2 B; maps: nothing more), src
    // and value out, the value gathered; maps: the key out
    const double R = (double)h.out_off[D];
    const bool any = h.a.out_src || h.a.out_key || val;
    double per = 0;
    if (any && !maps) per += h.kind == RN_LIST16 ? 2 : 4;
    if (h.a.out_src) per += 4;
    if (h.a.out_key) per += 8;
    per += 2.0 * h.value_size;
    c->pending[rec].bytes += R * per;
  }
  return 0;
}

bool render_value_size_ok(uint32_t v) { return v == 0 || v == 1 || v == 2 || v == 4 || v == 8; }

int render_lists_impl(cw_ctx *c, const cw_render_batch *b, cw_render_result *r, int memspace) {
  if (!b || !r) return fail(c, "null batch/result");
  if (memspace != CW_MEM_HOST && memspace != CW_MEM_DEVICE) return fail(c, "bad memspace");
  const bool dev = memspace == CW_MEM_DEVICE;
  const uint64_t D = b->n_docs;
  uint64_t largest = 0;
  if (check_doc_offsets(c, b->doc_offsets, D, 0, 0, &largest)) return -1;
  if (!r->rendered_offsets) return fail(c, "rendered_offsets is required (host memory)");
  if (!render_value_size_ok(b->value_size)) return fail(c, "value_size must be 0, 1, 2, 4 or 8");
  if (b->value_size && (b->value == nullptr) != (r->rendered_value == nullptr))
    return fail(c, "value and rendered_value go together");
  if (b->perm16 > 1) return fail(c, "perm16 must be 0 or 1");
  if (b->perm16 && largest >= 65536) return fail(c, "perm16 needs every document below 65,536 nodes");
  const uint64_t N = b->doc_offsets[D];
  const uint32_t vs = (b->value_size && b->value) ? b->value_size : 0;
  const bool expand = r->rendered_src || vs;
  if (N && (!b->visible_bits || (expand && !b->weave_perm))) return fail(c, "null input arrays");
  HIPCHK(c, hipSetDevice(c->device));
  RnHost h{};
  h.kind = b->perm16 ? RN_LIST16 : RN_LIST32;
  h.value_size = vs;
  h.n = N;
  h.n_docs = D;
  h.off = b->doc_offsets;
  h.out_off = r->rendered_offsets;
  h.a.perm = b->weave_perm;
  h.a.bits = b->visible_bits;
  h.a.value = vs ? b->value : nullptr;
  h.a.out_src = r->rendered_src;
  h.a.out_val = vs ? r->rendered_value : nullptr;
  const size_t pw = b->perm16 ? 2 : 4;
  if (!dev && N) {  // uploads, and the outputs staged
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint8_t *pp = nullptr, *vv = nullptr;
    if (upload(c, "rs_bits", b->visible_bits, (size_t)((N + 31) / 32) * 4, &h.a.bits)) return -1;
    if (expand) {
      if (upload(c, "rs_perm", static_cast<const uint8_t *>(b->weave_perm), (size_t)N * pw, &pp)) return -1;
      h.a.perm = pp;
    }
    if (vs) {
      if (upload(c, "rs_val", static_cast<const uint8_t *>(b->value), (size_t)N * vs, &vv)) return -1;
      h.a.value = vv;
      h.a.out_val = scratch(c, "rs_oval", (size_t)N * vs);
    }
    if (r->rendered_src) h.a.out_src = scratch_t<uint32_t>(c, "rs_osrc", N);
    if ((vs && !h.a.out_val) || (r->rendered_src && !h.a.out_src))
      return fail(c, "out of device memory (host-mode staging)");
  }
  bool bad;
  if (render_impl(c, h, &bad)) return -1;
  if (!dev && N) {  // (the stream is idle: render_impl's wait)
    const uint64_t R = r->rendered_offsets[D];
    if (R && r->rendered_src) HIPCHK(c, hipMemcpy(r->rendered_src, h.a.out_src, R * 4, hipMemcpyDeviceToHost));
    if (R && vs) HIPCHK(c, hipMemcpy(r->rendered_value, h.a.out_val, R * vs, hipMemcpyDeviceToHost));
  }
  return c->prof ? collect_prof(c) : 0;
}

int render_maps_impl(cw_ctx *c, const cw_map_render_batch *b, cw_map_render_result *r, int memspace) {
  if (!b || !r) return fail(c, "null batch/result");
  if (memspace != CW_MEM_HOST && memspace != CW_MEM_DEVICE) return fail(c, "bad memspace");
  const bool dev = memspace == CW_MEM_DEVICE;
  const uint64_t D = b->n_colls, S = b->n_segs;
  if (!r->entry_offsets) return fail(c, "entry_offsets is required (host memory)");
  if (!render_value_size_ok(b->value_size)) return fail(c, "value_size must be 0, 1, 2, 4 or 8");
  if (b->value_size && (b->value == nullptr) != (r->entry_value == nullptr))
    return fail(c, "value and entry_value go together");
  const uint32_t vs = (b->value_size && b->value) ? b->value_size : 0;
  if (S >= 0xFFFFFFFFull || D >= 0xFFFFFFFFull)
    return fail(c, "batch too large: n_segs=%llu (limit 2^32-1)", (unsigned long long)S);
  if (vs && check_doc_offsets(c, b->coll_offsets, D, 0, 0)) return -1;
  if (S && (!b->seg_coll || !b->seg_active || (r->entry_key && !b->seg_key))) return fail(c, "null input arrays");
  HIPCHK(c, hipSetDevice(c->device));
  RnHost h{};
  h.kind = RN_MAP;
  h.value_size = vs;
  h.n = S;
  h.n_docs = D;
  h.off = vs ? b->coll_offsets : nullptr;
  h.out_off = r->entry_offsets;
  h.a.active = b->seg_active;
  h.a.seg_coll = b->seg_coll;
  h.a.seg_key = b->seg_key;
  h.a.value = vs ? b->value : nullptr;
  h.a.out_src = r->entry_src;
  h.a.out_key = r->entry_key;
  h.a.out_val = vs ? r->entry_value : nullptr;
  if (!dev && S) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint8_t *vv = nullptr;
    if (upload(c, "rs_mcoll", b->seg_coll, (size_t)S * 4, &h.a.seg_coll) ||
        upload(c, "rs_mact", b->seg_active, (size_t)S * 8, &h.a.active))
      return -1;
    if (r->entry_key) {
      if (upload(c, "rs_mkey", b->seg_key, (size_t)S * 8, &h.a.seg_key)) return -1;
      h.a.out_key = scratch_t<uint64_t>(c, "rs_okey", S);
    }
    if (vs) {
      const uint64_t N = b->coll_offsets[D];
      if (upload(c, "rs_val", static_cast<const uint8_t *>(b->value), (size_t)N * vs, &vv)) return -1;
      h.a.value = vv;
      h.a.out_val = scratch(c, "rs_oval", (size_t)S * vs);
    }
    if (r->entry_src) h.a.out_src = scratch_t<uint32_t>(c, "rs_osrc", S);
    if ((vs && !h.a.out_val) || (r->entry_src && !h.a.out_src) || (r->entry_key && !h.a.out_key))
      return fail(c, "out of device memory (host-mode staging)");
  }
  bool bad;
  if (render_impl(c, h, &bad)) return -1;
  if (bad) return fail(c, "seg_coll is not ascending or names a collection >= n_colls");
  if (!dev && S) {
    const uint64_t R = r->entry_offsets[D];
    if (R && r->entry_src) HIPCHK(c, hipMemcpy(r->entry_src, h.a.out_src, R * 4, hipMemcpyDeviceToHost));
    if (R && r->entry_key) HIPCHK(c, hipMemcpy(r->entry_key, h.a.out_key, R * 8, hipMemcpyDeviceToHost));
    if (R && vs) HIPCHK(c, hipMemcpy(r->entry_value, h.a.out_val, R * vs, hipMemcpyDeviceToHost));
  }
  return c->prof ? collect_prof(c) : 0;
}

}  // namespace
