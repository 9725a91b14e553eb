// renderbase.hip -- cw_render_bases (include/causeweave_render_bases.h): cb->edn
// (base/core.cljc:83-96) over the entry table of a batch of documents: every
// base's root collection with its refs resolved, as a depth-first token stream.
// Included by causeweave.hip after invert.hip (in_doc_of, in_put_words, iv_scan,
// lookback.h).
//
// The flattening is a preorder over a forest of documents of any depth; it is
// ranked as a linked list of 2 * n_docs events, not walked level by level.
//
// k_rb_roots, a thread a base: the root's claim; rootbase[root] = the base.
// k_rb_link, tiles of RB_TILE = 8,192 entries: claims[target] += 1 for every ref
//   entry with a target < n_docs.
// k_rb_compact, the same tiles (a launch of its own: every claim must have
//   landed): the TREE REFS (target claimed once) balloted into the bitmap tbits
//   and numbered in entry order by the decoupled look-back; item[k].x = the
//   entry of tree ref k, kidx[target] = k, par[target] = the entry's document.
//   The children of a document are then the contiguous items [crank[d],
//   crank[d + 1]).  A ref to a document claimed twice marks its document shared.
// k_rb_bound, a thread a document boundary: crank[d] = the tree refs before
//   entry ent_offsets[d] (tile_base + the bits below it in its tile).
// k_rb_tour, a thread a document: its two events, 2d = OPEN and 2d + 1 = CLOSE,
//   each with its successor and the tokens from it up to the successor:
//     OPEN d  -> OPEN(first child c)     1 + pe[c] - ent_offsets[d]
//             -> CLOSE d (no children)   1 + the entries of d
//     CLOSE c -> OPEN(next sibling c')   pe[c'] - pe[c]
//             -> CLOSE(parent p)         ent_offsets[p + 1] - pe[c]
//   (pe[c]: the entry that refers to c.)  CLOSE of a root, of an unclaimed
//   document or of one claimed twice is terminal: its own successor, distance 0.
// k_rb_jump, ceil(log2(2 * n_docs)) rounds of pointer jumping over the 8-byte
//   words successor << 32 | distance, ping-pong buffered.  A chain has at most
//   2 * n_docs events, so every event that ends in a terminal has reached it; an
//   isolated cycle of once-claimed documents just keeps turning and is told
//   apart afterwards: the event it stops at is not the CLOSE of a base's root.
// k_rb_docs, a thread a document: dist(event) = distance + 1 tokens from the
//   event to the end of its stream; size[d] = dist(OPEN d) - dist(CLOSE d) + 1;
//   start[d] = size[root] - dist(OPEN d); the base that reaches d; a shared
//   document flags its base.
// k_rb_size, a thread a base: base_status, the base's tokens (0 when flagged),
//   base_tok_offsets by a block scan and the look-back.
// k_rb_place, a thread a document: doc_base, doc_open, the OPEN and CLOSE
//   tokens; item[kidx[d]].y = the position of d's CLOSE.
// k_rb_emit, the entry tiles again: entry e of a reached, unflagged document,
//   not a tree ref, goes to item[k - 1].y + (e - item[k - 1].x) when tree ref
//   k - 1, the last one before e, lies in e's document (the tokens after that
//   child's CLOSE), and to doc_open + 1 + (e - ent_offsets[d]) otherwise.  k is
//   the rank from tbits, as in k_rb_compact; no scan of subtree sizes is needed.
//   Every entry needs its document: 256 threads search the offsets once for the
//   first entry of each bitmap word, and an entry searches only between its
//   word's document and the next word's (mostly the same one).
//
// Nothing is read or written outside the caller's arrays: a target is checked
// against n_docs before claims[] is touched, a base against n_bases, and every
// token position against the capacity E + 2 * n_docs before it is written.

constexpr uint32_t RB_NT = 256;
constexpr uint32_t RB_TILE = RB_NT * 32;  // entries a tile, a bitmap word a thread
constexpr uint32_t RB_NONE = 0xFFFFFFFFu;

struct RbArgs {
  uint32_t E, D, G, tiles, cap;  // cap = E + 2 * D
  const uint32_t *off;           // device [D + 1]
  const uint32_t *ref, *root;
  // per document
  uint32_t *claims, *shared;     // (0)
  uint32_t *kidx;                // (RB_NONE)
  uint32_t *rootbase, *par, *dbase, *size, *start, *dopen;
  uint32_t *crank;               // [D + 1]
  // per tile
  uint32_t *tbits;               // [256 * tiles]
  uint32_t *tile_base;           // [tiles + 1]
  uint2 *item;                   // [min(E, D)] x: the tree ref's entry, y: the position of its child's CLOSE
  unsigned long long *jump;      // [2 * D] the ranked events
  uint32_t *flag;                // [G] (0)
  uint64_t *boff;                // [G + 1]
  unsigned long long *lb;
  uint32_t epoch;
  // outputs
  uint8_t *o_kind;
  uint32_t *o_doc, *o_entry, *o_status, *o_doc_base, *o_doc_open;
};

__global__ __launch_bounds__(256) void k_rb_roots(RbArgs a) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= a.G) return;
  const uint32_t t = a.root[g];
  if (t >= a.D) return;
  atomicAdd(a.claims + t, 1u);  // (no returned value)
  a.rootbase[t] = g;            // (read only where this claim is the only one)
}

__global__ __launch_bounds__(RB_NT) void k_rb_link(RbArgs a) {
  const uint32_t g0 = blockIdx.x * RB_TILE;  // (blockIdx.x < tiles: g0 < E)
  const uint32_t cnt = a.E - g0 < RB_TILE ? a.E - g0 : RB_TILE;
#pragma unroll 4
  for (uint32_t it = 0; it < 32; it++) {
    const uint32_t x = it * RB_NT + threadIdx.x;
    if (x >= cnt) break;
    const uint32_t r = a.ref[g0 + x];
    if (r < a.D) atomicAdd(a.claims + r, 1u);  // (no returned value)
  }
}

// (8 waves a SIMD: at most 64 VGPRs)
__global__ __launch_bounds__(RB_NT, 8) void k_rb_compact(RbArgs a) {
  __shared__ uint32_t fw[RB_NT], wpre[RB_NT], tmp[RB_NT / 64];
  __shared__ uint32_t s_dlo, s_dhi, s_base;

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t t = blockIdx.x, g0 = t * RB_TILE;  // (t < tiles: g0 < E)
  const uint32_t cnt = a.E - g0 < RB_TILE ? a.E - g0 : RB_TILE;
  fw[tid] = 0;
  if (tid == 0) s_dlo = in_doc_of(a.off, 0u, a.D - 1, g0);
  if (tid == 64) s_dhi = in_doc_of(a.off, 0u, a.D - 1, g0 + cnt - 1);
  __syncthreads();
  // 1. the tree refs' bits
  for (uint32_t it = 0; it < 32 && it * RB_NT < cnt; it++) {
    const uint32_t x = it * RB_NT + tid;
    const uint32_t r = x < cnt ? a.ref[g0 + x] : RB_NONE;
    const bool tree = r < a.D && a.claims[r] == 1;
    in_put_words(fw, __ballot(tree), x, lane);
  }
  __syncthreads();
  // 2. the words' counts scanned, the tile's first rank by the look-back
  const uint32_t word = fw[tid];
  uint32_t total;
  wpre[tid] = iv_scan<RB_NT>((uint32_t)__popc(word), tmp, &total);
  if (tid < 64) {
    if (tid == 0) lb_publish(a.lb, t, a.epoch, total);
    const uint32_t base = lb_exclusive(a.lb, t, a.epoch, total);
    if (tid == 0) {
      s_base = base;
      a.tile_base[t] = base;
      if (t + 1 == a.tiles) a.tile_base[a.tiles] = base + total;
    }
  }
  a.tbits[(g0 >> 5) + tid] = word;
  __syncthreads();
  // 3. the items, in entry order; the documents with a ref to a shared one
  const uint32_t base = s_base, d0 = s_dlo, dhi = s_dhi, h_end = a.off[d0 + 1];
  const uint32_t items = a.E < a.D ? a.E : a.D;
  for (uint32_t it = 0; it < 32 && it * RB_NT < cnt; it++) {
    const uint32_t x = it * RB_NT + tid, e = g0 + x;
    if (x >= cnt) continue;
    const uint32_t r = a.ref[e];
    if (r >= a.D) continue;
    const uint32_t d = e < h_end ? d0 : in_doc_of(a.off, d0 + 1, dhi, e);
    const uint32_t w = fw[x >> 5];
    if ((w >> (x & 31)) & 1u) {
      const uint32_t k = base + wpre[x >> 5] + (uint32_t)__popc(w & ((1u << (x & 31)) - 1));
      if (k < items) {  // (a tree ref has a target of its own: there are at most min(E, D))
        a.item[k] = make_uint2(e, RB_NONE);
        a.kidx[r] = k;
        a.par[r] = d;
      }
    } else if (a.claims[r] >= 2) {
      a.shared[d] = 1u;
    }
  }
}

__global__ __launch_bounds__(256) void k_rb_bound(RbArgs a) {
  const uint32_t d = blockIdx.x * 256 + threadIdx.x;
  if (d > a.D) return;
  uint32_t g = a.off[d];
  if (g > a.E) g = a.E;
  const uint32_t t = g / RB_TILE < a.tiles ? g / RB_TILE : a.tiles - 1;  // (tiles >= 1)
  // (g <= E: every word counted lies inside tbits, and the bits at or past E are 0)
  const uint32_t w1 = g >> 5;
  uint32_t r = a.tile_base[t];
  for (uint32_t w = t * RB_NT; w < w1; w++) r += (uint32_t)__popc(a.tbits[w]);
  if (g & 31) r += (uint32_t)__popc(a.tbits[w1] & ((1u << (g & 31)) - 1));
  a.crank[d] = r;
}

__device__ __forceinline__ unsigned long long rb_word(uint32_t succ, uint32_t dist) {
  return ((unsigned long long)succ << 32) | dist;
}

// A tree ref's target (< D by k_rb_compact's test; checked again: the caller's
// array may change under the call, which must then still stay inside its arrays).
__device__ __forceinline__ uint32_t rb_child(const RbArgs &a, uint32_t e, uint32_t self) {
  const uint32_t c = e < a.E ? a.ref[e] : RB_NONE;
  return c < a.D ? c : self;
}

__global__ __launch_bounds__(256) void k_rb_tour(RbArgs a) {
  const uint32_t d = blockIdx.x * 256 + threadIdx.x;
  if (d >= a.D) return;
  const uint32_t o0 = a.off[d], o1 = a.off[d + 1], c0 = a.crank[d], c1 = a.crank[d + 1];
  const uint32_t items = a.E < a.D ? a.E : a.D;
  unsigned long long op = rb_word(2 * d + 1, 1 + o1 - o0), cl = rb_word(2 * d + 1, 0);
  if (c0 < c1 && c1 <= items) {
    const uint32_t e = a.item[c0].x;
    op = rb_word(2 * rb_child(a, e, d), 1 + e - o0);
  }
  const uint32_t k = a.kidx[d];
  if (a.claims[d] == 1 && k < items) {
    const uint32_t p = a.par[d], e = a.item[k].x;
    if (p < a.D) {
      if (k + 1 < a.crank[p + 1] && k + 1 < items) {
        const uint32_t e2 = a.item[k + 1].x;
        cl = rb_word(2 * rb_child(a, e2, d), e2 - e);
      } else {
        cl = rb_word(2 * p + 1, a.off[p + 1] - e);
      }
    }
  }
  a.jump[2 * (size_t)d] = op;
  a.jump[2 * (size_t)d + 1] = cl;
}

__global__ __launch_bounds__(256) void k_rb_jump(const unsigned long long *__restrict__ in,
                                                 unsigned long long *__restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long v = in[i];
  const uint32_t s = (uint32_t)(v >> 32);
  const unsigned long long u = s < n ? in[s] : rb_word(s, 0);
  out[i] = (u & 0xFFFFFFFF00000000ull) | (uint32_t)((uint32_t)v + (uint32_t)u);
}

__global__ __launch_bounds__(256) void k_rb_docs(RbArgs a) {
  const uint32_t d = blockIdx.x * 256 + threadIdx.x;
  if (d >= a.D) return;
  const unsigned long long vo = a.jump[2 * (size_t)d], vc = a.jump[2 * (size_t)d + 1];
  const uint32_t s = (uint32_t)(vo >> 32), dist_o = (uint32_t)vo + 1, dist_c = (uint32_t)vc + 1;
  uint32_t g = RB_NONE, st = 0;
  if ((s & 1u) && (s >> 1) < a.D) {  // ended at a CLOSE: the root of a base, if claimed by it alone
    const uint32_t r = s >> 1;
    if (a.claims[r] == 1 && a.kidx[r] == RB_NONE) {
      g = a.rootbase[r];
      st = (uint32_t)a.jump[2 * (size_t)r] + 1 - dist_o;
    }
  }
  if (g >= a.G) g = RB_NONE;
  a.dbase[d] = g;
  a.size[d] = dist_o - dist_c + 1;
  a.start[d] = st;
  if (g != RB_NONE && a.shared[d]) a.flag[g] = 1u;
}

__global__ __launch_bounds__(256) void k_rb_size(RbArgs a) {
  __shared__ uint32_t tmp[4], s_base;
  const uint32_t tid = threadIdx.x, g = blockIdx.x * 256 + tid;
  uint32_t sz = 0;
  if (g < a.G) {
    const uint32_t t = a.root[g];
    uint32_t st = 0;
    if (t < a.D) {
      if (a.claims[t] >= 2 || a.flag[g]) st = (uint32_t)CW_STATUS_REF_SHARED;
      else sz = (uint32_t)a.jump[2 * (size_t)t] + 1;
    }
    if (st) a.flag[g] = 1u;
    a.o_status[g] = st;
  }
  uint32_t total;
  const uint32_t ex = iv_scan<256>(sz, tmp, &total);
  if (tid < 64) {
    if (tid == 0) lb_publish(a.lb, blockIdx.x, a.epoch, total);
    const uint32_t base = lb_exclusive(a.lb, blockIdx.x, a.epoch, total);
    if (tid == 0) s_base = base;
  }
  __syncthreads();
  if (g < a.G) {
    a.boff[g] = (uint64_t)s_base + ex;
    if (g == a.G - 1) a.boff[a.G] = (uint64_t)s_base + total;
  }
}

__global__ __launch_bounds__(256) void k_rb_place(RbArgs a) {
  const uint32_t d = blockIdx.x * 256 + threadIdx.x;
  if (d >= a.D) return;
  uint32_t g = a.dbase[d], po = RB_NONE;
  if (g != RB_NONE && a.flag[g]) g = RB_NONE;
  if (g != RB_NONE) {
    po = (uint32_t)a.boff[g] + a.start[d];
    const uint32_t pc = po + a.size[d] - 1, k = a.kidx[d];
    const uint32_t items = a.E < a.D ? a.E : a.D;
    uint32_t via = RB_NONE;
    if (k < items) {
      via = a.item[k].x;
      a.item[k].y = pc;
    }
    if (a.o_kind && po < pc && pc < a.cap) {
      a.o_kind[po] = (uint8_t)CW_TOK_OPEN;
      a.o_doc[po] = d;
      a.o_entry[po] = via;
      a.o_kind[pc] = (uint8_t)CW_TOK_CLOSE;
      a.o_doc[pc] = d;
      a.o_entry[pc] = via;
    }
  }
  a.dopen[d] = po;
  if (a.o_doc_base) a.o_doc_base[d] = g;
  if (a.o_doc_open) a.o_doc_open[d] = po;
}

// (8 waves a SIMD: at most 64 VGPRs)
__global__ __launch_bounds__(RB_NT, 8) void k_rb_emit(RbArgs a) {
  __shared__ uint32_t fw[RB_NT], wpre[RB_NT], wdoc[RB_NT + 1], tmp[RB_NT / 64];
  __shared__ uint32_t s_dlo, s_dhi;

  const uint32_t tid = threadIdx.x;
  const uint32_t t = blockIdx.x, g0 = t * RB_TILE;  // (t < tiles: g0 < E)
  const uint32_t cnt = a.E - g0 < RB_TILE ? a.E - g0 : RB_TILE;
  if (tid == 0) s_dlo = in_doc_of(a.off, 0u, a.D - 1, g0);
  if (tid == 64) s_dhi = in_doc_of(a.off, 0u, a.D - 1, g0 + cnt - 1);
  const uint32_t word = a.tbits[(g0 >> 5) + tid];
  fw[tid] = word;
  uint32_t total;
  wpre[tid] = iv_scan<RB_NT>((uint32_t)__popc(word), tmp, &total);
  __syncthreads();
  const uint32_t base = a.tile_base[t], d0 = s_dlo, dhi = s_dhi;
  // the document of each bitmap word's first entry: an entry's own is then one
  // of the few between its word's and the next word's
  wdoc[tid] = tid * 32 < cnt ? in_doc_of(a.off, d0, dhi, g0 + tid * 32) : dhi;
  if (tid == 0) wdoc[RB_NT] = dhi;
  __syncthreads();
  const uint32_t h_off = a.off[d0], h_end = a.off[d0 + 1], h_open = a.dopen[d0], h_c0 = a.crank[d0];
  const uint32_t items = a.E < a.D ? a.E : a.D;
  for (uint32_t it = 0; it < 32 && it * RB_NT < cnt; it++) {
    const uint32_t x = it * RB_NT + tid, e = g0 + x;
    if (x >= cnt) continue;
    const uint32_t w = fw[x >> 5];
    if ((w >> (x & 31)) & 1u) continue;  // a tree ref: its child's OPEN stands here
    uint32_t d = d0, o = h_off, po = h_open, c0 = h_c0;
    if (e >= h_end) {
      const uint32_t lo = wdoc[x >> 5], hi = wdoc[(x >> 5) + 1];
      d = lo == hi ? lo : in_doc_of(a.off, lo, hi, e);
      o = a.off[d];
      po = a.dopen[d];
      c0 = a.crank[d];
    }
    if (po == RB_NONE) continue;  // not reached, or its base is flagged
    const uint32_t r = a.ref[e];
    if (r < a.D) continue;  // (a ref to a shared document: the base is flagged; never here)
    const uint32_t k = base + wpre[x >> 5] + (uint32_t)__popc(w & ((1u << (x & 31)) - 1));
    uint32_t pos = po + 1 + (e - o);
    if (k > c0 && k <= items) {  // after the CLOSE of the child before it
      const uint2 pv = a.item[k - 1];
      pos = pv.y + (e - pv.x);
    }
    if (pos < a.cap) {
      a.o_kind[pos] = (uint8_t)(r == RB_NONE ? CW_TOK_LEAF : CW_TOK_NIL);
      a.o_doc[pos] = d;
      a.o_entry[pos] = e;
    }
  }
}

namespace {

int render_bases_impl(cw_ctx *c, const cw_render_bases_batch *b, cw_render_bases_result *r, int memspace) {
  if (!b || !r) return fail(c, "null batch/result");
  if (memspace != CW_MEM_HOST && memspace != CW_MEM_DEVICE) return fail(c, "bad memspace");
  const bool dev = memspace == CW_MEM_DEVICE;
  const uint64_t D = b->n_docs, G = b->n_bases;
  if (D >= 0x7FFFFFFFull) return fail(c, "batch too large: %llu documents (limit 2^31-1)", (unsigned long long)D);
  if (G >= 0xFFFFFFFFull) return fail(c, "batch too large: %llu bases (limit 2^32-1)", (unsigned long long)G);
  if (!b->ent_offsets || !r->base_tok_offsets)
    return fail(c, "ent_offsets and base_tok_offsets are required (host memory)");
  if (check_doc_offsets(c, b->ent_offsets, D, 0, 0)) return -1;
  const uint64_t E = b->ent_offsets[D];
  if (E + 2 * D >= 0xFFFFFFFFull)
    return fail(c, "batch too large: %llu entries + 2 * %llu documents (limit 2^32-1)", (unsigned long long)E,
                (unsigned long long)D);
  if (E && !b->ent_ref) return fail(c, "null ent_ref");
  if (G && (!b->root_doc || !r->base_status)) return fail(c, "null root_doc or base_status");
  const int given = (r->tok_kind != nullptr) + (r->tok_doc != nullptr) + (r->tok_entry != nullptr);
  if (given != 0 && given != 3) return fail(c, "tok_kind, tok_doc and tok_entry go together");
  const bool tokens = given == 3;
  HIPCHK(c, hipSetDevice(c->device));
  if (D == 0 || G == 0) {  // no base has a root: no tokens
    for (uint64_t g = 0; g <= G; g++) r->base_tok_offsets[g] = 0;
    if (!dev) {
      if (G) memset(r->base_status, 0, G * 4);
      if (r->doc_base && D) memset(r->doc_base, 0xFF, D * 4);
      return 0;
    }
    if (G) HIPCHK(c, hipMemsetAsync(r->base_status, 0, G * 4, c->stream));
    if (r->doc_base && D) HIPCHK(c, hipMemsetAsync(r->doc_base, 0xFF, D * 4, c->stream));
    if (!c->async) HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  }
  auto &st = c->rbase;
  const uint32_t tiles = (uint32_t)((E + RB_TILE - 1) / RB_TILE);
  const uint32_t dblocks = (uint32_t)((D + 256) / 256), gblocks = (uint32_t)((G + 255) / 256);
  const uint32_t eblocks = (uint32_t)((2 * D + 255) / 256);
  if (!grid_ok(tiles, RB_NT) || !grid_ok(eblocks, 256) || !grid_ok(gblocks, 256))
    return fail(c, "batch too large for one dispatch");

  RbArgs a{};
  a.E = (uint32_t)E;
  a.D = (uint32_t)D;
  a.G = (uint32_t)G;
  a.tiles = tiles;
  a.cap = (uint32_t)(E + 2 * D);
  a.ref = b->ent_ref;
  a.root = b->root_doc;
  a.o_kind = r->tok_kind;
  a.o_doc = r->tok_doc;
  a.o_entry = r->tok_entry;
  a.o_status = r->base_status;
  a.o_doc_base = r->doc_base;
  a.o_doc_open = r->doc_open;
  if (!dev) {  // uploads, and the outputs staged
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (upload(c, "rb_ref", b->ent_ref, (size_t)E * 4, &a.ref) || upload(c, "rb_root", b->root_doc, (size_t)G * 4, &a.root))
      return -1;
    a.o_status = scratch_t<uint32_t>(c, "rb_ost", G);
    a.o_doc_base = r->doc_base ? scratch_t<uint32_t>(c, "rb_odb", D) : nullptr;
    a.o_doc_open = r->doc_open ? scratch_t<uint32_t>(c, "rb_odo", D) : nullptr;
    if (tokens) {
      a.o_kind = scratch_t<uint8_t>(c, "rb_okd", a.cap);
      a.o_doc = scratch_t<uint32_t>(c, "rb_odc", a.cap);
      a.o_entry = scratch_t<uint32_t>(c, "rb_oen", a.cap);
    }
    if (!a.o_status || (r->doc_base && !a.o_doc_base) || (r->doc_open && !a.o_doc_open) ||
        (tokens && (!a.o_kind || !a.o_doc || !a.o_entry)))
      return fail(c, "out of device memory (host-mode staging)");
  }

  // the layout on the device, cached while it repeats
  const char *n_off = "rb_off";
  bool miss;
  if (device_layout(c, st.docs, D, b->ent_offsets, nullptr, &n_off, nullptr, &a.off, &miss)) return -1;
  // per document: claims, shared (zero), kidx (none), rootbase, par, dbase, size, start, dopen, crank
  uint32_t *dz = scratch_t<uint32_t>(c, "rb_doc", 10 * D + 1);
  const size_t items = (size_t)std::min(E, D);
  a.flag = scratch_t<uint32_t>(c, "rb_flag", G);
  a.boff = scratch_t<uint64_t>(c, "rb_boff", G + 1);
  a.tbits = scratch_t<uint32_t>(c, "rb_tbits", (size_t)tiles * RB_NT);
  a.tile_base = scratch_t<uint32_t>(c, "rb_tbase", (size_t)tiles + 1);
  a.item = scratch_t<uint2>(c, "rb_item", items);
  unsigned long long *jA = scratch_t<unsigned long long>(c, "rb_jA", 2 * D);
  unsigned long long *jB = scratch_t<unsigned long long>(c, "rb_jB", 2 * D);
  if (!dz || !a.flag || !a.boff || !a.tbits || !a.tile_base || !a.item || !jA || !jB)
    return fail(c, "out of device memory (render bases)");
  a.claims = dz;
  a.shared = dz + D;
  a.kidx = dz + 2 * D;
  a.rootbase = dz + 3 * D;
  a.par = dz + 4 * D;
  a.dbase = dz + 5 * D;
  a.size = dz + 6 * D;
  a.start = dz + 7 * D;
  a.dopen = dz + 8 * D;
  a.crank = dz + 9 * D;
  HIPCHK(c, hipMemsetAsync(dz, 0, 2 * D * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(a.kidx, 0xFF, D * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(a.flag, 0, G * 4, c->stream));

  {
    Launch L(c, "k_rb_roots", (double)G * 12);
    hipLaunchKernelGGL(k_rb_roots, dim3(gblocks), dim3(256), 0, c->stream, a);
  }
  if (check_launch(c, "k_rb_roots")) return -1;
  if (tiles) {
    {
      // per entry its ref in; per ref entry a claim
      Launch L(c, "k_rb_link", (double)E * 4);
      hipLaunchKernelGGL(k_rb_link, dim3(tiles), dim3(RB_NT), 0, c->stream, a);
    }
    if (check_launch(c, "k_rb_link")) return -1;
    a.lb = lookback_words(c, st.lb_tiles, "rb_lbt", tiles, 1, &a.epoch);
    if (!a.lb) return -1;
    {
      // per entry its ref in and its bit out; per tree ref (at most a document each) its item, kidx and par out
      Launch L(c, "k_rb_compact", (double)E * 4.125 + (double)items * 20 + (double)tiles * 24);
      hipLaunchKernelGGL(k_rb_compact, dim3(tiles), dim3(RB_NT), 0, c->stream, a);
    }
    if (check_launch(c, "k_rb_compact")) return -1;
    {
      // a boundary's offset and tile base in, on average half a tile of bitmap words, its rank out
      Launch L(c, "k_rb_bound", (double)(D + 1) * (12.0 + RB_TILE / 16.0));
      hipLaunchKernelGGL(k_rb_bound, dim3(dblocks), dim3(256), 0, c->stream, a);
    }
    if (check_launch(c, "k_rb_bound")) return -1;
  } else {
    HIPCHK(c, hipMemsetAsync(a.crank, 0, (D + 1) * 4, c->stream));
  }
  a.jump = jA;
  {
    Launch L(c, "k_rb_tour", (double)D * 60);
    hipLaunchKernelGGL(k_rb_tour, dim3(dblocks), dim3(256), 0, c->stream, a);
  }
  if (check_launch(c, "k_rb_tour")) return -1;
  const uint32_t rounds = std::max(1u, ceil_log2(2 * D));
  for (uint32_t k = 0; k < rounds; k++) {
    unsigned long long *out = a.jump == jA ? jB : jA;
    {
      Launch L(c, "k_rb_jump", (double)D * 2 * 24);
      hipLaunchKernelGGL(k_rb_jump, dim3(eblocks), dim3(256), 0, c->stream, a.jump, out, (uint32_t)(2 * D));
    }
    if (check_launch(c, "k_rb_jump")) return -1;
    a.jump = out;
  }
  {
    Launch L(c, "k_rb_docs", (double)D * 48);
    hipLaunchKernelGGL(k_rb_docs, dim3(dblocks), dim3(256), 0, c->stream, a);
  }
  if (check_launch(c, "k_rb_docs")) return -1;
  a.lb = lookback_words(c, st.lb_bases, "rb_lbb", gblocks, 1, &a.epoch);
  if (!a.lb) return -1;
  {
    Launch L(c, "k_rb_size", (double)G * 32);
    hipLaunchKernelGGL(k_rb_size, dim3(gblocks), dim3(256), 0, c->stream, a);
  }
  if (check_launch(c, "k_rb_size")) return -1;
  {
    // per document its base, offset, size and start in, dopen out; the optional outputs and its two tokens
    Launch L(c, "k_rb_place", (double)D * (36 + (tokens ? 18 : 0) + (a.o_doc_base ? 4 : 0) + (a.o_doc_open ? 4 : 0)));
    hipLaunchKernelGGL(k_rb_place, dim3(dblocks), dim3(256), 0, c->stream, a);
  }
  if (check_launch(c, "k_rb_place")) return -1;
  size_t rec_emit = NO_REC;
  if (tokens && tiles) {
    {
      // per entry its bit and ref in; per token (added below) 9 bytes out
      Launch L(c, "k_rb_emit", (double)E * 4.125 + (double)tiles * 24, nullptr, &rec_emit);
      hipLaunchKernelGGL(k_rb_emit, dim3(tiles), dim3(RB_NT), 0, c->stream, a);
    }
    if (check_launch(c, "k_rb_emit")) return -1;
  }
  // the call's one wait: the base offsets
  HIPCHK(c, hipMemcpyAsync(r->base_tok_offsets, a.boff, (G + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t T = r->base_tok_offsets[G];
  if (T > a.cap) return fail(c, "internal: tokens past the capacity");
  if (rec_emit != NO_REC && rec_emit < c->pending.size()) c->pending[rec_emit].bytes += (double)T * 9;
  if (!dev) {
    if (tokens && T) {
      HIPCHK(c, hipMemcpy(r->tok_kind, a.o_kind, T, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(r->tok_doc, a.o_doc, T * 4, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(r->tok_entry, a.o_entry, T * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(c, hipMemcpy(r->base_status, a.o_status, G * 4, hipMemcpyDeviceToHost));
    if (r->doc_base) HIPCHK(c, hipMemcpy(r->doc_base, a.o_doc_base, D * 4, hipMemcpyDeviceToHost));
    if (r->doc_open) HIPCHK(c, hipMemcpy(r->doc_open, a.o_doc_open, D * 4, hipMemcpyDeviceToHost));
  }
  return c->prof ? collect_prof(c) : 0;
}

}  // namespace
