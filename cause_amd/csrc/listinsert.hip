// listinsert.hip -- cw_insert_lists (include/causeweave_insert.h): c.list/weave's
// 2/3-arity (list.cljc:29-34) over s/weave-node (shared.cljc:225-241) behind
// s/insert (shared.cljc:151-184), one transaction a document, without a
// reweave.  Included by causeweave.hip after render.hip (lookback.h).
//
// With nm the first tx node, nr = weave[i], and per weave position i
//   e1(i) = id(weave[i]) == cause(nm)          (asap at i + 1; only this shows that the cause exists)
//   e2(i) = id(nm) == cause(weave[i])          (asap at i)
//   nl(i) = !later(i)                          (weave-later?, shared.cljc:202-223)
// the place of the tx is  a = min(min{i + 1 : e1(i)}, min{i : e2(i)}),
// p = min{i >= a : nl(i)} or n.  One geometry serves every document size:
// workgroups of IN_NT = 256 threads over fixed tiles of IN_TILE = 8,192 global
// positions, 256 bitmap words, one a thread (render.hip's tile).
//
// e1, e2 and nl are properties of the NODE weave[i], not of the position, so
// they are computed in input order, where id, cause and kind stream in with
// coalesced loads, and only three bits a node are gathered through weave_perm.
// (Gathering id, cause and kind themselves through weave_perm, three random
// lines a position out of 850 KB a config-2 document with ~170 documents in
// flight, ran at 0.38 TB/s of algorithmic bytes, 28 ms for 5 * 10^8 nodes; a
// document's marks are 19 KB.)
//
// k_insert_mark, a tile of input positions:
//   1. the tile's first and last document by a search of doc_off (two threads);
//      the first one's offsets and first tx node are wave-uniform and serve most
//      positions, the other documents of a tile are searched per position;
//   2. id, cause and kind, IN_U positions in flight; nl, e1 and e2 balloted
//      into the marks array (words 3w .. 3w + 2: nodes 32w .. 32w + 31); an id
//      equal to nm's (found, same body) and an id equal to nm's cause (the
//      cause exists) go to the document's flags word, the ids' maximum to its
//      max word (the tile's first document: one atomicMax a
//      wave).
// k_insert_find, a tile of OLD weave positions:
//   1. the tile's documents, as above;
//   2. position-major (thread i takes positions i, i + 256, ...): weave_perm
//      with coalesced loads, then the node's marks gathered through it; e1, e2
//      and nl are balloted into three LDS bitmaps; an e1 or e2 hit (one a
//      document, as a rule) goes to the document's `a` word with atomicMin;
//   3. every asap position of the tile (e2, e1 shifted by one inside a document,
//      and the e1 of the position before the tile, read by one thread) scans
//      the nl bitmap forward to the end of its document or tile: the first hit
//      is a candidate for p, atomicMin into the document's `f` word.  Every
//      candidate is an nl index >= a, and the first nl index >= a inside a's
//      tile is among them;
//   4. tile_g[t] = the first nl index of the tile's first document inside the
//      tile: the candidates of the tiles after a's.
// k_insert_plan, a wave a document (16 documents a workgroup): the validation
// (shared.cljc:163-178), p = min(f, the first tile_g of the tiles after a's up
// to f's), the new size, max_ts over the old ids and the tx ids, the place of
// every tx node in the new yarn (a binary search of the old yarn by (site, id)),
// status, insert_pos, visible_count zeroed; the new offsets by a scan of the
// workgroup's 16 sizes and the decoupled look-back over the workgroups.
// k_insert_splice, a tile of NEW positions: weave_perm shifted around p, the
// visible words balloted from the old bits with p-1 .. p+k-1 recomputed by
// hide? (list.cljc:48-55), visible_count (the tile's first document: one
// atomicAdd a wave; the others per word), yarn_perm merged, the output columns.
//
// Nothing is read or written outside the caller's arrays whatever weave_perm
// and yarn_perm hold: an index >= the document's size is skipped.

constexpr uint32_t IN_NT = 256;
constexpr uint32_t IN_TILE = IN_NT * 32;  // positions a tile
constexpr uint32_t IN_U = 4;              // loads in flight a thread: k_insert_mark's columns, k_insert_find's gathers
constexpr uint32_t IN_NONE = 0xFFFFFFFFu;
constexpr uint32_t IN_PLAN_NT = 1024, IN_PLAN_DOCS = IN_PLAN_NT / 64;
constexpr uint32_t IN_FOUND = 1, IN_SAME = 2, IN_CAUSE = 4;  // flags word: nm's id, with nm's body; nm's cause

struct InArgs {
  uint32_t N, D;            // old nodes, documents
  const uint32_t *doc_off;  // device [D + 1]
  const uint32_t *tx_off;   // device [D + 1]
  const uint64_t *id, *cause;
  const uint8_t *kind;
  const uint64_t *value;
  const uint32_t *perm, *bits, *yarn;
  const uint64_t *tx_id, *tx_cause;
  const uint8_t *tx_kind;
  const uint64_t *tx_value;
  uint32_t ts_shift, site_shift, site_bits;
  // per document: a, f (0xFF..), max id, flags (0), p; per tile: tile_g; per tx node: its yarn place
  uint32_t *doc_a, *doc_f, *flags, *pos, *tile_g, *tx_rank;
  uint32_t *marks;  // [3 * 256 * tiles]: nl, e1, e2 words of 32 nodes, by input index
  unsigned long long *max_id;
  uint64_t *new_off;  // device [D + 1]
  unsigned long long *lb;
  uint32_t epoch;
  // outputs
  uint32_t *o_perm, *o_bits, *o_count, *o_status, *o_yarn, *o_pos;
  uint64_t *o_maxts, *o_id, *o_cause, *o_value;
  uint8_t *o_kind;
};

// The last document of [lo, hi] that starts at or below g (off[lo] <= g).
template <typename T>
__device__ __forceinline__ uint32_t in_doc_of(const T *off, uint32_t lo, uint32_t hi, uint32_t g) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (off[mid] <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// A wave's two bitmap words of one ballot: lanes 0 and 1 store them.
__device__ __forceinline__ void in_put_words(uint32_t *words, uint64_t m, uint32_t x, uint32_t lane) {
  if (lane < 2) words[((x - lane) >> 5) + lane] = (uint32_t)(m >> (32 * lane));  // (x - lane: the wave's first position)
}

// The three marks of the node at global input index gi: words 3w, 3w + 1, 3w + 2
// of `marks` hold the nl, e1 and e2 bits of nodes 32w .. 32w + 31.
__device__ __forceinline__ uint32_t in_marks(const uint32_t *marks, uint32_t gi) {
  const uint32_t *w = marks + (size_t)(gi >> 5) * 3;
  const uint32_t b = gi & 31;
  return ((w[0] >> b) & 1u) | (((w[1] >> b) & 1u) << 1) | (((w[2] >> b) & 1u) << 2);
}

// (8 waves a SIMD: at most 64 VGPRs)
__global__ __launch_bounds__(IN_NT, 8) void k_insert_mark(InArgs a) {
  __shared__ uint32_t s_dlo, s_dhi;

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t t = blockIdx.x, g0 = t * IN_TILE;  // (t < tiles: g0 < N)
  const uint32_t cnt = a.N - g0 < IN_TILE ? a.N - g0 : IN_TILE;
  if (tid == 0) s_dlo = in_doc_of(a.doc_off, 0u, a.D - 1, g0);
  if (tid == 64) s_dhi = in_doc_of(a.doc_off, 0u, a.D - 1, g0 + cnt - 1);
  __syncthreads();
  const uint32_t d0 = s_dlo, dhi = s_dhi;
  const uint32_t h_end = a.doc_off[d0 + 1];
  const uint32_t h_to = a.tx_off[d0], h_k = a.tx_off[d0 + 1] - h_to;
  uint64_t h_id = 0, h_cause = 0;
  uint8_t h_kind = 0;
  if (h_k) {
    h_id = a.tx_id[h_to];
    h_cause = a.tx_cause[h_to];
    h_kind = a.tx_kind[h_to];
  }
  uint64_t hmax = 0;
  for (uint32_t it0 = 0; it0 < 32 && it0 * IN_NT < cnt; it0 += IN_U) {
    uint64_t idv[IN_U], cav[IN_U];
    uint8_t kdv[IN_U];
#pragma unroll
    for (uint32_t u = 0; u < IN_U; u++) {
      const uint32_t x = (it0 + u) * IN_NT + tid;
      idv[u] = cav[u] = 0;
      kdv[u] = 0;
      if (x < cnt) {
        idv[u] = a.id[g0 + x];
        cav[u] = a.cause[g0 + x];
        kdv[u] = a.kind[g0 + x];
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < IN_U; u++) {
      const uint32_t x = (it0 + u) * IN_NT + tid, g = g0 + x;
      const bool in = x < cnt;
      uint32_t d = d0, to = h_to, k = h_k;
      uint64_t mid = h_id, mca = h_cause;
      uint8_t mkd = h_kind;
      if (in && g >= h_end) {
        d = in_doc_of(a.doc_off, d0 + 1, dhi, g);
        to = a.tx_off[d];
        k = a.tx_off[d + 1] - to;
        if (k) {
          mid = a.tx_id[to];
          mca = a.tx_cause[to];
          mkd = a.tx_kind[to];
        }
      }
      if (in && a.o_maxts) {
        if (d == d0) hmax = idv[u] > hmax ? idv[u] : hmax;
        else atomicMax(a.max_id + d, (unsigned long long)idv[u]);  // (no returned value)
      }
      const bool on = in && k != 0;
      const bool sr = is_special(kdv[u]), sm = is_special(mkd), lt = mid < idv[u];
      const bool later = (sr && mid != cav[u] && (!sm || lt)) || (lt && (!sm || sr));
      const bool e1 = on && idv[u] == mca;
      if (on && idv[u] == mid) {
        const bool same = cav[u] == mca && kdv[u] == mkd && (!a.value || a.value[g] == a.tx_value[to]);
        atomicOr(a.flags + d, IN_FOUND | (same ? IN_SAME : 0u));
      }
      if (e1) atomicOr(a.flags + d, IN_CAUSE);  // (an e2 hit alone, an orphan that names nm, is no cause)
      const uint64_t m_nl = __ballot(on && !later), m_e1 = __ballot(e1), m_e2 = __ballot(on && cav[u] == mid);
      if (lane < 2) {  // (x - lane: the wave's first position)
        uint32_t *w = a.marks + (size_t)((g0 >> 5) + ((x - lane) >> 5) + lane) * 3;
        w[0] = (uint32_t)(m_nl >> (32 * lane));
        w[1] = (uint32_t)(m_e1 >> (32 * lane));
        w[2] = (uint32_t)(m_e2 >> (32 * lane));
      }
    }
  }
  if (a.o_maxts) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t y = __shfl_xor(hmax, o, 64);
      hmax = y > hmax ? y : hmax;
    }
    if (lane == 0 && hmax) atomicMax(a.max_id + d0, (unsigned long long)hmax);
  }
}

// (8 waves a SIMD: at most 64 VGPRs)
__global__ __launch_bounds__(IN_NT, 8) void k_insert_find(InArgs a) {
  __shared__ uint32_t nlw[IN_NT], e1w[IN_NT], e2w[IN_NT];
  __shared__ uint32_t s_dlo, s_dhi, s_prev, s_g;

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t t = blockIdx.x, g0 = t * IN_TILE;  // (t < tiles: g0 < N)
  const uint32_t cnt = a.N - g0 < IN_TILE ? a.N - g0 : IN_TILE;
  // 1. the tile's documents
  nlw[tid] = e1w[tid] = e2w[tid] = 0;
  if (tid == 0) {
    s_dlo = in_doc_of(a.doc_off, 0u, a.D - 1, g0);
    s_prev = 0;
    s_g = IN_NONE;
  }
  if (tid == 64) s_dhi = in_doc_of(a.doc_off, 0u, a.D - 1, g0 + cnt - 1);
  __syncthreads();
  const uint32_t d0 = s_dlo, dhi = s_dhi;
  const uint32_t h_off = a.doc_off[d0], h_end = a.doc_off[d0 + 1];
  if (tid == 0 && h_off < g0) {  // e1 of the position before the tile: asap at its first
    const uint32_t s = a.perm[g0 - 1];
    if (s < h_end - h_off && (in_marks(a.marks, h_off + s) & 2u)) s_prev = 1;
  }

  // 2. the marks gathered through weave_perm, and the three bitmaps
  for (uint32_t it0 = 0; it0 < 32 && it0 * IN_NT < cnt; it0 += IN_U) {
    uint32_t src[IN_U];
#pragma unroll
    for (uint32_t u = 0; u < IN_U; u++) {
      const uint32_t x = (it0 + u) * IN_NT + tid;
      src[u] = x < cnt ? a.perm[g0 + x] : IN_NONE;
    }
#pragma unroll
    for (uint32_t u = 0; u < IN_U; u++) {
      const uint32_t x = (it0 + u) * IN_NT + tid, g = g0 + x;
      uint32_t d = d0, o = h_off, n = h_end - h_off;
      if (x < cnt && g >= h_end) {
        d = in_doc_of(a.doc_off, d0 + 1, dhi, g);
        o = a.doc_off[d];
        n = a.doc_off[d + 1] - o;
      }
      const uint32_t i = g - o;
      const uint32_t mk = (x < cnt && src[u] < n) ? in_marks(a.marks, o + src[u]) : 0u;
      const bool e1 = mk & 2u, e2 = mk & 4u;
      if (e1) atomicMin(a.doc_a + d, i + 1);
      if (e2) atomicMin(a.doc_a + d, i);
      const uint64_t m_nl = __ballot(mk & 1u), m_e1 = __ballot(e1 && i + 1 < n), m_e2 = __ballot(e2);
      in_put_words(nlw, m_nl, x, lane);
      in_put_words(e1w, m_e1, x, lane);
      in_put_words(e2w, m_e2, x, lane);
    }
  }
  __syncthreads();

  // 3. candidates for p: the first nl position at or after each asap position
  uint32_t as = e2w[tid] | (e1w[tid] << 1) | (tid ? e1w[tid - 1] >> 31 : s_prev);
  while (as) {
    const uint32_t x = tid * 32 + (uint32_t)__builtin_ctz(as), g = g0 + x;
    as &= as - 1;
    const uint32_t d = g < h_end ? d0 : in_doc_of(a.doc_off, d0 + 1, dhi, g);
    const uint32_t o = a.doc_off[d], n = a.doc_off[d + 1] - o, i = g - o;
    const uint32_t rest = n - i, lim = cnt - x < rest ? cnt : x + rest;  // the document's end inside the tile
    uint32_t ww = x >> 5, word = nlw[ww] & (~0u << (x & 31));
    for (;;) {
      if (word) {
        const uint32_t y = ww * 32 + (uint32_t)__builtin_ctz(word);
        if (y < lim) atomicMin(a.doc_f + d, i + (y - x));
        break;
      }
      if (++ww * 32 >= lim) break;
      word = nlw[ww];
    }
  }
  // 4. the first nl position of the tile's first document
  const uint32_t hl = h_end - g0 < cnt ? h_end - g0 : cnt;
  if (tid * 32 < hl) {
    uint32_t word = nlw[tid];
    if (hl - tid * 32 < 32) word &= (1u << (hl - tid * 32)) - 1;
    if (word) atomicMin(&s_g, tid * 32 + (uint32_t)__builtin_ctz(word));
  }
  __syncthreads();
  if (tid == 0) a.tile_g[t] = s_g == IN_NONE ? IN_NONE : g0 + s_g - h_off;
}

__device__ __forceinline__ uint64_t in_yarn_key(uint64_t id, uint32_t shift, uint64_t smask) {
  return (id >> shift) & smask;
}

__global__ __launch_bounds__(IN_PLAN_NT) void k_insert_plan(InArgs a) {
  __shared__ uint32_t cnts[IN_PLAN_DOCS];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t d = blockIdx.x * IN_PLAN_DOCS + w;
  uint32_t newn = 0;
  if (d < a.D) {  // (wave-uniform)
    const uint32_t o = a.doc_off[d], n = a.doc_off[d + 1] - o;
    const uint32_t to = a.tx_off[d], k = a.tx_off[d + 1] - to;
    uint32_t status = 0, p = IN_NONE;
    if (k) {
      const uint32_t fl = a.flags[d], A = a.doc_a[d];
      if (fl & IN_FOUND) {
        if (!(fl & IN_SAME)) status = CW_STATUS_DUP;
      } else if (!(fl & IN_CAUSE)) {
        status = CW_STATUS_ORPHAN;
      } else if (A >= n) {  // (the cause is the last node; or weave_perm does not hold it: IN_NONE)
        p = n;
      } else {
        const uint32_t F = a.doc_f[d];
        p = F < n ? F : n;
        // the tiles after a's, up to p's: their first nl index is one >= a
        const uint32_t ta = (o + A) / IN_TILE, tl = (o + n - 1) / IN_TILE;
        const uint32_t tp = (o + p) / IN_TILE, te = tp < tl ? tp : tl;
        for (uint32_t t0 = ta + 1; t0 <= te; t0 += 64) {
          const uint32_t g = (t0 + lane <= te) ? a.tile_g[t0 + lane] : IN_NONE;
          const uint64_t m = __ballot(g != IN_NONE);
          if (m) {
            const uint32_t first = __shfl(g, (int)__builtin_ctzll(m), 64);
            p = first < p ? first : p;
            break;
          }
        }
      }
    }
    const uint32_t kk = p != IN_NONE ? k : 0u;
    newn = n + kk;
    if (a.o_maxts) {  // refresh-ts: the largest id of the new document
      uint64_t mx = a.max_id[d];
      for (uint32_t m = lane; m < kk; m += 64) {
        const uint64_t x = a.tx_id[to + m];
        mx = x > mx ? x : mx;
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        const uint64_t y = __shfl_xor(mx, s, 64);
        mx = y > mx ? y : mx;
      }
      if (lane == 0) a.o_maxts[d] = mx >> a.ts_shift;
    }
    if (a.o_yarn) {  // tx node m goes behind the old yarn entries below it by (site, id)
      const uint64_t smask = (1ull << a.site_bits) - 1;
      for (uint32_t m = lane; m < kk; m += 64) {
        const uint64_t x = a.tx_id[to + m], xs = in_yarn_key(x, a.site_shift, smask);
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
          const uint32_t mid = lo + ((hi - lo) >> 1), e = a.yarn[o + mid];
          const uint64_t y = e < n ? a.id[(uint64_t)o + e] : 0ull, ys = in_yarn_key(y, a.site_shift, smask);
          if (ys < xs || (ys == xs && y < x)) lo = mid + 1;
          else hi = mid;
        }
        a.tx_rank[to + m] = lo + m;
      }
    }
    if (lane == 0) {
      a.pos[d] = p;
      if (a.o_pos) a.o_pos[d] = p;
      a.o_status[d] = status;
      a.o_count[d] = 0;
    }
  }
  if (lane == 0) cnts[w] = newn;
  __syncthreads();
  if (tid < 64) {  // the workgroup's sizes scanned, its base by the look-back
    const uint32_t v = lane < IN_PLAN_DOCS ? cnts[lane] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int s = 1; s < (int)IN_PLAN_DOCS; s <<= 1) {
      const uint32_t y = __shfl_up(x, s, 64);
      if (lane >= (uint32_t)s) x += y;
    }
    const uint32_t tot = __shfl(x, (int)IN_PLAN_DOCS - 1, 64);
    if (tid == 0) lb_publish(a.lb, blockIdx.x, a.epoch, tot);
    const uint32_t base = lb_exclusive(a.lb, blockIdx.x, a.epoch, tot);
    const uint32_t dd = blockIdx.x * IN_PLAN_DOCS + lane;
    if (lane < IN_PLAN_DOCS && dd < a.D) {
      a.new_off[dd] = (uint64_t)base + (x - v);
      if (dd == a.D - 1) a.new_off[a.D] = (uint64_t)base + x;
    }
  }
}

struct InDoc {  // a document of the result
  uint32_t no, oo, n, to, k, p;  // new and old first position, old size, first tx node, accepted tx nodes, place
};

__device__ __forceinline__ InDoc in_load_doc(const InArgs &a, uint32_t d) {
  InDoc r;
  r.no = (uint32_t)a.new_off[d];
  r.oo = a.doc_off[d];
  r.n = a.doc_off[d + 1] - r.oo;
  r.to = a.tx_off[d];
  r.p = a.pos[d];
  r.k = r.p != IN_NONE ? a.tx_off[d + 1] - r.to : 0u;
  return r;
}

// hide? (list.cljc:48-55) of new weave position j in p-1 .. p+k-1 of an accepted tx.
__device__ __forceinline__ bool in_renders(const InArgs &a, const InDoc &dc, uint32_t j) {
  uint64_t nid = 0, ncause = CW_NIL;
  uint8_t nkind = KIND_ROOT, xkind = 0;  // (a node that cannot be read does not render)
  if (j + 1 == dc.p) {
    const uint32_t s = a.perm[dc.oo + j];
    if (s < dc.n) {
      nid = a.id[(uint64_t)dc.oo + s];
      nkind = a.kind[(uint64_t)dc.oo + s];
    }
  } else {
    nid = a.tx_id[dc.to + (j - dc.p)];
    nkind = a.tx_kind[dc.to + (j - dc.p)];
  }
  bool next = false;
  if (j + 1 < dc.p + dc.k) {
    ncause = a.tx_cause[dc.to + (j + 1 - dc.p)];
    xkind = a.tx_kind[dc.to + (j + 1 - dc.p)];
    next = true;
  } else if (dc.p < dc.n) {  // the last tx node looks at the old weave[p]
    const uint32_t s = a.perm[dc.oo + dc.p];
    if (s < dc.n) {
      ncause = a.cause[(uint64_t)dc.oo + s];
      xkind = a.kind[(uint64_t)dc.oo + s];
      next = true;
    }
  }
  return !(is_special(nkind) || (nkind & KIND_ROOT) || (next && is_hide(xkind) && nid == ncause));
}

// (4 waves a SIMD: at most 128 VGPRs)
__global__ __launch_bounds__(IN_NT, 4) void k_insert_splice(InArgs a, uint32_t M) {
  __shared__ uint32_t words[IN_NT];
  __shared__ uint32_t s_dlo, s_dhi;

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t t = blockIdx.x, g0 = t * IN_TILE;  // (g0 < M)
  const uint32_t cnt = M - g0 < IN_TILE ? M - g0 : IN_TILE;
  words[tid] = 0;
  if (tid == 0) s_dlo = in_doc_of(a.new_off, 0u, a.D - 1, g0);
  if (tid == 64) s_dhi = in_doc_of(a.new_off, 0u, a.D - 1, g0 + cnt - 1);
  __syncthreads();
  const uint32_t d0 = s_dlo, dhi = s_dhi;
  const InDoc hd = in_load_doc(a, d0);
  const uint32_t h_ne = (uint32_t)a.new_off[d0 + 1];

  for (uint32_t it = 0; it < 32 && it * IN_NT < cnt; it++) {
    const uint32_t x = it * IN_NT + tid, q = g0 + x;
    bool vis = false;
    if (x < cnt) {
      InDoc dc = hd;
      uint32_t d = d0;
      if (q >= h_ne) {
        d = in_doc_of(a.new_off, d0 + 1, dhi, q);
        dc = in_load_doc(a, d);
      }
      const uint32_t j = q - dc.no;
      // the weave: old positions below p stay, the tx, the rest shifted by k
      const bool tx = dc.k && j >= dc.p && j < dc.p + dc.k;
      const uint32_t from = dc.oo + (j < dc.p ? j : j - dc.k);  // old global position
      a.o_perm[q] = tx ? dc.n + (j - dc.p) : a.perm[from];
      if (dc.k && j + 1 >= dc.p && j < dc.p + dc.k) vis = in_renders(a, dc, j);
      else vis = (a.bits[from >> 5] >> (from & 31)) & 1u;
      if (a.o_yarn) {
        uint32_t c = 0;  // tx nodes placed below yarn position j
        bool mine = false;
        if (dc.k && j >= a.tx_rank[dc.to]) {
          c = dc.k;
          if (j <= a.tx_rank[dc.to + dc.k - 1]) {  // the first tx node placed at or after j
            uint32_t lo = 0, hi = dc.k - 1;
            while (lo < hi) {
              const uint32_t mid = lo + ((hi - lo) >> 1);
              if (a.tx_rank[dc.to + mid] < j) lo = mid + 1;
              else hi = mid;
            }
            c = lo;
            mine = a.tx_rank[dc.to + lo] == j;
          }
        }
        uint32_t y = dc.n + c;
        if (!mine) y = j - c < dc.n ? a.yarn[dc.oo + (j - c)] : 0u;
        a.o_yarn[q] = y;
      }
      if (a.o_id) {  // the columns: old nodes in input order, then the tx
        const bool old = j < dc.n;
        const uint64_t at = old ? (uint64_t)dc.oo + j : (uint64_t)dc.to + (j - dc.n);
        a.o_id[q] = old ? a.id[at] : a.tx_id[at];
        a.o_cause[q] = old ? a.cause[at] : a.tx_cause[at];
        a.o_kind[q] = old ? a.kind[at] : a.tx_kind[at];
        if (a.o_value) a.o_value[q] = old ? a.value[at] : a.tx_value[at];
      }
    }
    in_put_words(words, __ballot(vis), x, lane);
  }
  __syncthreads();
  const uint32_t word = words[tid], x0 = tid * 32;
  if (x0 < cnt) a.o_bits[(g0 >> 5) + tid] = word;
  // visible_count: the tile's first document by waves, the others word by word
  const uint32_t hl = h_ne - g0 < cnt ? h_ne - g0 : cnt;
  uint32_t hc = 0;
  if (x0 < hl) hc = __popc(hl - x0 < 32 ? word & ((1u << (hl - x0)) - 1) : word);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hc += __shfl_xor(hc, o, 64);
  if (lane == 0 && hc) atomicAdd(a.o_count + d0, hc);
  const uint32_t x1 = x0 + 32 < cnt ? x0 + 32 : cnt;
  for (uint32_t x = x0 > hl ? x0 : hl; x < x1;) {
    const uint32_t d = in_doc_of(a.new_off, d0 + 1, dhi, g0 + x);
    const uint64_t e64 = a.new_off[d + 1] - g0;
    const uint32_t e = e64 < x1 ? (uint32_t)e64 : x1;
    uint32_t m = word >> (x - x0);
    if (e - x < 32) m &= (1u << (e - x)) - 1;
    if (m) atomicAdd(a.o_count + d, (uint32_t)__popc(m));
    x = e;
  }
}

namespace {

int insert_lists_impl(cw_ctx *c, const cw_insert_batch *b, cw_insert_result *r, int memspace) {
  if (!b || !r) return fail(c, "null batch/result");
  if (memspace != CW_MEM_HOST && memspace != CW_MEM_DEVICE) return fail(c, "bad memspace");
  const bool dev = memspace == CW_MEM_DEVICE;
  const uint64_t D = b->docs.n_docs;
  if (!b->docs.doc_offsets || !b->tx_offsets || !r->new_offsets)
    return fail(c, "doc_offsets, tx_offsets and new_offsets are required (host memory)");
  if (check_doc_offsets(c, b->docs.doc_offsets, D, LINK_IDX, LINK_IDX)) return -1;
  const uint64_t *off = b->docs.doc_offsets, *toff = b->tx_offsets;
  if (toff[0] != 0) return fail(c, "tx_offsets[0] must be 0");
  for (uint64_t d = 0; d < D; d++) {
    if (toff[d + 1] < toff[d]) return fail(c, "tx_offsets not monotone");
    if ((off[d + 1] - off[d]) + (toff[d + 1] - toff[d]) >= LINK_IDX)
      return fail(c, "document %llu too large with its tx (limit %llu nodes)", (unsigned long long)d,
                  (unsigned long long)LINK_IDX - 1);
  }
  const uint64_t N = off[D], T = toff[D];
  if (N + T >= 0xFFFFFFFFull || D >= 0xFFFFFFFFull)
    return fail(c, "batch too large: N+T=%llu (limit 2^32-1)", (unsigned long long)(N + T));
  if (N && (!b->weave_perm || !b->visible_bits || !b->docs.id_key || !b->docs.cause_key || !b->docs.kind))
    return fail(c, "null input arrays");
  if (T && (!b->tx_id || !b->tx_cause || !b->tx_kind)) return fail(c, "null tx arrays");
  if ((b->doc_value == nullptr) != (b->tx_value == nullptr))
    return fail(c, "doc_value and tx_value go together");
  const cw_list_result &res = r->weave;
  if (res.yarn_perm && (!b->yarn_perm || b->docs.site_bits == 0))
    return fail(c, "weave.yarn_perm needs yarn_perm and site_bits > 0");
  if (b->docs.site_bits > 32 || b->docs.site_shift > 63 || b->docs.ts_shift > 63)
    return fail(c, "bad key layout");
  const int cols = (r->id_key != nullptr) + (r->cause_key != nullptr) + (r->kind != nullptr);
  if (cols != 0 && cols != 3) return fail(c, "output columns id_key, cause_key, kind: all three or none");
  if (r->value && (!cols || !b->doc_value)) return fail(c, "value goes with the output columns and doc_value");
  if (!res.weave_perm || !res.visible_bits || !res.visible_count || !res.status)
    return fail(c, "null output arrays");
  if (D == 0) {
    r->new_offsets[0] = 0;
    return 0;
  }
  HIPCHK(c, hipSetDevice(c->device));
  auto &st = c->insert;
  const uint32_t tiles = (uint32_t)((N + IN_TILE - 1) / IN_TILE);
  const uint32_t pblocks = (uint32_t)((D + IN_PLAN_DOCS - 1) / IN_PLAN_DOCS);
  if (!grid_ok(tiles, IN_NT) || !grid_ok(pblocks, IN_PLAN_NT) || !grid_ok((N + T + IN_TILE - 1) / IN_TILE, IN_NT))
    return fail(c, "batch too large for one dispatch");

  InArgs a{};
  a.N = (uint32_t)N;
  a.D = (uint32_t)D;
  a.id = b->docs.id_key;
  a.cause = b->docs.cause_key;
  a.kind = b->docs.kind;
  a.value = b->doc_value;
  a.perm = b->weave_perm;
  a.bits = b->visible_bits;
  a.yarn = res.yarn_perm ? b->yarn_perm : nullptr;
  a.tx_id = b->tx_id;
  a.tx_cause = b->tx_cause;
  a.tx_kind = b->tx_kind;
  a.tx_value = b->tx_value;
  a.ts_shift = b->docs.ts_shift;
  a.site_shift = b->docs.site_shift;
  a.site_bits = b->docs.site_bits;
  a.o_perm = res.weave_perm;
  a.o_bits = res.visible_bits;
  a.o_count = res.visible_count;
  a.o_status = res.status;
  a.o_yarn = res.yarn_perm;
  a.o_maxts = res.max_ts;
  a.o_pos = r->insert_pos;
  a.o_id = r->id_key;
  a.o_cause = r->cause_key;
  a.o_kind = r->kind;
  a.o_value = r->value;
  const uint64_t NT = N + T, NTs = std::max<uint64_t>(NT, 1);
  cw_list_result dres{};
  if (!dev) {  // uploads, and the outputs staged
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (upload(c, "is_id", b->docs.id_key, (size_t)N * 8, &a.id) ||
        upload(c, "is_cause", b->docs.cause_key, (size_t)N * 8, &a.cause) ||
        upload(c, "is_kind", b->docs.kind, (size_t)N, &a.kind) ||
        upload(c, "is_perm", b->weave_perm, (size_t)N * 4, &a.perm) ||
        upload(c, "is_bits", b->visible_bits, (size_t)((N + 31) / 32) * 4, &a.bits) ||
        upload(c, "is_txid", b->tx_id, (size_t)T * 8, &a.tx_id) ||
        upload(c, "is_txca", b->tx_cause, (size_t)T * 8, &a.tx_cause) ||
        upload(c, "is_txkd", b->tx_kind, (size_t)T, &a.tx_kind))
      return -1;
    if (a.yarn && upload(c, "is_yarn", b->yarn_perm, (size_t)N * 4, &a.yarn)) return -1;
    if (a.value && (upload(c, "is_val", b->doc_value, (size_t)N * 8, &a.value) ||
                    upload(c, "is_txval", b->tx_value, (size_t)T * 8, &a.tx_value)))
      return -1;
    if (stage_list_result(c, res, NT, D, &dres)) return -1;
    a.o_perm = dres.weave_perm;
    a.o_bits = dres.visible_bits;
    a.o_count = dres.visible_count;
    a.o_status = dres.status;
    a.o_yarn = dres.yarn_perm;
    a.o_maxts = dres.max_ts;
    if (r->insert_pos) a.o_pos = scratch_t<uint32_t>(c, "is_opos", D);
    if (cols) {
      a.o_id = scratch_t<uint64_t>(c, "is_oid", NTs);
      a.o_cause = scratch_t<uint64_t>(c, "is_oca", NTs);
      a.o_kind = scratch_t<uint8_t>(c, "is_okd", NTs);
    }
    if (r->value) a.o_value = scratch_t<uint64_t>(c, "is_oval", NTs);
    if ((r->insert_pos && !a.o_pos) || (cols && (!a.o_id || !a.o_cause || !a.o_kind)) || (r->value && !a.o_value))
      return fail(c, "out of device memory (host-mode staging)");
  }

  // the two layouts on the device, each cached while it repeats (a chain of
  // calls grows the documents under the same tx_offsets)
  const char *n_off = "in_off", *n_toff = "in_toff";
  bool miss;
  if (device_layout(c, st.docs, D, off, nullptr, &n_off, nullptr, &a.doc_off, &miss) ||
      device_layout(c, st.txs, D, toff, nullptr, &n_toff, nullptr, &a.tx_off, &miss))
    return -1;
  // per document: a and f (all ones), the max id and the flags (zero), p
  uint32_t *af = scratch_t<uint32_t>(c, "in_af", 2 * D);
  unsigned long long *mf = scratch_t<unsigned long long>(c, "in_mf", D + (D + 1) / 2);
  a.pos = scratch_t<uint32_t>(c, "in_pos", D);
  a.tile_g = scratch_t<uint32_t>(c, "in_tg", tiles);
  a.tx_rank = scratch_t<uint32_t>(c, "in_txr", T);
  a.new_off = scratch_t<uint64_t>(c, "in_noff", D + 1);
  a.marks = scratch_t<uint32_t>(c, "in_marks", (size_t)tiles * IN_NT * 3);
  if (!af || !mf || !a.pos || !a.tile_g || !a.tx_rank || !a.new_off || !a.marks)
    return fail(c, "out of device memory (list insert)");
  a.doc_a = af;
  a.doc_f = af + D;
  a.max_id = mf;
  a.flags = reinterpret_cast<uint32_t *>(mf + D);
  a.lb = lookback_words(c, st.lb, "in_lb", pblocks, 1, &a.epoch);
  if (!a.lb) return -1;
  HIPCHK(c, hipMemsetAsync(af, 0xFF, 2 * D * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(mf, 0, (D + (D + 1) / 2) * 8, c->stream));

  if (tiles) {
    // per node its id, cause and kind in and its three marks out; per document
    // its offsets, first tx node and record
    Launch L(c, "k_insert_mark", (double)N * 17.375 + (double)D * 48);
    hipLaunchKernelGGL(k_insert_mark, dim3(tiles), dim3(IN_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_insert_mark")) return -1;
  if (tiles) {
    // per old position its weave_perm word and the marks gathered through it
    // (a document's marks: 3 bits a node); per document its offsets and `a`
    Launch L(c, "k_insert_find", (double)N * 4.375 + (double)D * 16 + (double)tiles * 4);
    hipLaunchKernelGGL(k_insert_find, dim3(tiles), dim3(IN_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_insert_find")) return -1;
  {
    // per document its offsets, record, outputs and new offset; per tx node its
    // id (max_ts) and, with yarns, its id again and its place
    Launch L(c, "k_insert_plan", (double)D * 76 + (double)T * (a.o_maxts ? 8 : 0) + (double)T * (a.o_yarn ? 12 : 0));
    hipLaunchKernelGGL(k_insert_plan, dim3(pblocks), dim3(IN_PLAN_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_insert_plan")) return -1;
  // the call's one wait: the new offsets size the splice
  HIPCHK(c, hipMemcpyAsync(r->new_offsets, a.new_off, (D + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t M = r->new_offsets[D];
  if (M > NT) return fail(c, "internal: new offsets past N + T");
  if (M) {
    // per new position: weave_perm in and out, its bit in and out; yarn_perm in
    // and out; the columns in and out
    double per = 8.25;
    if (a.o_yarn) per += 8;
    if (a.o_id) per += 34;
    if (a.o_value) per += 16;
    Launch L(c, "k_insert_splice", (double)M * per + (double)D * 28);
    hipLaunchKernelGGL(k_insert_splice, dim3((uint32_t)((M + IN_TILE - 1) / IN_TILE)), dim3(IN_NT), 0, c->stream,
                       a, (uint32_t)M);
  }
  if (check_launch(c, "k_insert_splice")) return -1;
  if (!dev) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (unstage_list_result(c, dres, M, D, res)) return -1;
    if (r->insert_pos) HIPCHK(c, hipMemcpy(r->insert_pos, a.o_pos, D * 4, hipMemcpyDeviceToHost));
    if (M && cols) {
      HIPCHK(c, hipMemcpy(r->id_key, a.o_id, M * 8, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(r->cause_key, a.o_cause, M * 8, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(r->kind, a.o_kind, M, hipMemcpyDeviceToHost));
    }
    if (M && r->value) HIPCHK(c, hipMemcpy(r->value, a.o_value, M * 8, hipMemcpyDeviceToHost));
  } else if (!c->async) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return c->prof ? collect_prof(c) : 0;
}

}  // namespace
