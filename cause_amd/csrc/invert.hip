// invert.hip -- cw_invert (include/causeweave_invert.h): invert- (base/core.cljc:
// 313-343), the transaction of h.hide / h.show nodes that takes a slice of a
// base's history back; what undo-, redo- and reset- end in.  Included by
// causeweave.hip after listinsert.hip (in_doc_of, in_put_words, lookback.h).
//
// A CANDIDATE is a selected node of a document that is not hidden, already
// inverted: (document, cause_is_id', cause', id, kind', src).  The parts of a
// base are its candidates with one kept per (document, cause_is_id', cause'):
// the one with the smallest id, numbered by descending largest id of its key.
//
// k_invert_mark, a tile of IV_TILE = 8,192 input positions (listinsert.hip's
//   geometry): the range and site test of every node, balloted into the
//   bitmap selw; hidden[ref_doc] = 1 for a selected node's reference inside its
//   base; the tile's count of selected nodes.  Reads id, kind and ref_doc; the
//   cause is read for selected nodes only, by the next pass.
// k_invert_compact, the same tiles (a launch of its own: every hidden flag
//   must be there before a candidate is emitted): the selected bits of hidden
//   documents cleared, the bitmap written back, the tile's candidates counted
//   and numbered by the decoupled look-back (tile_base), then emitted in input
//   order -- position-major, so the columns stream in with coalesced loads.
// k_invert_base_w, a wave a base: the base's candidates are the contiguous
//   range [rank(first position), rank(end position)) with rank(p) = tile_base
//   + the bits below p in p's tile.  None: nothing to do.  Up to IV_CAP_W =
//   256 (and invert_cap): finished here, iv_base.  Up to invert_cap: appended
//   to the list `big`.  More: the overflow flag, the call takes the general route.
// k_invert_base_wg, workgroups of 512 threads over the list `big`: iv_base with
//   IV_CAP = 4,096 slots of LDS (29 bytes a slot).
// iv_base, all in LDS: indices bitonic-sorted by (document, cause_is_id, cause,
//   id); the run heads are the parts (oldest node) and a run's tail gives the
//   order key; the parts sorted by descending order key: the tx-index; the
//   parts sorted by (document, tx-index); written to the staging columns at the
//   base's own candidate slots, with each document's first and end slot.
// invert_general, any base above the cap: the same over every candidate of the
//   call with the library's stable key sort (radix_sort), least significant key
//   first: id, cause, document << 2 | cause_is_id; k_iv_runs marks the run
//   heads and finds each one's tail; then order key, base, and k_iv_txidx
//   numbers the parts of a base; then document, and k_iv_stage fills the same
//   staging columns.
// k_invert_write, a wave a document (16 a workgroup): the document's parts
//   counted, the part offsets by a scan and the look-back, the parts copied from
//   the staging columns to their place; status and base_parts.
//
// Nothing is read or written outside the caller's arrays: every position is
// < N, every candidate rank < the tile's count, ref_doc is checked against the
// base's documents before hidden[] is written.

constexpr uint32_t IV_NT = 256;
constexpr uint32_t IV_TILE = IV_NT * 32;  // positions a tile, a bitmap word a thread
constexpr uint32_t IV_U = 4;              // loads in flight a thread (k_invert_mark)
constexpr uint32_t IV_NONE = 0xFFFFFFFFu;
constexpr uint32_t IV_CAP = 4096, IV_CAP_W = 256;  // candidates a workgroup / a wave finishes in LDS
constexpr uint32_t IV_WG_NT = 512;
constexpr uint32_t IV_OVER = 0xFFFFFFFFu;  // base_cnt: more parts than the tx field holds
constexpr uint32_t IV_WR_NT = 1024, IV_WR_DOCS = IV_WR_NT / 64;
constexpr uint16_t IV_PAD = 0xFFFFu;  // a sort slot past the last element
// iv_base's LDS for `cap` slots: id, cause (8), document (4), four index arrays (2), kc (1); the scan's words
__host__ __device__ constexpr uint32_t iv_lds_bytes(uint32_t cap) { return cap * 29u + 64u; }

struct IvArgs {
  uint32_t N, D, G, tiles;
  const uint32_t *doc_off, *base_off;  // device [D + 1], [G + 1]
  const uint64_t *id, *cause;
  const uint8_t *kind, *cii;
  const uint32_t *ref;
  const uint64_t *sel_lo, *sel_hi, *sel_sites, *new_tx;
  uint32_t site_shift, site_bits, mask_words;
  uint32_t cap, wg;  // invert_cap; the workgroup kernel can run
  uint32_t *selw;    // [256 * tiles] the selected bits; after k_invert_compact the candidates' bits
  uint32_t *hidden;  // [D] (0)
  uint32_t *tile_sel, *tile_base;  // [tiles], [tiles + 1]
  // the candidates, in input order
  uint64_t *c_id, *c_cause;
  uint32_t *c_doc, *c_src;
  uint8_t *c_kc;  // cause_is_id' | kind' << 2
  // per base: its first candidate and their number; the bases left to the workgroup kernel
  uint32_t *base_lo, *base_n, *big;
  uint32_t *ctl;  // [0] entries of big, [1] a base above the cap, [2] candidates
  // the staged parts: per document its first and end slot (0), per base its parts or IV_OVER (0)
  uint64_t *s_id, *s_cause;
  uint32_t *s_src;
  uint8_t *s_kc;
  uint32_t *doc_stage, *doc_end, *base_cnt;
  uint64_t *new_off;  // device [D + 1]
  unsigned long long *lb;
  uint32_t epoch;
  // outputs
  uint64_t *o_id, *o_cause;
  uint8_t *o_cii, *o_kind;
  uint32_t *o_src, *o_base_parts, *o_status;
};

// Exclusive prefix of v over the workgroup's NT threads; *total: the sum.
// tmp: NT / 64 words of LDS, free again after the call.
template <uint32_t NT>
__device__ __forceinline__ uint32_t iv_scan(uint32_t v, uint32_t *tmp, uint32_t *total) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t y = __shfl_up(x, s, 64);
    if (lane >= (uint32_t)s) x += y;
  }
  if constexpr (NT == 64) {
    *total = __shfl(x, 63, 64);
    return x - v;
  } else {
    __syncthreads();
    if (lane == 63) tmp[w] = x;
    __syncthreads();
    uint32_t b = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < NT / 64; k++) {
      const uint32_t c = tmp[k];
      b += k < w ? c : 0u;
      tot += c;
    }
    *total = tot;
    return b + x - v;
  }
}

// (8 waves a SIMD: at most 64 VGPRs)
__global__ __launch_bounds__(IV_NT, 8) void k_invert_mark(IvArgs a) {
  __shared__ uint32_t s_dlo, s_dhi, s_cnt;

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t t = blockIdx.x, g0 = t * IV_TILE;  // (t < tiles: g0 < N)
  const uint32_t cnt = a.N - g0 < IV_TILE ? a.N - g0 : IV_TILE;
  if (tid == 0) {
    s_dlo = in_doc_of(a.doc_off, 0u, a.D - 1, g0);
    s_cnt = 0;
  }
  if (tid == 64) s_dhi = in_doc_of(a.doc_off, 0u, a.D - 1, g0 + cnt - 1);
  __syncthreads();
  // the tile's first document and its base serve most positions
  const uint32_t d0 = s_dlo, dhi = s_dhi, h_end = a.doc_off[d0 + 1];
  const uint32_t hb = in_doc_of(a.base_off, 0u, a.G - 1, d0);
  const uint32_t h_b0 = a.base_off[hb], h_b1 = a.base_off[hb + 1];
  const uint64_t h_lo = a.sel_lo[hb], h_hi = a.sel_hi[hb];
  const uint32_t smask = (1u << a.site_bits) - 1;
  for (uint32_t it0 = 0; it0 < 32 && it0 * IV_NT < cnt; it0 += IV_U) {
    uint64_t idv[IV_U];
    uint32_t rfv[IV_U];
    uint8_t kdv[IV_U];
#pragma unroll
    for (uint32_t u = 0; u < IV_U; u++) {
      const uint32_t x = (it0 + u) * IV_NT + tid;
      idv[u] = 0;
      rfv[u] = IV_NONE;
      kdv[u] = KIND_ROOT;
      if (x < cnt) {
        idv[u] = a.id[g0 + x];
        kdv[u] = a.kind[g0 + x];
        if (a.ref) rfv[u] = a.ref[g0 + x];
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < IV_U; u++) {
      const uint32_t x = (it0 + u) * IV_NT + tid, g = g0 + x;
      const bool in = x < cnt;
      uint32_t gb = hb, b0 = h_b0, b1 = h_b1;
      uint64_t lo = h_lo, hi = h_hi;
      if (in && g >= h_end) {
        const uint32_t d = in_doc_of(a.doc_off, d0 + 1, dhi, g);
        if (d >= h_b1) {
          gb = in_doc_of(a.base_off, hb, a.G - 1, d);
          b0 = a.base_off[gb];
          b1 = a.base_off[gb + 1];
          lo = a.sel_lo[gb];
          hi = a.sel_hi[gb];
        }
      }
      bool sel = in && !(kdv[u] & KIND_ROOT) && idv[u] >= lo && idv[u] <= hi;
      if (sel) {
        const uint32_t r = (uint32_t)(idv[u] >> a.site_shift) & smask;
        sel = (a.sel_sites[(size_t)gb * a.mask_words + (r >> 6)] >> (r & 63)) & 1ull;
      }
      if (sel && rfv[u] >= b0 && rfv[u] < b1) a.hidden[rfv[u]] = 1u;  // (b1 <= D: IV_NONE is outside)
      const uint64_t m = __ballot(sel);
      if (lane < 2)  // (x - lane: the wave's first position)
        a.selw[(g0 >> 5) + ((x - lane) >> 5) + lane] = (uint32_t)(m >> (32 * lane));
      if (lane == 0 && m) atomicAdd(&s_cnt, (uint32_t)__popcll(m));
    }
  }
  __syncthreads();
  if (tid == 0) a.tile_sel[t] = s_cnt;
}

// (8 waves a SIMD: at most 64 VGPRs)
__global__ __launch_bounds__(IV_NT, 8) void k_invert_compact(IvArgs a) {
  __shared__ uint32_t fw[IV_NT], wpre[IV_NT], tmp[IV_NT / 64];
  __shared__ uint32_t s_dlo, s_dhi, s_base;

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t t = blockIdx.x, g0 = t * IV_TILE;  // (t < tiles: g0 < N)
  const uint32_t cnt = a.N - g0 < IV_TILE ? a.N - g0 : IV_TILE;
  const uint32_t nsel = a.tile_sel[t];
  fw[tid] = 0;
  if (tid == 0) s_dlo = in_doc_of(a.doc_off, 0u, a.D - 1, g0);
  if (tid == 64) s_dhi = in_doc_of(a.doc_off, 0u, a.D - 1, g0 + cnt - 1);
  __syncthreads();
  const uint32_t d0 = s_dlo, dhi = s_dhi, h_off = a.doc_off[d0], h_end = a.doc_off[d0 + 1];
  // 1. the selected bits of documents that are not hidden
  if (nsel) {
    for (uint32_t it = 0; it < 32 && it * IV_NT < cnt; it++) {
      const uint32_t x = it * IV_NT + tid, g = g0 + x;
      bool c = x < cnt && ((a.selw[(g0 >> 5) + (x >> 5)] >> (x & 31)) & 1u);
      if (c) c = a.hidden[g < h_end ? d0 : in_doc_of(a.doc_off, d0 + 1, dhi, g)] == 0;
      in_put_words(fw, __ballot(c), x, lane);
    }
    __syncthreads();
  }
  // 2. the words' counts scanned, the tile's first rank by the look-back
  const uint32_t word = fw[tid];
  uint32_t total;
  wpre[tid] = iv_scan<IV_NT>((uint32_t)__popc(word), tmp, &total);
  if (tid < 64) {
    if (tid == 0) lb_publish(a.lb, t, a.epoch, total);
    const uint32_t base = lb_exclusive(a.lb, t, a.epoch, total);
    if (tid == 0) {
      s_base = base;
      a.tile_base[t] = base;
      if (t + 1 == a.tiles) {
        a.tile_base[a.tiles] = base + total;
        a.ctl[2] = base + total;
      }
    }
  }
  if (tid * 32 < cnt) a.selw[(g0 >> 5) + tid] = word;
  __syncthreads();
  if (!total) return;
  // 3. the candidates, in input order
  const uint32_t base = s_base;
  for (uint32_t it = 0; it < 32 && it * IV_NT < cnt; it++) {
    const uint32_t x = it * IV_NT + tid, g = g0 + x;
    const uint32_t w = fw[x >> 5];
    if (x >= cnt || !((w >> (x & 31)) & 1u)) continue;
    const uint32_t r = base + wpre[x >> 5] + (uint32_t)__popc(w & ((1u << (x & 31)) - 1));
    uint32_t d = d0, o = h_off;
    if (g >= h_end) {
      d = in_doc_of(a.doc_off, d0 + 1, dhi, g);
      o = a.doc_off[d];
    }
    const uint64_t id = a.id[g];
    const uint32_t k = a.kind[g] & KIND_CLASS;
    // invert-path (:313-320)
    uint64_t ca = id;
    uint32_t ci = 1, ki = KIND_HHIDE;
    if (k) {
      ci = a.cii ? a.cii[g] & 3u : 1u;
      ca = ci == 2 ? 0ull : a.cause[g];
      ki = k == 3 ? KIND_HHIDE : 3u;
    }
    a.c_id[r] = id;
    a.c_cause[r] = ca;
    a.c_doc[r] = d;
    a.c_src[r] = g - o;
    a.c_kc[r] = (uint8_t)(ci | (ki << 2));
  }
}

// The candidates before input position p (p <= N): all 64 lanes, wave-uniform.
__device__ __forceinline__ uint32_t iv_rank(const IvArgs &a, uint32_t p, uint32_t lane) {
  if (p >= a.N) return a.tile_base[a.tiles];
  const uint32_t t = p / IV_TILE, wp = p >> 5;
  uint32_t s = 0;
  for (uint32_t w = t * IV_NT + lane; w < wp; w += 64) s += (uint32_t)__popc(a.selw[w]);
  if (lane == 0 && (p & 31)) s += (uint32_t)__popc(a.selw[wp] & ((1u << (p & 31)) - 1));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return a.tile_base[t] + s;
}

// p[0 .. m) (m a power of two) sorted by less(x, y) over the entries; IV_PAD sorts last.
template <uint32_t NT, typename Less>
__device__ __forceinline__ void iv_bitonic(uint16_t *p, uint32_t m, Less less) {
  for (uint32_t k = 2; k <= m; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < (m >> 1); i += NT) {
        const uint32_t lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const bool up = (lo & k) == 0;
        const uint16_t x = p[lo], y = p[hi];
        const bool lt = y != IV_PAD && (x == IV_PAD || less(y, x));  // y before x
        if (lt == up && x != y) {
          p[lo] = y;
          p[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ uint32_t iv_pow2(uint32_t n) {
  uint32_t m = 1;
  while (m < n) m <<= 1;
  return m;
}

// One base's n candidates (1 <= n <= CAP), [lo, lo + n) of the candidate columns,
// to its staged parts.  Every thread of the workgroup; n, lo and g uniform.
template <uint32_t CAP, uint32_t NT>
__device__ void iv_base(const IvArgs &a, uint32_t g, uint32_t lo, uint32_t n, unsigned char *lds) {
  uint64_t *const id = reinterpret_cast<uint64_t *>(lds), *const cause = id + CAP;
  uint32_t *const doc = reinterpret_cast<uint32_t *>(cause + CAP);
  uint16_t *const p = reinterpret_cast<uint16_t *>(doc + CAP), *const q = p + CAP, *const tl = q + CAP,
                  *const tx = tl + CAP;
  uint8_t *const kc = reinterpret_cast<uint8_t *>(tx + CAP);
  uint32_t *const tmp = reinterpret_cast<uint32_t *>(kc + CAP);
  const uint32_t tid = threadIdx.x;

  // 1. ordered by (document, cause_is_id, cause, id)
  const uint32_t m = iv_pow2(n);
  for (uint32_t i = tid; i < m; i += NT) {
    if (i < n) {
      id[i] = a.c_id[lo + i];
      cause[i] = a.c_cause[lo + i];
      doc[i] = a.c_doc[lo + i];
      kc[i] = a.c_kc[lo + i];
    }
    p[i] = i < n ? (uint16_t)i : IV_PAD;
  }
  __syncthreads();
  iv_bitonic<NT>(p, m, [&](uint32_t x, uint32_t y) {
    if (doc[x] != doc[y]) return doc[x] < doc[y];
    const uint32_t cx = kc[x] & 3u, cy = kc[y] & 3u;
    if (cx != cy) return cx < cy;
    if (cause[x] != cause[y]) return cause[x] < cause[y];
    return id[x] < id[y];
  });
  // 2. a run's head is the part (the oldest node), its tail's id the order key
  const uint32_t ch = (n + NT - 1) / NT, i0 = tid * ch < n ? tid * ch : n, i1 = i0 + ch < n ? i0 + ch : n;
  auto head = [&](uint32_t i) {
    if (i == 0) return true;
    const uint32_t x = p[i], y = p[i - 1];
    return doc[x] != doc[y] || ((kc[x] ^ kc[y]) & 3u) || cause[x] != cause[y];
  };
  uint32_t hc = 0;
  for (uint32_t i = i0; i < i1; i++) hc += head(i) ? 1u : 0u;
  uint32_t P;
  uint32_t j = iv_scan<NT>(hc, tmp, &P);
  for (uint32_t i = i0; i < i1; i++) {
    if (!head(i)) continue;
    q[j] = p[i];
    if (j) tl[j - 1] = p[i - 1];
    j++;
  }
  if (tid == 0) tl[P - 1] = p[n - 1];
  __syncthreads();
  if ((uint64_t)P > (1ull << a.site_shift)) {  // the tx field does not hold them
    if (tid == 0) a.base_cnt[g] = IV_OVER;
    return;
  }
  // 3. the tx-index: the rank by descending order key
  const uint32_t mp = iv_pow2(P);
  for (uint32_t i = tid; i < mp; i += NT) p[i] = i < P ? (uint16_t)i : IV_PAD;
  __syncthreads();
  iv_bitonic<NT>(p, mp, [&](uint32_t x, uint32_t y) { return id[tl[x]] > id[tl[y]]; });
  for (uint32_t k = tid; k < P; k += NT) tx[p[k]] = (uint16_t)k;
  __syncthreads();
  // 4. regrouped by document, tx-index ascending
  for (uint32_t i = tid; i < mp; i += NT) p[i] = i < P ? (uint16_t)i : IV_PAD;
  __syncthreads();
  iv_bitonic<NT>(p, mp, [&](uint32_t x, uint32_t y) {
    const uint32_t dx = doc[q[x]], dy = doc[q[y]];
    return dx != dy ? dx < dy : tx[x] < tx[y];
  });
  // 5. staged at the base's own slots
  const uint64_t tx0 = a.new_tx[g];
  for (uint32_t k = tid; k < P; k += NT) {
    const uint32_t e = p[k], h = q[e], d = doc[h], s = lo + k;
    a.s_id[s] = tx0 + tx[e];
    a.s_cause[s] = cause[h];
    a.s_kc[s] = kc[h];
    a.s_src[s] = a.c_src[lo + h];
    if (k == 0 || doc[q[p[k - 1]]] != d) a.doc_stage[d] = s;
    if (k + 1 == P || doc[q[p[k + 1]]] != d) a.doc_end[d] = s + 1;
  }
  if (tid == 0) a.base_cnt[g] = P;
}

__global__ __launch_bounds__(64) void k_invert_base_w(IvArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char iv_lds[];
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  const uint32_t lo = iv_rank(a, a.doc_off[a.base_off[g]], lane);
  const uint32_t hi = iv_rank(a, a.doc_off[a.base_off[g + 1]], lane), C = a.tile_base[a.tiles];
  const uint32_t n = lo <= hi && hi <= C ? hi - lo : 0u;  // (the ranks do not decrease: never the 0)
  if (lane == 0) {
    a.base_lo[g] = lo;
    a.base_n[g] = n;
  }
  if (n == 0) return;  // (base_cnt, doc_stage and doc_end are zero)
  if (n <= IV_CAP_W && n <= a.cap) {
    iv_base<IV_CAP_W, 64>(a, g, lo, n, iv_lds);
  } else if (lane == 0) {
    if (a.wg && n <= a.cap) a.big[atomicAdd(a.ctl, 1u)] = g;
    else atomicOr(a.ctl + 1, 1u);
  }
}

__global__ __launch_bounds__(IV_WG_NT) void k_invert_base_wg(IvArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char iv_lds[];
  const uint32_t nb = a.ctl[0] < a.G ? a.ctl[0] : a.G;
  for (uint32_t i = blockIdx.x; i < nb; i += gridDim.x) {
    const uint32_t g = a.big[i];
    if (g >= a.G) continue;
    const uint32_t n = a.base_n[g];
    if (n && n <= IV_CAP) iv_base<IV_CAP, IV_WG_NT>(a, g, a.base_lo[g], n, iv_lds);
    __syncthreads();
  }
}

// ---- the general route: kernels around the key sort --------------------------
enum { IV_K_CAUSE = 0, IV_K_DOCKEY, IV_K_BASE, IV_K_DOC };

// The next sort's keys and values: element e = idx[i] (or i), key by `mode`.
__global__ __launch_bounds__(256) void k_iv_keys(IvArgs a, uint32_t C, int mode, const uint32_t *idx,
                                                 const uint8_t *head, uint64_t *key, uint32_t *val) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C) return;
  const uint32_t e = idx ? idx[i] : i;
  if (e >= C) return;
  uint64_t k;
  if (mode == IV_K_CAUSE) k = a.c_cause[e];
  else if (mode == IV_K_DOCKEY) k = ((uint64_t)a.c_doc[e] << 2) | (a.c_kc[e] & 3u);
  else if (mode == IV_K_BASE) k = head[e] ? in_doc_of(a.base_off, 0u, a.G - 1, a.c_doc[e]) : a.G;
  else k = head[e] ? a.c_doc[e] : a.D;
  key[i] = k;
  val[i] = e;
}

__device__ __forceinline__ bool iv_same_key(const IvArgs &a, uint32_t x, uint32_t y) {
  return a.c_doc[x] == a.c_doc[y] && !((a.c_kc[x] ^ a.c_kc[y]) & 3u) && a.c_cause[x] == a.c_cause[y];
}

// Sorted position i of v (by document, cause_is_id, cause, id): a run's head is
// a part; its order key, the complement of its tail's id (a search for the
// run's end: the keys do not decrease), sorts ascending = newest first.
__global__ __launch_bounds__(256) void k_iv_runs(IvArgs a, uint32_t C, const uint32_t *v, uint8_t *head,
                                                 uint64_t *okey) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C) return;
  const uint32_t e = v[i];
  if (e >= C) return;
  const bool h = i == 0 || v[i - 1] >= C || !iv_same_key(a, e, v[i - 1]);
  head[e] = h;
  uint64_t ok = ~0ull;
  if (h) {
    uint32_t lo = i, hi = C - 1;  // the last position of e's run
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo + 1) >> 1), x = v[mid];
      if (x < C && iv_same_key(a, e, x)) lo = mid;
      else hi = mid - 1;
    }
    ok = ~a.c_id[v[lo] < C ? v[lo] : e];
  }
  okey[e] = ok;
}

// Sorted position i of v (by base, order key): the part's tx-index is its
// distance from its base's first position; the base's last part counts them.
__global__ __launch_bounds__(256) void k_iv_txidx(IvArgs a, uint32_t C, const uint32_t *v, const uint64_t *bkey,
                                                  const uint8_t *head, uint32_t *txi) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C) return;
  const uint32_t e = v[i];
  if (e >= C || !head[e]) return;
  const uint64_t g = bkey[i];
  uint32_t lo = 0, hi = i;  // the first position with this base
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (bkey[mid] < g) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t tx = i - lo;
  txi[e] = tx;
  if (g < a.G && (i + 1 == C || bkey[i + 1] != g))
    a.base_cnt[g] = (uint64_t)tx + 1 > (1ull << a.site_shift) ? IV_OVER : tx + 1;
}

// Sorted position i of v (by document, tx-index; the parts first): staged at slot i.
__global__ __launch_bounds__(256) void k_iv_stage(IvArgs a, uint32_t C, const uint32_t *v, const uint8_t *head,
                                                  const uint32_t *txi) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C) return;
  const uint32_t e = v[i];
  if (e >= C || !head[e]) return;
  const uint32_t d = a.c_doc[e], g = in_doc_of(a.base_off, 0u, a.G - 1, d);
  a.s_id[i] = a.new_tx[g] + txi[e];
  a.s_cause[i] = a.c_cause[e];
  a.s_kc[i] = a.c_kc[e];
  a.s_src[i] = a.c_src[e];
  const uint32_t pv = i ? v[i - 1] : IV_NONE, nx = i + 1 < C ? v[i + 1] : IV_NONE;
  if (pv >= C || a.c_doc[pv] != d) a.doc_stage[d] = i;
  if (nx >= C || !head[nx] || a.c_doc[nx] != d) a.doc_end[d] = i + 1;
}

__global__ __launch_bounds__(IV_WR_NT) void k_invert_write(IvArgs a) {
  __shared__ uint32_t cnts[IV_WR_DOCS], offs[IV_WR_DOCS];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t d = blockIdx.x * IV_WR_DOCS + w;
  uint32_t cnt = 0, from = 0;
  if (d < a.D) {  // (wave-uniform)
    const uint32_t g = in_doc_of(a.base_off, 0u, a.G - 1, d), bc = a.base_cnt[g];
    from = a.doc_stage[d];
    const uint32_t end = a.doc_end[d];
    cnt = bc != IV_OVER && end > from && end <= a.N ? end - from : 0u;
    if (lane == 0) {
      a.o_status[d] = bc == IV_OVER ? (uint32_t)CW_STATUS_KEY_RANGE : 0u;
      if (a.o_base_parts && d == a.base_off[g]) a.o_base_parts[g] = bc == IV_OVER ? 0u : bc;
    }
  }
  if (lane == 0) cnts[w] = cnt;
  __syncthreads();
  if (tid < 64) {  // the workgroup's counts scanned, its base by the look-back
    const uint32_t v = lane < IV_WR_DOCS ? cnts[lane] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int s = 1; s < (int)IV_WR_DOCS; s <<= 1) {
      const uint32_t y = __shfl_up(x, s, 64);
      if (lane >= (uint32_t)s) x += y;
    }
    const uint32_t tot = __shfl(x, (int)IV_WR_DOCS - 1, 64);
    if (tid == 0) lb_publish(a.lb, blockIdx.x, a.epoch, tot);
    const uint32_t base = lb_exclusive(a.lb, blockIdx.x, a.epoch, tot);
    const uint32_t dd = blockIdx.x * IV_WR_DOCS + lane;
    if (lane < IV_WR_DOCS) offs[lane] = base + (x - v);
    if (lane < IV_WR_DOCS && dd < a.D) {
      a.new_off[dd] = (uint64_t)base + (x - v);
      if (dd == a.D - 1) a.new_off[a.D] = (uint64_t)base + x;
    }
  }
  __syncthreads();
  const uint32_t to = offs[w];
  for (uint32_t i = lane; i < cnt; i += 64) {  // (to + cnt <= the parts <= N)
    const uint8_t kc = a.s_kc[from + i];
    a.o_id[to + i] = a.s_id[from + i];
    a.o_cause[to + i] = a.s_cause[from + i];
    a.o_kind[to + i] = kc >> 2;
    if (a.o_cii) a.o_cii[to + i] = kc & 3u;
    if (a.o_src) a.o_src[to + i] = a.s_src[from + i];
  }
}

namespace {

// Adds to the algorithmic bytes of a launch of this call once its sizes are known.
void iv_add_bytes(cw_ctx *c, size_t rec, double bytes) {
  if (rec != NO_REC && rec < c->pending.size()) c->pending[rec].bytes += bytes;
}

// The general route: the staging columns, doc_stage / doc_end and base_cnt of
// every base by the stable key sort over the call's C candidates.
int invert_general(cw_ctx *c, const IvArgs &a, uint32_t C) {
  const uint64_t off[2] = {0, C};
  if (ensure_tables(c, 1, off)) return -1;
  uint64_t *kA = scratch_t<uint64_t>(c, "iv_kA", C), *kB = scratch_t<uint64_t>(c, "iv_kB", C);
  uint64_t *kC = scratch_t<uint64_t>(c, "iv_kC", C), *okey = scratch_t<uint64_t>(c, "iv_okey", C);
  uint32_t *vA = scratch_t<uint32_t>(c, "iv_vA", C), *vB = scratch_t<uint32_t>(c, "iv_vB", C);
  uint32_t *vC = scratch_t<uint32_t>(c, "iv_vC", C), *txi = scratch_t<uint32_t>(c, "iv_txi", C);
  uint8_t *head = scratch_t<uint8_t>(c, "iv_head", C);
  if (!kA || !kB || !kC || !okey || !vA || !vB || !vC || !txi || !head)
    return fail(c, "out of device memory (invert, general route)");
  const uint32_t blocks = (C + 255) / 256;
  uint64_t *ko = nullptr;
  uint32_t *vo = nullptr;
  // one link of a chain: the elements in the order `vin` (nullptr: input order)
  // sorted, stably, by the key `mode` makes (or by the array `direct`)
  auto sort_by = [&](int mode, const uint64_t *direct, uint32_t bits, const uint32_t *vin) -> int {
    const uint64_t *kin = direct;
    if (!direct) {
      Launch L(c, "k_iv_keys", (double)C * 24);
      hipLaunchKernelGGL(k_iv_keys, dim3(blocks), dim3(256), 0, c->stream, a, C, mode, vin, head, kC, vC);
      kin = kC;
      vin = vC;
    }
    if (check_launch(c, "k_iv_keys")) return -1;
    return radix_sort<uint64_t>(c, "iv_sort", kin, vin, kA, vA, kB, vB, bits, 0, C, &ko, &vo);
  };
  const uint32_t dbits = ceil_log2((uint64_t)a.D + 1), gbits = ceil_log2((uint64_t)a.G + 1);
  if (sort_by(0, a.c_id, 64, nullptr) || sort_by(IV_K_CAUSE, nullptr, 64, vo) ||
      sort_by(IV_K_DOCKEY, nullptr, dbits + 2, vo))
    return -1;
  {
    Launch L(c, "k_iv_runs", (double)C * 38);
    hipLaunchKernelGGL(k_iv_runs, dim3(blocks), dim3(256), 0, c->stream, a, C, vo, head, okey);
  }
  if (check_launch(c, "k_iv_runs")) return -1;
  if (sort_by(0, okey, 64, nullptr) || sort_by(IV_K_BASE, nullptr, std::max(gbits, 1u), vo)) return -1;
  {
    Launch L(c, "k_iv_txidx", (double)C * 17);
    hipLaunchKernelGGL(k_iv_txidx, dim3(blocks), dim3(256), 0, c->stream, a, C, vo, ko, head, txi);
  }
  if (check_launch(c, "k_iv_txidx")) return -1;
  if (sort_by(IV_K_DOC, nullptr, std::max(dbits, 1u), vo)) return -1;
  {
    Launch L(c, "k_iv_stage", (double)C * 55);
    hipLaunchKernelGGL(k_iv_stage, dim3(blocks), dim3(256), 0, c->stream, a, C, vo, head, txi);
  }
  return check_launch(c, "k_iv_stage");
}

int invert_impl(cw_ctx *c, const cw_invert_batch *b, cw_invert_result *r, int memspace) {
  if (!b || !r) return fail(c, "null batch/result");
  if (memspace != CW_MEM_HOST && memspace != CW_MEM_DEVICE) return fail(c, "bad memspace");
  const bool dev = memspace == CW_MEM_DEVICE;
  const uint64_t D = b->n_docs, G = b->n_bases;
  if (!b->doc_offsets || !b->base_offsets || !r->part_offsets)
    return fail(c, "doc_offsets, base_offsets and part_offsets are required (host memory)");
  if (b->site_bits < 1 || b->site_bits > 10) return fail(c, "site_bits %u outside 1..10", b->site_bits);
  if (b->site_shift > 63 || b->ts_shift > 63) return fail(c, "bad key layout");
  if (check_doc_offsets(c, b->doc_offsets, D, 0, 0)) return -1;
  const uint64_t *off = b->doc_offsets, *boff = b->base_offsets;
  if (boff[0] != 0) return fail(c, "base_offsets[0] must be 0");
  for (uint64_t g = 0; g < G; g++)
    if (boff[g + 1] < boff[g]) return fail(c, "base_offsets not monotone");
  if (boff[G] != D)
    return fail(c, "base_offsets[n_bases] = %llu, n_docs = %llu", (unsigned long long)boff[G], (unsigned long long)D);
  const uint64_t N = off[D];
  if (D >= 0xFFFFFFFFull || G >= 0xFFFFFFFFull) return fail(c, "batch too large: %llu documents", (unsigned long long)D);
  if (D && !r->status) return fail(c, "status is required");
  if (N && (!b->id_key || !b->cause || !b->kind || !r->inv_id || !r->inv_cause || !r->inv_kind))
    return fail(c, "null node or output columns");
  if (G && (!b->sel_lo || !b->sel_hi || !b->sel_sites || !b->new_tx)) return fail(c, "null selection arrays");
  if ((b->cause_is_id == nullptr) != (r->inv_cause_is_id == nullptr))
    return fail(c, "cause_is_id and inv_cause_is_id go together");
  HIPCHK(c, hipSetDevice(c->device));
  if (N == 0) {  // no nodes: no parts
    for (uint64_t d = 0; d <= D; d++) r->part_offsets[d] = 0;
    if (!dev) {
      if (D) memset(r->status, 0, D * 4);
      if (r->base_parts && G) memset(r->base_parts, 0, G * 4);
      return 0;
    }
    if (D) HIPCHK(c, hipMemsetAsync(r->status, 0, D * 4, c->stream));
    if (r->base_parts && G) HIPCHK(c, hipMemsetAsync(r->base_parts, 0, G * 4, c->stream));
    if (!c->async) HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  }
  auto &st = c->invert;
  const uint32_t tiles = (uint32_t)((N + IV_TILE - 1) / IV_TILE);
  const uint32_t wblocks = (uint32_t)((D + IV_WR_DOCS - 1) / IV_WR_DOCS);
  if (!grid_ok(tiles, IV_NT) || !grid_ok(wblocks, IV_WR_NT) || !grid_ok(G, 64))
    return fail(c, "batch too large for one dispatch");

  IvArgs a{};
  a.N = (uint32_t)N;
  a.D = (uint32_t)D;
  a.G = (uint32_t)G;
  a.tiles = tiles;
  a.id = b->id_key;
  a.cause = b->cause;
  a.kind = b->kind;
  a.cii = b->cause_is_id;
  a.ref = b->ref_doc;
  a.sel_lo = b->sel_lo;
  a.sel_hi = b->sel_hi;
  a.sel_sites = b->sel_sites;
  a.new_tx = b->new_tx;
  a.site_shift = b->site_shift;
  a.site_bits = b->site_bits;
  a.mask_words = ((1u << b->site_bits) + 63) / 64;
  a.wg = iv_lds_bytes(IV_CAP) <= c->lds_max ? 1u : 0u;
  a.cap = std::min(c->invert_cap, IV_CAP);
  a.o_id = r->inv_id;
  a.o_cause = r->inv_cause;
  a.o_cii = r->inv_cause_is_id;
  a.o_kind = r->inv_kind;
  a.o_src = r->inv_src;
  a.o_base_parts = r->base_parts;
  a.o_status = r->status;
  if (!dev) {  // uploads, and the outputs staged
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t mw = (size_t)G * a.mask_words * 8;
    if (upload(c, "iv_id", b->id_key, (size_t)N * 8, &a.id) || upload(c, "iv_cause", b->cause, (size_t)N * 8, &a.cause) ||
        upload(c, "iv_kind", b->kind, (size_t)N, &a.kind) || upload(c, "iv_lo", b->sel_lo, (size_t)G * 8, &a.sel_lo) ||
        upload(c, "iv_hi", b->sel_hi, (size_t)G * 8, &a.sel_hi) || upload(c, "iv_sites", b->sel_sites, mw, &a.sel_sites) ||
        upload(c, "iv_tx", b->new_tx, (size_t)G * 8, &a.new_tx))
      return -1;
    if (a.cii && upload(c, "iv_cii", b->cause_is_id, (size_t)N, &a.cii)) return -1;
    if (a.ref && upload(c, "iv_ref", b->ref_doc, (size_t)N * 4, &a.ref)) return -1;
    a.o_id = scratch_t<uint64_t>(c, "iv_oid", N);
    a.o_cause = scratch_t<uint64_t>(c, "iv_oca", N);
    a.o_kind = scratch_t<uint8_t>(c, "iv_okd", N);
    a.o_cii = a.cii ? scratch_t<uint8_t>(c, "iv_oci", N) : nullptr;
    a.o_src = r->inv_src ? scratch_t<uint32_t>(c, "iv_osrc", N) : nullptr;
    a.o_base_parts = r->base_parts ? scratch_t<uint32_t>(c, "iv_obp", G) : nullptr;
    a.o_status = scratch_t<uint32_t>(c, "iv_ost", D);
    if (!a.o_id || !a.o_cause || !a.o_kind || (a.cii && !a.o_cii) || (r->inv_src && !a.o_src) ||
        (r->base_parts && !a.o_base_parts) || !a.o_status)
      return fail(c, "out of device memory (host-mode staging)");
  }

  // the two layouts on the device, each cached while it repeats
  const char *n_off = "iv_off", *n_boff = "iv_boff";
  bool miss;
  if (device_layout(c, st.docs, D, off, nullptr, &n_off, nullptr, &a.doc_off, &miss) ||
      device_layout(c, st.bases, G, boff, nullptr, &n_boff, nullptr, &a.base_off, &miss))
    return -1;
  // per document: hidden, first and end slot (zero); per base: parts (zero), range; ctl (zero)
  uint32_t *dz = scratch_t<uint32_t>(c, "iv_doc", 3 * D), *gz = scratch_t<uint32_t>(c, "iv_base", 4 * G + 4);
  a.selw = scratch_t<uint32_t>(c, "iv_selw", (size_t)tiles * IV_NT);
  a.tile_sel = scratch_t<uint32_t>(c, "iv_tsel", tiles);
  a.tile_base = scratch_t<uint32_t>(c, "iv_tbase", (size_t)tiles + 1);
  a.c_id = scratch_t<uint64_t>(c, "iv_cid", N);
  a.c_cause = scratch_t<uint64_t>(c, "iv_cca", N);
  a.c_doc = scratch_t<uint32_t>(c, "iv_cdoc", N);
  a.c_src = scratch_t<uint32_t>(c, "iv_csrc", N);
  a.c_kc = scratch_t<uint8_t>(c, "iv_ckc", N);
  a.s_id = scratch_t<uint64_t>(c, "iv_sid", N);
  a.s_cause = scratch_t<uint64_t>(c, "iv_sca", N);
  a.s_src = scratch_t<uint32_t>(c, "iv_ssrc", N);
  a.s_kc = scratch_t<uint8_t>(c, "iv_skc", N);
  a.new_off = scratch_t<uint64_t>(c, "iv_noff", D + 1);
  if (!dz || !gz || !a.selw || !a.tile_sel || !a.tile_base || !a.c_id || !a.c_cause || !a.c_doc || !a.c_src ||
      !a.c_kc || !a.s_id || !a.s_cause || !a.s_src || !a.s_kc || !a.new_off)
    return fail(c, "out of device memory (invert)");
  a.hidden = dz;
  a.doc_stage = dz + D;
  a.doc_end = dz + 2 * D;
  a.base_cnt = gz;
  a.ctl = gz + G;
  a.base_lo = gz + G + 4;
  a.base_n = gz + 2 * G + 4;
  a.big = gz + 3 * G + 4;
  HIPCHK(c, hipMemsetAsync(dz, 0, 3 * D * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(gz, 0, (G + 4) * 4, c->stream));
  if (a.o_base_parts) HIPCHK(c, hipMemsetAsync(a.o_base_parts, 0, G * 4, c->stream));

  size_t rec_compact = NO_REC, rec_w = NO_REC, rec_write = NO_REC;
  {
    // per node its id, kind and ref_doc in and its bit out; per tile its documents, range and count
    Launch L(c, "k_invert_mark", (double)N * (9.125 + (a.ref ? 4 : 0)) + (double)tiles * 48);
    hipLaunchKernelGGL(k_invert_mark, dim3(tiles), dim3(IV_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_invert_mark")) return -1;
  a.lb = lookback_words(c, st.lb_tiles, "iv_lbt", tiles, 1, &a.epoch);
  if (!a.lb) return -1;
  {
    // per node its bit in and out; per candidate (added below) its columns in and its record out
    Launch L(c, "k_invert_compact", (double)N * 0.25 + (double)tiles * 24, nullptr, &rec_compact);
    hipLaunchKernelGGL(k_invert_compact, dim3(tiles), dim3(IV_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_invert_compact")) return -1;
  {
    // per base its offsets and two ranks (up to a tile's words each); per candidate its record in, per part out
    Launch L(c, "k_invert_base_w", (double)G * 32, nullptr, &rec_w);
    hipLaunchKernelGGL(k_invert_base_w, dim3((uint32_t)G), dim3(64), iv_lds_bytes(IV_CAP_W), c->stream, a);
  }
  if (check_launch(c, "k_invert_base_w")) return -1;
  if (a.wg && a.cap > IV_CAP_W) {
    Launch L(c, "k_invert_base_wg", (double)G * 4);
    hipLaunchKernelGGL(k_invert_base_wg, dim3((uint32_t)std::min<uint64_t>(G, c->n_cu)), dim3(IV_WG_NT),
                       iv_lds_bytes(IV_CAP), c->stream, a);
  }
  if (check_launch(c, "k_invert_base_wg")) return -1;
  uint32_t C = 0;
  for (int pass = 0;; pass++) {
    a.lb = lookback_words(c, st.lb_docs, "iv_lbd", wblocks, 1, &a.epoch);
    if (!a.lb) return -1;
    {
      // per document its slots, its base's count, status and offset; per part (added below) its columns in and out
      Launch L(c, "k_invert_write", (double)D * 28, nullptr, &rec_write);
      hipLaunchKernelGGL(k_invert_write, dim3(wblocks), dim3(IV_WR_NT), 0, c->stream, a);
    }
    if (check_launch(c, "k_invert_write")) return -1;
    // the call's one wait: the part offsets, with the route's control words
    HIPCHK(c, hipMemcpyAsync(r->part_offsets, a.new_off, (D + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    const uint32_t *ctl = read_small(c, a.ctl, 16);
    if (!ctl) return -1;
    C = ctl[2];
    const bool over = ctl[1] != 0;
    if (C > N) return fail(c, "internal: candidates past N");
    const double parts = (double)r->part_offsets[D] * (21 + (a.o_cii ? 1 : 0) + (a.o_src ? 4 : 0));
    iv_add_bytes(c, rec_write, 2 * parts);
    if (pass == 0) {
      iv_add_bytes(c, rec_compact, (double)C * (9 + 8 + (a.cii ? 1 : 0) + 25));
      iv_add_bytes(c, rec_w, (double)C * 25 + (over ? 0 : parts));
    }
    if (pass || !over) break;
    // a base above the cap: every base again, by the key sort (the second wait was the one above)
    HIPCHK(c, hipMemsetAsync(a.doc_stage, 0, 2 * D * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(a.base_cnt, 0, G * 4, c->stream));
    if (invert_general(c, a, C)) return -1;
  }
  const uint64_t P = r->part_offsets[D];
  if (P > C) return fail(c, "internal: parts past the candidates");
  if (!dev) {
    if (P) {
      HIPCHK(c, hipMemcpy(r->inv_id, a.o_id, P * 8, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(r->inv_cause, a.o_cause, P * 8, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(r->inv_kind, a.o_kind, P, hipMemcpyDeviceToHost));
      if (a.o_cii) HIPCHK(c, hipMemcpy(r->inv_cause_is_id, a.o_cii, P, hipMemcpyDeviceToHost));
      if (a.o_src) HIPCHK(c, hipMemcpy(r->inv_src, a.o_src, P * 4, hipMemcpyDeviceToHost));
    }
    if (a.o_base_parts && G) HIPCHK(c, hipMemcpy(r->base_parts, a.o_base_parts, G * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(r->status, a.o_status, D * 4, hipMemcpyDeviceToHost));
  }
  return c->prof ? collect_prof(c) : 0;
}

}  // namespace
