// mapinsert.hip -- cw_insert_maps (include/causeweave_map_insert.h): c.map/weave's
// 2/3-arity (map.cljc:29-45) over s/weave-node (shared.cljc:225-241) behind
// s/insert (shared.cljc:151-184), one transaction a collection, without a
// reweave.  Included by causeweave.hip after mapweft.hip (lookback.h).
//
// One kernel, k_map_insert<G>: a group of G lanes takes one collection -- G = 64,
// a wave a collection and four collections a workgroup, when every collection
// has n_d + k_d <= MPK nodes (and map_insert_wave = 1); G = 256, a workgroup a
// collection, for the whole call otherwise.  The same body serves both.
//
// No interim weave.  Tx node j's place is (key weave, gap g in the OLD key
// weave, rank r among the tx nodes of that gap): it sorts before old element g
// and behind old element g - 1.  Elements of the virtual key weave carry a
// 64-bit order word: old element i is i << 32 | 0xFFFFFFFF, a tx node g << 32 | r.
//
//   1. one strided scan of the collection's ids: is the first tx id a node (and
//      which), and which node does every id cause name (old nodes, then the tx);
//      the validation of the first tx node; key tokens >= 2^62;
//   2. the key word of every tx node and, by a binary search of the collection's
//      seg_key run, its key weave or the place of a new one.  The collection's
//      run is found by two binary searches of seg_coll (a boundary pass over
//      seg_coll would be one more kernel and one more array per call);
//   3. step j = 0 .. k-1: E = the first element whose id is nm's cause-in-weave,
//      F = the first whose cause-in-weave is nm's id, A = min(E + 1, F) (order
//      words are distinct integers, so "behind E" is ">= E + 1"), P = the first
//      element >= A that is not later, each a min-reduction over the old key weave
//      (read through the old seg_perm, the group in parallel) and the earlier tx
//      nodes of the same key weave.  nm takes P's gap: behind the tx nodes of the
//      gap when P is old, at P's rank when P is a tx node (the ranks >= it move
//      up), the end when there is no P.  A key or nil cause has E = the root and
//      skips the first two reductions;
//   4. the insertions -- k tx nodes and a root per new key weave -- are ranked by
//      (old position they go before, new key weaves behind appends, key, place)
//      and get their final positions; the group's two counts (accepted tx nodes,
//      new key weaves) are published and numbered across the batch by two
//      decoupled look-backs (lookback.h): both are known before any wait;
//   5. every output straight to its final place: a lane of the new seg_perm run
//      finds its source by counting the insertions before it (a binary search of
//      the <= 2 k final positions); seg_offsets / seg_coll / seg_key likewise;
//      seg_active of a touched key weave by active-node (map.cljc:47-59) over
//      the new run, an untouched one keeps its word; tx_seg / tx_pos, status, the
//      new offsets and n_segs, the output columns.
//
// The plan is 18 words a tx node: in LDS for a tx of <= 32 (G = 64) or <= 128
// (G = 256) nodes, in a scratch array of the context otherwise.
// Nothing is read or written outside the caller's arrays whatever the seg
// arrays hold: every index taken from them is checked, and the outputs are
// produced per output position of the collection's own run.

constexpr uint32_t MI_NT = 256;
constexpr uint32_t MI_PW = 18;             // plan words a tx node
constexpr uint32_t MI_LDS_TX = 128;        // tx nodes a workgroup keeps in LDS
constexpr uint32_t MI_NONE = 0xFFFFFFFFu;
constexpr uint32_t MI_NEW = 0x80000000u;   // plan: a new key weave | its place among the old ones
constexpr uint32_t MI_ROOT = 0x80000000u;  // item: the root of tx node (low bits)'s new key weave
constexpr uint64_t MI_INF = ~0ull;

struct MiArgs {
  uint32_t D, N, S;  // collections, old nodes, old key weaves
  const uint32_t *coll_off, *tx_off;  // device [D + 1]
  const uint64_t *id, *cause;
  const uint8_t *cis, *kind;
  const uint64_t *value;
  const uint64_t *seg_off;
  const uint32_t *seg_coll;
  const uint64_t *seg_key;
  const int64_t *seg_active;
  const uint32_t *seg_perm;
  const uint64_t *tx_id, *tx_cause;
  const uint8_t *tx_cis, *tx_kind;
  const uint64_t *tx_value;
  uint64_t *new_off;  // device [D + 2]: the new offsets, then n_segs
  uint32_t *o_txseg, *o_txpos;
  uint64_t *o_seg_off;
  uint32_t *o_seg_coll;
  uint64_t *o_seg_key;
  int64_t *o_seg_active;
  uint32_t *o_seg_perm, *o_status;
  uint64_t *o_id, *o_cause;
  uint8_t *o_cis, *o_kind;
  uint64_t *o_value;
  uint32_t *gplan;  // [T * MI_PW]: the plans of txs too long for LDS
  unsigned long long *lb;  // look-back words: accepted tx nodes [blocks], new key weaves [blocks]
  uint32_t epoch, blocks;
};

// The group's barrier: its plan words (LDS or scratch) written before are read after.
template <int G>
__device__ __forceinline__ void mi_sync() {
  if (G == 64) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

template <int G>
__device__ __forceinline__ uint64_t mi_min64(uint64_t v, uint64_t *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t x = __shfl_xor((unsigned long long)v, o, 64);
    v = x < v ? x : v;
  }
  if (G != 64) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    for (uint32_t w = 0; w < G / 64; w++) v = red[w] < v ? red[w] : v;
  }
  return v;
}

template <int G>
__device__ __forceinline__ uint32_t mi_sum(uint32_t v, uint64_t *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (G != 64) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0;
    for (uint32_t w = 0; w < G / 64; w++) v += (uint32_t)red[w];
  }
  return v;
}

// the first index of [0, n) whose word is >= x (n when there is none)
template <typename T>
__device__ __forceinline__ uint32_t mi_lower(const T *p, uint32_t n, T x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (p[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// weave-later? (shared.cljc:202-223) of nm = (nid, special sm) against nr = (rid, its cause-in-weave, kind)
__device__ __forceinline__ bool mi_later(uint64_t nid, bool sm, uint64_t rid, uint64_t rciw, uint8_t rkd) {
  const bool sr = is_special(rkd), lt = nid < rid;
  return (sr && nid != rciw && (!sm || lt)) || (lt && (!sm || sr));
}

// A collection as its group sees it (all wave-uniform).
struct MiColl {
  uint32_t o, n, t0, k, kk;  // first node, nodes, first tx node, tx nodes, accepted tx nodes
  uint32_t s0, ns;           // first key weave, key weaves
  uint32_t P0, L;            // first old seg_perm position, old run length
  uint32_t cnt, nnew;        // insertions, new key weaves
};

// The plan of a collection's tx (cap = k words per row).
struct MiPlan {
  uint64_t *kw;  // [k] key word
  uint32_t *g, *r, *ci, *ws;  // [k] gap, rank, the cause's node (local index, n + tx node), key weave
  uint32_t *it_c, *it_sub;    // [2k] insertion x: the old position it goes before (its final position after
                              // the ranking); new key weave << 31 | place.  x < k: tx node x, x >= k: the
                              // root of tx node x - k's new key weave (MI_NONE: no such root)
  uint32_t *s_fp, *s_it, *s_c;  // [2k] by rank: final position, insertion, old position
  uint32_t *ns_idx, *ns_lead;   // [k] new key weaves by key: new local index, first tx node
};

__device__ __forceinline__ MiPlan mi_plan(uint32_t *pl, uint32_t k) {
  MiPlan p;
  p.kw = reinterpret_cast<uint64_t *>(pl);
  p.g = pl + 2 * k;
  p.r = pl + 3 * k;
  p.ci = pl + 4 * k;
  p.ws = pl + 5 * k;
  p.it_c = pl + 6 * k;
  p.it_sub = pl + 8 * k;
  p.s_fp = pl + 10 * k;
  p.s_it = pl + 12 * k;
  p.s_c = pl + 14 * k;
  p.ns_idx = pl + 16 * k;
  p.ns_lead = pl + 17 * k;
  return p;
}

// the old seg_offsets word s (global key weave), as a position of the collection's old run
__device__ __forceinline__ uint32_t mi_segpos(const MiArgs &a, const MiColl &c, uint32_t s) {
  const uint64_t v = a.seg_off[s];
  return v >= c.P0 && v - c.P0 <= c.L ? (uint32_t)(v - c.P0) : c.L;
}

// the new seg_perm word at position q of the collection's new run
__device__ __forceinline__ uint32_t mi_value_at(const MiArgs &a, const MiColl &c, const MiPlan &p, uint32_t q) {
  const uint32_t m = mi_lower<uint32_t>(p.s_fp, c.cnt, q);
  if (m < c.cnt && p.s_fp[m] == q) {
    const uint32_t it = p.s_it[m];
    return (it & MI_ROOT) ? MI_NONE : c.n + it;
  }
  const uint32_t x = q - m;
  return x < c.L && (uint64_t)c.P0 + x < (uint64_t)a.N + a.S ? a.seg_perm[c.P0 + x] : MI_NONE;
}

// the kind of the node a seg_perm word names (a root or a stray word: passed over like a special)
__device__ __forceinline__ uint8_t mi_kind_of(const MiArgs &a, const MiColl &c, uint32_t v) {
  if (v < c.n) return a.kind[c.o + v];
  if (v - c.n < c.k) return a.tx_kind[c.t0 + (v - c.n)];
  return 3;
}

// where tx node j's key weave starts in the new run, and its new local index
__device__ __forceinline__ void mi_weave_of(const MiArgs &a, const MiColl &c, const MiPlan &p, uint32_t j,
                                            uint32_t *seg, uint32_t *start) {
  const uint32_t ws = p.ws[j];
  if (ws & MI_NEW) {
    const uint64_t kw = p.kw[j];
    uint32_t m = 0;
    while (m + 1 < c.nnew && p.kw[p.ns_lead[m]] != kw) m++;
    *seg = p.ns_idx[m];
    *start = p.it_c[c.k + p.ns_lead[m]];
  } else {
    uint32_t before = 0;
    for (uint32_t m = 0; m < c.nnew; m++) before += (p.ws[p.ns_lead[m]] & ~MI_NEW) <= ws;
    *seg = ws + before;
    const uint32_t x = mi_segpos(a, c, c.s0 + ws);
    *start = x + mi_lower<uint32_t>(p.s_c, c.cnt, x + 1);
  }
}

template <int G>
__global__ __launch_bounds__(MI_NT) void k_map_insert(MiArgs a) {
  constexpr uint32_t GP = MI_NT / G, KL = MI_LDS_TX / GP;
  __shared__ uint64_t s_plan[GP][KL * MI_PW / 2];
  __shared__ uint64_t s_red[4];
  __shared__ uint32_t s_cnt[GP][2], s_base[2];

  const uint32_t tid = threadIdx.x, grp = tid / G, gl = tid % G, lane = tid & 63;
  const uint32_t d = blockIdx.x * GP + grp;
  const bool live = d < a.D;
  const uint32_t NS = a.N + a.S < a.N ? MI_NONE : a.N + a.S;  // the old seg_perm's size

  MiColl c{};
  MiPlan p{};
  uint32_t status = 0;
  if (live) {
    c.o = a.coll_off[d];
    c.n = a.coll_off[d + 1] - c.o;
    c.t0 = a.tx_off[d];
    c.k = a.tx_off[d + 1] - c.t0;
    {  // the collection's key weaves: two searches of seg_coll, a lane each
      uint32_t f = 0;
      if (lane < 2) f = mi_lower<uint32_t>(a.seg_coll, a.S, d + lane);
      c.s0 = __shfl(f, 0, 64);
      const uint32_t s1 = __shfl(f, 1, 64);
      c.ns = s1 > c.s0 ? s1 - c.s0 : 0;
    }
    c.L = c.n + c.ns;
    if (c.ns) {
      const uint64_t v = a.seg_off[c.s0];
      c.P0 = v < NS ? (uint32_t)v : NS;
    }
    if (c.L > NS - c.P0) c.L = NS - c.P0;
    uint32_t *pl = c.k <= KL ? reinterpret_cast<uint32_t *>(s_plan[grp]) : a.gplan + (size_t)c.t0 * MI_PW;
    p = mi_plan(pl, c.k);

    // ---- 1. the scan of the ids, the validation
    for (uint32_t j = gl; j < c.k; j += G) p.ci[j] = MI_NONE;
    mi_sync<G>();
    uint32_t dup = MI_NONE;
    const uint64_t id0 = c.k ? a.tx_id[c.t0] : 0;
    for (uint32_t s = gl; s < c.n && c.k; s += G) {
      const uint64_t id = a.id[c.o + s];
      if (id == id0) dup = s;
      for (uint32_t j = 0; j < c.k; j++)
        if (a.tx_cis[c.t0 + j] == 1 && a.tx_cause[c.t0 + j] == id) p.ci[j] = s;
    }
    dup = (uint32_t)mi_min64<G>(dup, s_red);
    mi_sync<G>();
    bool accept = c.k > 0;
    if (c.k) {
      const uint8_t c0 = a.tx_cis[c.t0];
      if (dup != MI_NONE) {  // shared.cljc:164-171
        accept = false;
        bool same = a.cis[c.o + dup] == c0 && a.kind[c.o + dup] == a.tx_kind[c.t0] &&
                    (c0 == 2 || a.cause[c.o + dup] == a.tx_cause[c.t0]);
        if (a.value && a.value[c.o + dup] != a.tx_value[c.t0]) same = false;
        if (!same) status = CW_STATUS_DUP;
      } else if (c0 == 2 || (c0 == 1 && p.ci[0] == MI_NONE)) {  // :175-178, before the tx joins ::nodes
        accept = false;
        status = CW_STATUS_ORPHAN;
      }
    }
    if (accept) {
      uint32_t bad = 0;
      for (uint32_t j = gl; j < c.k; j += G)
        bad += a.tx_cis[c.t0 + j] == 0 && a.tx_cause[c.t0 + j] >= (1ull << 62);
      if (mi_sum<G>(bad, s_red)) {
        accept = false;
        status = CW_STATUS_MAP_KEY;
      }
    }
    c.kk = accept ? c.k : 0;

    // ---- 2. the key words and their key weaves
    for (uint32_t j = gl; j < c.kk; j += G) {
      const uint8_t ci = a.tx_cis[c.t0 + j];
      const uint64_t ca = a.tx_cause[c.t0 + j];
      uint64_t kw = CW_NIL;
      if (ci == 0) {
        kw = ca;
      } else if (ci == 1) {
        uint32_t at = p.ci[j];
        if (at == MI_NONE)  // ... among the tx nodes, earlier or later
          for (uint32_t i = 0; i < c.k; i++)
            if (a.tx_id[c.t0 + i] == ca) {
              at = c.n + i;
              break;
            }
        if (at != MI_NONE) {
          const bool old = at < c.n;
          const uint8_t cci = old ? a.cis[c.o + at] : a.tx_cis[c.t0 + (at - c.n)];
          const uint64_t cca = old ? a.cause[c.o + at] : a.tx_cause[c.t0 + (at - c.n)];
          kw = cci == 0 ? cca : cci == 1 ? (CW_MAP_ID_KEY | cca) : CW_NIL;
        }
      }
      const uint32_t lo = mi_lower<uint64_t>(a.seg_key + c.s0, c.ns, kw);
      p.kw[j] = kw;
      p.ws[j] = lo < c.ns && a.seg_key[c.s0 + lo] == kw ? lo : (MI_NEW | lo);
    }
    mi_sync<G>();

    // ---- 3. the steps
    for (uint32_t j = 0; j < c.kk; j++) {
      const uint64_t kwj = p.kw[j], nid = a.tx_id[c.t0 + j];
      const uint32_t ws = p.ws[j];
      const uint64_t ciw = a.tx_cis[c.t0 + j] == 1 ? a.tx_cause[c.t0 + j] : 0;
      const bool sm = is_special(a.tx_kind[c.t0 + j]);
      uint32_t so = 0, len = 1;  // the old key weave: its first position in the old run, its length with the root
      if (!(ws & MI_NEW)) {
        so = mi_segpos(a, c, c.s0 + ws);
        const uint32_t se = mi_segpos(a, c, c.s0 + ws + 1);
        len = se > so ? se - so : 1;
      }
      const uint32_t *perm = a.seg_perm + c.P0 + so;
      uint64_t A = 1ull << 32;  // a key or nil cause: behind the root
      if (ciw != 0) {
        uint64_t E = MI_INF, F = MI_INF;
        for (uint32_t i = 1 + gl; i < len; i += G) {
          const uint32_t s = perm[i];
          if (s >= c.n) continue;
          const uint64_t ord = (uint64_t)i << 32 | 0xFFFFFFFFu;
          const uint64_t rid = a.id[c.o + s], rciw = a.cis[c.o + s] == 1 ? a.cause[c.o + s] : 0;
          if (rid == ciw && ord < E) E = ord;
          if (rciw == nid && ord < F) F = ord;
        }
        for (uint32_t i = gl; i < j; i += G) {
          if (p.kw[i] != kwj) continue;
          const uint64_t ord = (uint64_t)p.g[i] << 32 | p.r[i];
          const uint64_t rid = a.tx_id[c.t0 + i], rciw = a.tx_cis[c.t0 + i] == 1 ? a.tx_cause[c.t0 + i] : 0;
          if (rid == ciw && ord < E) E = ord;
          if (rciw == nid && ord < F) F = ord;
        }
        E = mi_min64<G>(E, s_red);
        F = mi_min64<G>(F, s_red);
        A = E == MI_INF ? MI_INF : E + 1;
        A = F < A ? F : A;
      }
      uint64_t P = MI_INF;
      if (A != MI_INF) {
        const uint32_t i0 = (uint32_t)(A >> 32) > 1 ? (uint32_t)(A >> 32) : 1;  // old i is >= A from A's gap on
        for (uint32_t i = i0 + gl; i < len; i += G) {
          const uint32_t s = perm[i];
          if (s >= c.n) continue;
          const uint64_t rid = a.id[c.o + s], rciw = a.cis[c.o + s] == 1 ? a.cause[c.o + s] : 0;
          if (!mi_later(nid, sm, rid, rciw, a.kind[c.o + s])) {
            P = (uint64_t)i << 32 | 0xFFFFFFFFu;
            break;
          }
        }
        for (uint32_t i = gl; i < j; i += G) {
          if (p.kw[i] != kwj) continue;
          const uint64_t ord = (uint64_t)p.g[i] << 32 | p.r[i];
          if (ord < A || ord >= P) continue;
          const uint64_t rciw = a.tx_cis[c.t0 + i] == 1 ? a.tx_cause[c.t0 + i] : 0;
          if (!mi_later(nid, sm, a.tx_id[c.t0 + i], rciw, a.tx_kind[c.t0 + i])) P = ord;
        }
        P = mi_min64<G>(P, s_red);
      }
      // nm goes just before P
      const uint32_t g = P == MI_INF ? len : (uint32_t)(P >> 32);
      const bool at_tx = P != MI_INF && (uint32_t)P != 0xFFFFFFFFu;
      uint32_t r = at_tx ? (uint32_t)P : 0, behind = 0;
      for (uint32_t i = gl; i < j; i += G) {
        if (p.kw[i] != kwj || p.g[i] != g) continue;
        if (at_tx) {
          if (p.r[i] >= r) p.r[i]++;
        } else {
          behind++;
        }
      }
      if (!at_tx) r = mi_sum<G>(behind, s_red);
      if (gl == 0) {
        p.g[j] = g;
        p.r[j] = r;
      }
      mi_sync<G>();
    }

    // ---- 4. the insertions: what they go before, their ranks, their final positions
    uint32_t lead = 0;
    for (uint32_t j = gl; j < c.kk; j += G) {
      const uint32_t ws = p.ws[j];
      uint32_t root = MI_NONE;
      if (ws & MI_NEW) {
        const uint32_t ip = ws & ~MI_NEW;
        const uint32_t at = ip < c.ns ? mi_segpos(a, c, c.s0 + ip) : c.L;
        p.it_c[j] = at;
        p.it_sub[j] = MI_NEW | (1 + p.r[j]);
        const uint64_t kw = p.kw[j];
        bool first = true;
        for (uint32_t i = 0; i < j; i++) first = first && p.kw[i] != kw;
        if (first) {
          root = at;
          lead++;
        }
      } else {
        p.it_c[j] = mi_segpos(a, c, c.s0 + ws) + p.g[j];
        p.it_sub[j] = p.r[j];
      }
      p.it_c[c.k + j] = root;
      p.it_sub[c.k + j] = MI_NEW;
    }
    c.nnew = mi_sum<G>(lead, s_red);
    c.cnt = c.kk + c.nnew;
    mi_sync<G>();
    for (uint32_t x = gl; x < 2 * c.kk; x += G) {
      const uint32_t xj = x < c.kk ? x : c.k + (x - c.kk);  // the rows of the tx nodes, then of the roots
      const uint32_t xc = p.it_c[xj];
      if (xc == MI_NONE) continue;
      const uint32_t xs = p.it_sub[xj];
      const uint64_t xk = p.kw[xj < c.k ? xj : xj - c.k];
      uint32_t rank = 0, lrank = 0;
      for (uint32_t y = 0; y < 2 * c.kk; y++) {
        const uint32_t yj = y < c.kk ? y : c.k + (y - c.kk);
        const uint32_t yc = p.it_c[yj];
        if (yc == MI_NONE) continue;
        const uint32_t ys = p.it_sub[yj];
        const uint64_t yk = p.kw[yj < c.k ? yj : yj - c.k];
        bool less;
        if (yc != xc) less = yc < xc;
        else if ((ys ^ xs) & MI_NEW) less = !(ys & MI_NEW);
        else if (yk != xk) less = yk < xk;
        else if (ys != xs) less = ys < xs;
        else less = y < x;
        rank += less;
        lrank += yj >= c.k && yk < xk;  // new key weaves with a smaller key
      }
      p.s_fp[rank] = xc + rank;
      p.s_it[rank] = xj < c.k ? xj : (MI_ROOT | (xj - c.k));
      p.s_c[rank] = xc;
      if (xj >= c.k) {
        p.ns_idx[lrank] = (p.ws[xj - c.k] & ~MI_NEW) + lrank;
        p.ns_lead[lrank] = xj - c.k;
      }
    }
    mi_sync<G>();
    for (uint32_t m = gl; m < c.cnt; m += G) {  // it_c: from now the final position
      const uint32_t it = p.s_it[m];
      p.it_c[(it & MI_ROOT) ? c.k + (it & ~MI_ROOT) : it] = p.s_fp[m];
    }
    mi_sync<G>();
    if (gl == 0) {
      s_cnt[grp][0] = c.kk;
      s_cnt[grp][1] = c.nnew;
    }
  } else if (gl == 0) {
    s_cnt[grp][0] = 0;
    s_cnt[grp][1] = 0;
  }
  __syncthreads();
  if (tid < 64) {  // publish, then look back
    uint32_t ca = 0, cb = 0;
    for (uint32_t g2 = 0; g2 < GP; g2++) {
      ca += s_cnt[g2][0];
      cb += s_cnt[g2][1];
    }
    unsigned long long *lb2 = a.lb + a.blocks;
    if (tid == 0) {
      lb_publish(a.lb, blockIdx.x, a.epoch, ca);
      lb_publish(lb2, blockIdx.x, a.epoch, cb);
    }
    const uint32_t ba = lb_exclusive(a.lb, blockIdx.x, a.epoch, ca);
    const uint32_t bb = lb_exclusive(lb2, blockIdx.x, a.epoch, cb);
    if (tid == 0) {
      s_base[0] = ba;
      s_base[1] = bb;
    }
  }
  __syncthreads();
  if (!live) return;
  uint32_t ba = s_base[0], bb = s_base[1];
  for (uint32_t g2 = 0; g2 < grp; g2++) {
    ba += s_cnt[g2][0];
    bb += s_cnt[g2][1];
  }

  // ---- 5. the outputs
  const uint32_t no = c.o + ba;         // the collection's first new node
  const uint32_t S0 = c.s0 + bb;        // ... and key weave
  const uint32_t nsn = c.ns + c.nnew;   // its key weaves
  const uint32_t Ln = c.n + c.kk + nsn;  // its new run
  const uint64_t Q0 = (uint64_t)no + S0;
  if (gl == 0) {
    if (d == 0) a.new_off[0] = 0;
    a.new_off[d + 1] = (uint64_t)no + c.n + c.kk;
    a.o_status[d] = status;
    if (d == a.D - 1) {
      a.new_off[a.D + 1] = S0 + nsn;
      a.o_seg_off[S0 + nsn] = Q0 + Ln;
    }
  }
  for (uint32_t q = gl; q < Ln; q += G) a.o_seg_perm[Q0 + q] = mi_value_at(a, c, p, q);
  for (uint32_t s = gl; s < nsn; s += G) {
    const uint32_t m = mi_lower<uint32_t>(p.ns_idx, c.nnew, s);
    if (m < c.nnew && p.ns_idx[m] == s) {  // a new key weave: its active node below
      const uint32_t j = p.ns_lead[m];
      a.o_seg_off[S0 + s] = Q0 + p.it_c[c.k + j];
      a.o_seg_key[S0 + s] = p.kw[j];
    } else {
      const uint32_t os = s - m, x = mi_segpos(a, c, c.s0 + os);
      a.o_seg_off[S0 + s] = Q0 + x + mi_lower<uint32_t>(p.s_c, c.cnt, x + 1);
      a.o_seg_key[S0 + s] = a.seg_key[c.s0 + os];
      bool touched = false;
      for (uint32_t j = 0; j < c.kk; j++) touched = touched || p.ws[j] == os;
      if (!touched) a.o_seg_active[S0 + s] = a.seg_active[c.s0 + os];
    }
    a.o_seg_coll[S0 + s] = d;
  }
  for (uint32_t j = gl; j < c.k; j += G) {
    uint32_t seg = MI_NONE, pos = MI_NONE;
    if (j < c.kk) {
      uint32_t start;
      mi_weave_of(a, c, p, j, &seg, &start);
      seg += S0;
      pos = p.it_c[j] - start;
    }
    if (a.o_txseg) a.o_txseg[c.t0 + j] = seg;
    if (a.o_txpos) a.o_txpos[c.t0 + j] = pos;
  }
  // active-node (map.cljc:47-59) of every touched key weave, at its first tx node
  for (uint32_t j = 0; j < c.kk; j++) {
    const uint64_t kwj = p.kw[j];
    bool first = true;
    uint32_t mine = 1;
    for (uint32_t i = 0; i < c.kk; i++) {
      if (i == j || p.kw[i] != kwj) continue;
      if (i < j) first = false;
      mine++;
    }
    if (!first) continue;
    const uint32_t ws = p.ws[j];
    uint32_t seg, start, len = 1 + mine;
    mi_weave_of(a, c, p, j, &seg, &start);
    if (!(ws & MI_NEW)) {
      const uint32_t so = mi_segpos(a, c, c.s0 + ws), se = mi_segpos(a, c, c.s0 + ws + 1);
      len = (se > so ? se - so : 1) + mine;
    }
    if (len > Ln - start) len = start < Ln ? Ln - start : 0;
    uint32_t act = MI_NONE;  // the first position that is no special and has no hide behind it
    for (uint32_t q = 1 + gl; q < len; q += G) {
      if (is_special(mi_kind_of(a, c, mi_value_at(a, c, p, start + q)))) continue;
      if (q + 1 < len && is_hide(mi_kind_of(a, c, mi_value_at(a, c, p, start + q + 1)))) continue;
      act = q;
      break;
    }
    act = (uint32_t)mi_min64<G>(act, s_red);
    if (gl == 0) {
      int64_t v = -1;
      if (act != MI_NONE && !(len > 1 && is_hide(mi_kind_of(a, c, mi_value_at(a, c, p, start + 1)))))
        v = mi_value_at(a, c, p, start + act);
      a.o_seg_active[S0 + seg] = v;
    }
  }
  if (a.o_id) {  // the columns: old nodes in input order, then the accepted tx
    for (uint32_t q = gl; q < c.n + c.kk; q += G) {
      const bool old = q < c.n;
      const uint64_t at = old ? (uint64_t)c.o + q : (uint64_t)c.t0 + (q - c.n);
      a.o_id[no + q] = old ? a.id[at] : a.tx_id[at];
      a.o_cause[no + q] = old ? a.cause[at] : a.tx_cause[at];
      a.o_cis[no + q] = old ? a.cis[at] : a.tx_cis[at];
      a.o_kind[no + q] = old ? a.kind[at] : a.tx_kind[at];
      if (a.o_value) a.o_value[no + q] = old ? a.value[at] : a.tx_value[at];
    }
  }
}

namespace {

int insert_maps_impl(cw_ctx *c, const cw_map_insert_batch *b, cw_map_insert_result *r, int memspace) {
  if (!b || !r) return fail(c, "null batch/result");
  if (memspace != CW_MEM_HOST && memspace != CW_MEM_DEVICE) return fail(c, "bad memspace");
  const bool dev = memspace == CW_MEM_DEVICE;
  const uint64_t D = b->colls.n_colls, S = b->n_segs;
  const uint64_t *off = b->colls.coll_offsets, *toff = b->tx_offsets;
  if (!off || !toff || !r->new_offsets)
    return fail(c, "coll_offsets, tx_offsets and new_offsets are required (host memory)");
  if (off[0] != 0 || toff[0] != 0) return fail(c, "coll_offsets[0] and tx_offsets[0] must be 0");
  uint64_t largest = 0, kmax = 0;
  for (uint64_t d = 0; d < D; d++) {
    if (off[d + 1] < off[d]) return fail(c, "coll_offsets not monotone");
    if (toff[d + 1] < toff[d]) return fail(c, "tx_offsets not monotone");
    largest = std::max(largest, (off[d + 1] - off[d]) + (toff[d + 1] - toff[d]));
    kmax = std::max(kmax, toff[d + 1] - toff[d]);
  }
  const uint64_t N = off[D], T = toff[D];
  if (N + T >= 0xFFFFFFFFull || S + T >= 0xFFFFFFFFull || N + S + T >= 0xFFFFFFFFull || D >= 0xFFFFFFFFull)
    return fail(c, "batch too large: N+T=%llu, n_segs+T=%llu (limit 2^32-1)", (unsigned long long)(N + T),
                (unsigned long long)(S + T));
  const cw_map_batch &m = b->colls;
  if ((N || S) && (!m.id_key || !m.cause || !m.cause_is_id || !m.kind || !b->seg_offsets || !b->seg_coll ||
                   !b->seg_key || !b->seg_active || !b->seg_perm))
    return fail(c, "null input arrays");
  if (T && (!b->tx_id || !b->tx_cause || !b->tx_cause_is_id || !b->tx_kind)) return fail(c, "null tx arrays");
  if ((b->coll_value == nullptr) != (b->tx_value == nullptr))
    return fail(c, "coll_value and tx_value go together");
  const int cols = (r->id_key != nullptr) + (r->cause != nullptr) + (r->cause_is_id != nullptr) + (r->kind != nullptr);
  if (cols != 0 && cols != 4)
    return fail(c, "output columns id_key, cause, cause_is_id, kind: all four or none");
  if (r->value && (!cols || !b->coll_value)) return fail(c, "value goes with the output columns and coll_value");
  cw_map_result &res = r->maps;
  if (!res.seg_offsets || !res.seg_coll || !res.seg_key || !res.seg_active || !res.seg_perm || !res.status)
    return fail(c, "null output arrays");
  if (res.cap_segs < S + T)
    return fail(c, "cap_segs %llu below n_segs + T = %llu", (unsigned long long)res.cap_segs,
                (unsigned long long)(S + T));
  if (D == 0) {
    r->new_offsets[0] = 0;
    res.n_segs = 0;
    return 0;
  }
  HIPCHK(c, hipSetDevice(c->device));
  auto &st = c->minsert;
  const bool wave = c->map_insert_wave && largest <= MPK;
  const uint32_t gp = wave ? MI_NT / 64 : 1, blocks = (uint32_t)((D + gp - 1) / gp);
  if (!grid_ok(blocks, MI_NT)) return fail(c, "batch too large for one dispatch");

  MiArgs a{};
  a.D = (uint32_t)D;
  a.N = (uint32_t)N;
  a.S = (uint32_t)S;
  a.id = m.id_key;
  a.cause = m.cause;
  a.cis = m.cause_is_id;
  a.kind = m.kind;
  a.value = b->coll_value;
  a.seg_off = b->seg_offsets;
  a.seg_coll = b->seg_coll;
  a.seg_key = b->seg_key;
  a.seg_active = b->seg_active;
  a.seg_perm = b->seg_perm;
  a.tx_id = b->tx_id;
  a.tx_cause = b->tx_cause;
  a.tx_cis = b->tx_cause_is_id;
  a.tx_kind = b->tx_kind;
  a.tx_value = b->tx_value;
  a.o_txseg = r->tx_seg;
  a.o_txpos = r->tx_pos;
  a.o_seg_off = res.seg_offsets;
  a.o_seg_coll = res.seg_coll;
  a.o_seg_key = res.seg_key;
  a.o_seg_active = res.seg_active;
  a.o_seg_perm = res.seg_perm;
  a.o_status = res.status;
  a.o_id = r->id_key;
  a.o_cause = r->cause;
  a.o_cis = r->cause_is_id;
  a.o_kind = r->kind;
  a.o_value = r->value;
  const uint64_t NTs = std::max<uint64_t>(N + T, 1), Ts = std::max<uint64_t>(T, 1);
  cw_map_result dres{};
  if (!dev) {  // uploads, and the outputs staged
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (upload(c, "ms_id", m.id_key, (size_t)N * 8, &a.id) || upload(c, "ms_cause", m.cause, (size_t)N * 8, &a.cause) ||
        upload(c, "ms_cis", m.cause_is_id, (size_t)N, &a.cis) || upload(c, "ms_kind", m.kind, (size_t)N, &a.kind) ||
        upload(c, "ms_so", b->seg_offsets, (size_t)(S || N ? S + 1 : 0) * 8, &a.seg_off) ||
        upload(c, "ms_sc", b->seg_coll, (size_t)S * 4, &a.seg_coll) ||
        upload(c, "ms_sk", b->seg_key, (size_t)S * 8, &a.seg_key) ||
        upload(c, "ms_sa", b->seg_active, (size_t)S * 8, &a.seg_active) ||
        upload(c, "ms_sp", b->seg_perm, (size_t)(N + S) * 4, &a.seg_perm) ||
        upload(c, "ms_txid", b->tx_id, (size_t)T * 8, &a.tx_id) ||
        upload(c, "ms_txca", b->tx_cause, (size_t)T * 8, &a.tx_cause) ||
        upload(c, "ms_txci", b->tx_cause_is_id, (size_t)T, &a.tx_cis) ||
        upload(c, "ms_txkd", b->tx_kind, (size_t)T, &a.tx_kind))
      return -1;
    if (a.value && (upload(c, "ms_val", b->coll_value, (size_t)N * 8, &a.value) ||
                    upload(c, "ms_txval", b->tx_value, (size_t)T * 8, &a.tx_value)))
      return -1;
    if (stage_map_result(c, res, N + T, D, &dres)) return -1;
    a.o_seg_off = dres.seg_offsets;
    a.o_seg_coll = dres.seg_coll;
    a.o_seg_key = dres.seg_key;
    a.o_seg_active = dres.seg_active;
    a.o_seg_perm = dres.seg_perm;
    a.o_status = dres.status;
    if (r->tx_seg) a.o_txseg = scratch_t<uint32_t>(c, "ms_otseg", Ts);
    if (r->tx_pos) a.o_txpos = scratch_t<uint32_t>(c, "ms_otpos", Ts);
    if (cols) {
      a.o_id = scratch_t<uint64_t>(c, "ms_oid", NTs);
      a.o_cause = scratch_t<uint64_t>(c, "ms_oca", NTs);
      a.o_cis = scratch_t<uint8_t>(c, "ms_oci", NTs);
      a.o_kind = scratch_t<uint8_t>(c, "ms_okd", NTs);
    }
    if (r->value) a.o_value = scratch_t<uint64_t>(c, "ms_oval", NTs);
    if ((r->tx_seg && !a.o_txseg) || (r->tx_pos && !a.o_txpos) ||
        (cols && (!a.o_id || !a.o_cause || !a.o_cis || !a.o_kind)) || (r->value && !a.o_value))
      return fail(c, "out of device memory (host-mode staging)");
  }

  // the two layouts on the device, each cached while it repeats
  const char *n_off = "mi_off", *n_toff = "mi_toff";
  bool miss;
  if (device_layout(c, st.colls, D, off, nullptr, &n_off, nullptr, &a.coll_off, &miss) ||
      device_layout(c, st.txs, D, toff, nullptr, &n_toff, nullptr, &a.tx_off, &miss))
    return -1;
  a.new_off = scratch_t<uint64_t>(c, "mi_noff", D + 2);
  if (!a.new_off) return fail(c, "out of device memory (map insert)");
  const uint32_t kl = MI_LDS_TX / gp;
  if (kmax > kl) {  // a tx too long for LDS plans in scratch
    a.gplan = scratch_t<uint32_t>(c, "mi_plan", (size_t)T * MI_PW);
    if (!a.gplan) return fail(c, "out of device memory (map insert plan)");
  }
  a.blocks = blocks;
  a.lb = lookback_words(c, st.lb, "mi_lb", 2 * blocks, 1, &a.epoch);
  if (!a.lb) return -1;
  {
    // per node its id in, its seg_perm word in and out, the columns in and out;
    // per key weave its four words in and out; per tx node its columns, its plan
    // and its two outputs; per collection its offsets, status and look-back words
    double per = 8 + 8;
    if (a.o_id) per += 36;
    if (a.o_value) per += 16;
    const double bytes = (double)N * per + (double)S * 56 + (double)T * (18 + 28 + 8 + (a.o_id ? 18 : 0)) +
                         (double)D * 44;
    Launch L(c, wave ? "map_insert" : "map_insert_wg", bytes);
    if (wave) hipLaunchKernelGGL(k_map_insert<64>, dim3(blocks), dim3(MI_NT), 0, c->stream, a);
    else hipLaunchKernelGGL(k_map_insert<256>, dim3(blocks), dim3(MI_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_map_insert")) return -1;
  // the call's one wait: the new offsets and n_segs
  std::vector<uint64_t> h(D + 2);
  HIPCHK(c, hipMemcpyAsync(h.data(), a.new_off, (D + 2) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t M = h[D], Sn = h[D + 1];
  if (M > N + T || Sn > S + T) return fail(c, "internal: new offsets past N + T");
  memcpy(r->new_offsets, h.data(), (D + 1) * 8);
  res.n_segs = Sn;
  if (!dev) {
    dres.n_segs = Sn;
    if (unstage_map_result(c, dres, M, D, res)) return -1;
    if (T && r->tx_seg) HIPCHK(c, hipMemcpy(r->tx_seg, a.o_txseg, T * 4, hipMemcpyDeviceToHost));
    if (T && r->tx_pos) HIPCHK(c, hipMemcpy(r->tx_pos, a.o_txpos, T * 4, hipMemcpyDeviceToHost));
    if (M && cols) {
      HIPCHK(c, hipMemcpy(r->id_key, a.o_id, M * 8, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(r->cause, a.o_cause, M * 8, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(r->cause_is_id, a.o_cis, M, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(r->kind, a.o_kind, M, hipMemcpyDeviceToHost));
    }
    if (M && r->value) HIPCHK(c, hipMemcpy(r->value, a.o_value, M * 8, hipMemcpyDeviceToHost));
  }
  return c->prof ? collect_prof(c) : 0;
}

}  // namespace
