// transact.hip -- cw_transact (include/causeweave_transact.h): transact- (base/
// core.cljc:100-252) over the token streams of a batch of bases: the tx-index, a
// collection per nested list or map, the list chains, the spliced strings.
// Included by causeweave.hip after renderbase.hip (in_doc_of, lookback.h).
//
// Nothing walks a stream: a stack would be as deep as the nesting.  The tokens
// take their depth from a scan and are sorted once, stably, by (base, depth,
// target of their part); that lays the direct children of every group side by
// side, each run ending in the group's CLOSE, and within a base the k-th CLOSE
// in sorted order closes the k-th opener in sorted order (the openers of depth
// L are as many as the CLOSEs of depth L + 1 and stand in the same order).
// Tiles are TX_TILE = 2,048 positions, eight a thread.
//
// k_tx_scan, token tiles: three scans by the look-back over the token kinds:
//   the depth (+1 after an opener, -1 before a CLOSE), the parts (PART, ROOT_*)
//   and the new collections (ROOT_*, OPEN_*); the parts compacted (part_tok).
// k_tx_level, token tiles: the token's base, its depth within the base, every
//   MALFORMED test, the new lists of a base counted, its last ROOT_*; the sort
//   key base | depth | target, the target being the part's document within the
//   base (a ROOT_*: past the base's documents, by its collection number), so
//   that several parts into one document stand together, in part order.
// (the library's stable key sort, radix_sort)
// k_tx_rank, sorted tiles: the openers and the CLOSEs numbered in sorted order
//   (two scans); the openers compacted (op), own[token] = an opener's number.
// k_tx_group, a thread a sorted position: the token's group r = the base's first
//   opener + the base's CLOSEs before the token; gr[token] = r, close_tok[r];
//   the group's kind gives the token's node count (cnt, token order) and what
//   the child adds to its group (es, sorted order: an OPEN_* stands for its ref).
// k_tx_count, token tiles: cnt scanned (64 bits, saturating): the tx-index.
// k_tx_bases, 256 bases a workgroup: base_status, the base's new collections and
//   nodes, their offsets by two scans, root_doc.
// k_tx_runs, sorted tiles: es of the bases that are not flagged scanned: W, the
//   VIRTUAL NODE number -- the nodes of a group, and of an existing document, are
//   consecutive in it.  A run's head gives w_start[r], its CLOSE w_close[r], the
//   first and last child of the parts into document d doc_w0[d] and doc_w1[d];
//   new_tok[c] = the token that opens new collection c.
// k_tx_docoff, a thread a document, existing and new: its nodes (a new list's
//   root added), node_offsets by a scan; the entries past the last collection
//   repeat the total.
// (the call's one wait: the three offset arrays and the totals; the capacities)
// k_tx_expand, tiles of virtual nodes: a node finds its child by a search in W
//   (so a STR of any length is spread), then its group, document, position, id,
//   cause (in a list group the id of virtual node v - 1, by a second search
//   when that is another child's) and the other columns.
// k_tx_news, a thread a new collection: new_is_map, new_open, a list's root node.
//
// Nothing is read or written outside the caller's arrays: a target is checked
// against the base's documents before doc_is_map is read, every group, opener
// and collection number against its array before it is used, and every node
// position against M and node_cap before it is written.

constexpr uint32_t TX_NT = 256, TX_IPT = 8;
constexpr uint32_t TX_TILE = TX_NT * TX_IPT;
constexpr uint32_t TX_NONE = 0xFFFFFFFFu;
constexpr uint32_t TX_CAP = 4096;  // tokens of a base that one workgroup sorts in LDS (10 bytes a token)
// the look-back word's count field holds 46 bits: 64-bit sums saturate below it
constexpr unsigned long long TX_CNT = (1ull << LB_EPOCH) - 1, TX_SAT = (1ull << 45) - 1;

struct TxArgs {
  uint32_t T, D, G, tiles;
  uint32_t K;        // the node_offsets entries made: D + min(new_cap, T) + 1
  uint32_t V, M;     // (after the wait) virtual nodes, nodes
  uint64_t node_cap;
  uint32_t site_shift;
  uint32_t tbits, lbits;  // the key: base << (lbits + tbits) | depth << tbits | target
  const uint32_t *tok_off, *bdoc_off;  // device [G + 1]
  const uint8_t *is_map, *kind, *cii, *vkind;
  const uint32_t *arg;
  const uint64_t *cause, *new_tx;
  // per token (+ 1: the total)
  uint32_t *lvl_p, *part_p, *new_p, *nl_p;  // the four scans of k_tx_scan
  uint32_t *part_tok;                // the parts, compacted
  uint64_t *key;                     // the sort's input
  uint32_t *gr, *own, *cnt;
  unsigned long long *cnt_p;         // [T + 1]
  // in sorted order
  const uint64_t *skey;
  const uint32_t *sval;
  uint32_t *o_rank, *c_rank;         // [T + 1]
  uint32_t *op, *close_tok, *w_start, *w_close;  // by group
  uint32_t *es, *W;                  // W: [T + 1]
  uint32_t *new_tok;                 // [T] by new collection
  // per existing document (0), per base
  uint32_t *doc_w0, *doc_w1;
  uint32_t *flag, *root_tok;  // (0)
  unsigned long long *bnew, *bnode;   // [G + 1]
  unsigned long long *noff;           // [K]
  unsigned long long *ctl;            // [0] virtual nodes, [1] the sum of every count
  unsigned long long *lb;
  uint32_t epoch;
  // outputs
  uint32_t *o_status, *o_root;
  uint64_t *o_id, *o_cause;
  uint8_t *o_cii, *o_kind, *o_run, *o_is_map;
  uint32_t *o_src, *o_sub, *o_ref, *o_open;
};

__device__ __forceinline__ bool tx_opener(uint32_t k) { return k == CW_TX_OPEN_LIST || k == CW_TX_OPEN_MAP || (k >= CW_TX_PART && k <= CW_TX_ROOT_MAP); }
__device__ __forceinline__ bool tx_part(uint32_t k) { return k >= CW_TX_PART && k <= CW_TX_ROOT_MAP; }
__device__ __forceinline__ bool tx_new(uint32_t k) { return k == CW_TX_OPEN_LIST || k == CW_TX_OPEN_MAP || k == CW_TX_ROOT_LIST || k == CW_TX_ROOT_MAP; }
__device__ __forceinline__ bool tx_new_list(uint32_t k) { return k == CW_TX_OPEN_LIST || k == CW_TX_ROOT_LIST; }

// Exclusive prefix of v over the workgroup's TX_NT threads; *total: the sum.
// tmp: TX_NT / 64 words of LDS.
template <typename T>
__device__ __forceinline__ T tx_scan(T v, T *tmp, T *total) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T x = v;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const T y = __shfl_up(x, s, 64);
    if (lane >= (uint32_t)s) x += y;
  }
  __syncthreads();
  if (lane == 63) tmp[w] = x;
  __syncthreads();
  T b = 0, tot = 0;
#pragma unroll
  for (uint32_t k = 0; k < TX_NT / 64; k++) {
    const T c = tmp[k];
    b += k < w ? c : (T)0;
    tot += c;
  }
  *total = tot;
  return b + x - v;
}

// lookback.h's protocol with the whole 46-bit count field: the sums saturate at
// TX_SAT (no legal call comes near: M < 2^32), so a word never overflows into
// the epoch.  One thread publishes, the first wave looks back.
__device__ __forceinline__ void tx_lb_publish(unsigned long long *lb, uint32_t i, uint32_t epoch,
                                              unsigned long long count) {
  const unsigned long long w =
      (i == 0 ? LB_INC : LB_AGG) | ((unsigned long long)epoch << LB_EPOCH) | (count < TX_SAT ? count : TX_SAT);
  __hip_atomic_store(lb + i, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned long long tx_lb_exclusive(unsigned long long *lb, uint32_t i, uint32_t epoch,
                                                              unsigned long long count) {
  if (i == 0) return 0;
  const unsigned long long ep = (unsigned long long)epoch << LB_EPOCH;
  const uint32_t lane = threadIdx.x;  // (the first wave: < 64)
  unsigned long long base = 0;
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
    unsigned long long x = lane <= first ? (v & TX_CNT) : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    base = base + x < TX_SAT ? base + x : TX_SAT;
    if (first < 64) break;
    q0 -= 64;
  }
  if (lane == 0) {
    const unsigned long long s = base + count < TX_SAT ? base + count : TX_SAT;
    __hip_atomic_store(lb + i, LB_INC | ep | s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return base;
}

// The base of a sorted position's key.
__device__ __forceinline__ uint32_t tx_key_base(const TxArgs &a, uint64_t key) {
  const uint32_t sh = a.lbits + a.tbits;  // (<= 63)
  const uint64_t g = key >> sh;
  return g < a.G ? (uint32_t)g : a.G - 1;
}

__global__ __launch_bounds__(TX_NT) void k_tx_scan(TxArgs a) {
  __shared__ uint32_t tmp[TX_NT / 64], s_base[4];
  const uint32_t tid = threadIdx.x, t = blockIdx.x, g0 = t * TX_TILE;  // (t < tiles: g0 < T)
  uint8_t kd[TX_IPT];
  uint32_t s_inc = 0, s_part = 0, s_new = 0, s_nl = 0;
#pragma unroll
  for (uint32_t k = 0; k < TX_IPT; k++) {
    const uint32_t i = g0 + tid * TX_IPT + k;
    kd[k] = i < a.T ? a.kind[i] : (uint8_t)0xFF;
    s_inc += tx_opener(kd[k]) ? 1u : kd[k] == CW_TX_CLOSE ? 0xFFFFFFFFu : 0u;  // (mod 2^32: a depth is a difference)
    s_part += tx_part(kd[k]) ? 1u : 0u;
    s_new += tx_new(kd[k]) ? 1u : 0u;
    s_nl += tx_new_list(kd[k]) ? 1u : 0u;
  }
  uint32_t t_inc, t_part, t_new, t_nl;
  uint32_t e_inc = tx_scan<uint32_t>(s_inc, tmp, &t_inc);
  uint32_t e_part = tx_scan<uint32_t>(s_part, tmp, &t_part);
  uint32_t e_new = tx_scan<uint32_t>(s_new, tmp, &t_new);
  uint32_t e_nl = tx_scan<uint32_t>(s_nl, tmp, &t_nl);
  if (tid < 64) {
    if (tid == 0) {
      lb_publish(a.lb, t, a.epoch, t_inc);
      lb_publish(a.lb + a.tiles, t, a.epoch, t_part);
      lb_publish(a.lb + 2 * (size_t)a.tiles, t, a.epoch, t_new);
      lb_publish(a.lb + 3 * (size_t)a.tiles, t, a.epoch, t_nl);
    }
    const uint32_t b0 = lb_exclusive(a.lb, t, a.epoch, t_inc);
    const uint32_t b1 = lb_exclusive(a.lb + a.tiles, t, a.epoch, t_part);
    const uint32_t b2 = lb_exclusive(a.lb + 2 * (size_t)a.tiles, t, a.epoch, t_new);
    const uint32_t b3 = lb_exclusive(a.lb + 3 * (size_t)a.tiles, t, a.epoch, t_nl);
    if (tid == 0) {
      s_base[0] = b0;
      s_base[1] = b1;
      s_base[2] = b2;
      s_base[3] = b3;
      if (t + 1 == a.tiles) {
        a.lvl_p[a.T] = b0 + t_inc;
        a.part_p[a.T] = b1 + t_part;
        a.new_p[a.T] = b2 + t_new;
        a.nl_p[a.T] = b3 + t_nl;
      }
    }
  }
  __syncthreads();
  e_inc += s_base[0];
  e_part += s_base[1];
  e_new += s_base[2];
  e_nl += s_base[3];
#pragma unroll
  for (uint32_t k = 0; k < TX_IPT; k++) {
    const uint32_t i = g0 + tid * TX_IPT + k;
    if (i >= a.T) break;
    a.lvl_p[i] = e_inc;
    a.part_p[i] = e_part;
    a.new_p[i] = e_new;
    a.nl_p[i] = e_nl;
    if (tx_part(kd[k]) && e_part < a.T) a.part_tok[e_part] = i;
    e_inc += tx_opener(kd[k]) ? 1u : kd[k] == CW_TX_CLOSE ? 0xFFFFFFFFu : 0u;
    e_part += tx_part(kd[k]) ? 1u : 0u;
    e_new += tx_new(kd[k]) ? 1u : 0u;
    e_nl += tx_new_list(kd[k]) ? 1u : 0u;
  }
}

__global__ __launch_bounds__(TX_NT) void k_tx_level(TxArgs a) {
  __shared__ uint32_t s_glo, s_ghi;
  const uint32_t tid = threadIdx.x, g0 = blockIdx.x * TX_TILE;  // (g0 < T)
  const uint32_t n = a.T - g0 < TX_TILE ? a.T - g0 : TX_TILE;
  if (tid == 0) s_glo = in_doc_of(a.tok_off, 0u, a.G - 1, g0);
  if (tid == 64) s_ghi = in_doc_of(a.tok_off, 0u, a.G - 1, g0 + n - 1);
  __syncthreads();
  const uint32_t glo = s_glo, ghi = s_ghi, h_end = a.tok_off[glo + 1];
  const uint64_t lmask = (1ull << a.lbits) - 1, tmask = (1ull << a.tbits) - 1;  // (lbits <= 32, tbits <= 33)
  for (uint32_t k = 0; k < TX_IPT; k++) {
    const uint32_t i = g0 + tid * TX_IPT + k;
    if (i >= a.T) break;
    const uint32_t g = i < h_end ? glo : in_doc_of(a.tok_off, glo + 1, ghi, i);
    const uint32_t t0 = a.tok_off[g], t1 = a.tok_off[g + 1], d0 = a.bdoc_off[g], d1 = a.bdoc_off[g + 1];
    const uint32_t kd = a.kind[i], ar = a.arg[i];
    const int32_t lv = (int32_t)(a.lvl_p[i] - a.lvl_p[t0]);
    bool bad = kd > CW_TX_ROOT_MAP;
    int32_t after = lv;
    if (kd == CW_TX_CLOSE) {
      bad |= lv <= 0;
      after = lv - 1;
    } else if (tx_part(kd)) {
      bad |= lv != 0;
      if (kd == CW_TX_PART) bad |= ar < d0 || ar >= d1;
      after = lv + 1;
    } else if (kd <= CW_TX_OPEN_MAP) {
      bad |= lv <= 0;
      if (kd >= CW_TX_OPEN_LIST) after = lv + 1;
    }
    if (i + 1 == t1) bad |= after != 0;
    if (bad) a.flag[g] = 1u;
    if (kd == CW_TX_ROOT_LIST || kd == CW_TX_ROOT_MAP) atomicMax(a.root_tok + g, i + 1);  // (no returned value)
    // the target of the token's part
    uint64_t tg = 0;
    const uint32_t pidx = a.part_p[i] + (tx_part(kd) ? 1u : 0u);
    if (pidx > a.part_p[t0] && pidx - 1 < a.T) {
      const uint32_t pt = a.part_tok[pidx - 1];
      if (pt < a.T) {
        const uint32_t pa = a.arg[pt];
        if (a.kind[pt] == CW_TX_PART) tg = pa >= d0 && pa < d1 ? pa - d0 : 0u;
        else tg = (uint64_t)(d1 - d0) + (a.new_p[pt] - a.new_p[t0]);
      }
    }
    if (tg > tmask) tg = tmask;
    uint64_t lk = lv < 0 ? 0ull : (uint64_t)lv;
    if (lk > lmask) lk = lmask;
    a.key[i] = ((uint64_t)g << (a.lbits + a.tbits)) | (lk << a.tbits) | tg;
  }
}

// The small route: a base of at most TX_CAP tokens a workgroup, its keys sorted
// in LDS (invert.hip's bitonic network over 16-bit indices; equal keys by token,
// so the order is the stable sort's) and written to the base's own range of the
// sorted arrays, which is where the key sort over all bases puts them.
__global__ __launch_bounds__(TX_NT) void k_tx_sort_wg(TxArgs a, uint64_t *ko, uint32_t *vo) {
  __shared__ uint64_t keys[TX_CAP];
  __shared__ uint16_t p[TX_CAP];
  const uint32_t g = blockIdx.x, tid = threadIdx.x;  // (g < G)
  const uint32_t t0 = a.tok_off[g], t1 = a.tok_off[g + 1];
  if (t1 <= t0 || t1 - t0 > TX_CAP || t1 > a.T) return;  // (the host takes this route only when every base fits)
  const uint32_t n = t1 - t0, m = iv_pow2(n);
  for (uint32_t i = tid; i < m; i += TX_NT) {
    if (i < n) keys[i] = a.key[t0 + i];
    p[i] = i < n ? (uint16_t)i : IV_PAD;
  }
  __syncthreads();
  iv_bitonic<TX_NT>(p, m, [&](uint32_t x, uint32_t y) { return keys[x] != keys[y] ? keys[x] < keys[y] : x < y; });
  for (uint32_t i = tid; i < n; i += TX_NT) {
    const uint32_t e = p[i];
    if (e >= n) continue;
    ko[t0 + i] = keys[e];
    vo[t0 + i] = t0 + e;
  }
}

__global__ __launch_bounds__(TX_NT) void k_tx_rank(TxArgs a) {
  __shared__ uint32_t tmp[TX_NT / 64], s_base[2];
  const uint32_t tid = threadIdx.x, t = blockIdx.x, g0 = t * TX_TILE;
  uint32_t tk[TX_IPT];
  uint8_t kd[TX_IPT];
  uint32_t s_o = 0, s_c = 0;
#pragma unroll
  for (uint32_t k = 0; k < TX_IPT; k++) {
    const uint32_t s = g0 + tid * TX_IPT + k;
    tk[k] = s < a.T ? a.sval[s] : TX_NONE;
    kd[k] = tk[k] < a.T ? a.kind[tk[k]] : (uint8_t)0xFF;
    s_o += tx_opener(kd[k]) ? 1u : 0u;
    s_c += kd[k] == CW_TX_CLOSE ? 1u : 0u;
  }
  uint32_t t_o, t_c;
  uint32_t e_o = tx_scan<uint32_t>(s_o, tmp, &t_o);
  uint32_t e_c = tx_scan<uint32_t>(s_c, tmp, &t_c);
  if (tid < 64) {
    if (tid == 0) {
      lb_publish(a.lb, t, a.epoch, t_o);
      lb_publish(a.lb + a.tiles, t, a.epoch, t_c);
    }
    const uint32_t b0 = lb_exclusive(a.lb, t, a.epoch, t_o);
    const uint32_t b1 = lb_exclusive(a.lb + a.tiles, t, a.epoch, t_c);
    if (tid == 0) {
      s_base[0] = b0;
      s_base[1] = b1;
      if (t + 1 == a.tiles) {
        a.o_rank[a.T] = b0 + t_o;
        a.c_rank[a.T] = b1 + t_c;
      }
    }
  }
  __syncthreads();
  e_o += s_base[0];
  e_c += s_base[1];
#pragma unroll
  for (uint32_t k = 0; k < TX_IPT; k++) {
    const uint32_t s = g0 + tid * TX_IPT + k;
    if (s >= a.T) break;
    a.o_rank[s] = e_o;
    a.c_rank[s] = e_c;
    if (tx_opener(kd[k]) && e_o < a.T) {  // (kd is an opener's: tk < T)
      a.op[e_o] = tk[k];
      a.own[tk[k]] = e_o;
    }
    e_o += tx_opener(kd[k]) ? 1u : 0u;
    e_c += kd[k] == CW_TX_CLOSE ? 1u : 0u;
  }
}

__global__ __launch_bounds__(256) void k_tx_group(TxArgs a) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s >= a.T) return;
  const uint32_t i = a.sval[s];
  if (i >= a.T) return;
  const uint64_t key = a.skey[s];
  const uint32_t g = tx_key_base(a, key), t0 = a.tok_off[g], t1 = a.tok_off[g + 1];
  const uint64_t lv = (key >> a.tbits) & ((1ull << a.lbits) - 1);
  const uint32_t kd = a.kind[i];
  uint32_t r = TX_NONE, cnt = 0, e = 0;
  if (lv > 0 && t0 <= s && s < t1) {
    r = a.o_rank[t0] + (a.c_rank[s] - a.c_rank[t0]);
    if (r >= a.o_rank[t1] || r >= a.T) r = TX_NONE;  // (a malformed base)
  }
  if (r != TX_NONE) {
    const uint32_t o = a.op[r], ok = o < a.T ? a.kind[o] : 0xFFu;
    bool gmap = ok == CW_TX_OPEN_MAP || ok == CW_TX_ROOT_MAP;
    if (ok == CW_TX_PART) {
      const uint32_t d = a.arg[o];
      gmap = d < a.D && a.is_map[d] != 0;
    }
    if (kd == CW_TX_CLOSE) {
      a.close_tok[r] = i;
      cnt = ok == CW_TX_OPEN_LIST || ok == CW_TX_OPEN_MAP ? 1u : 0u;
    } else if (kd == CW_TX_LEAF) {
      cnt = e = 1;
    } else if (kd == CW_TX_STR) {
      cnt = e = gmap ? 1u : a.arg[i];
    } else if (kd == CW_TX_OPEN_LIST || kd == CW_TX_OPEN_MAP) {
      e = 1;
    }
  }
  a.gr[i] = r;
  a.cnt[i] = cnt;
  a.es[s] = e;
}

__global__ __launch_bounds__(TX_NT) void k_tx_count(TxArgs a) {
  __shared__ unsigned long long tmp[TX_NT / 64], s_base;
  const uint32_t tid = threadIdx.x, t = blockIdx.x, g0 = t * TX_TILE;
  uint32_t v[TX_IPT];
  unsigned long long sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < TX_IPT; k++) {
    const uint32_t i = g0 + tid * TX_IPT + k;
    v[k] = i < a.T ? a.cnt[i] : 0u;
    sum += v[k];
  }
  unsigned long long tot;
  unsigned long long ex = tx_scan<unsigned long long>(sum, tmp, &tot);
  if (tid < 64) {
    if (tid == 0) tx_lb_publish(a.lb, t, a.epoch, tot);
    const unsigned long long b = tx_lb_exclusive(a.lb, t, a.epoch, tot);
    if (tid == 0) {
      s_base = b;
      if (t + 1 == a.tiles) {
        const unsigned long long all = b + tot < TX_SAT ? b + tot : TX_SAT;
        a.cnt_p[a.T] = all;
        a.ctl[1] = all;
      }
    }
  }
  __syncthreads();
  ex += s_base;
#pragma unroll
  for (uint32_t k = 0; k < TX_IPT; k++) {
    const uint32_t i = g0 + tid * TX_IPT + k;
    if (i >= a.T) break;
    a.cnt_p[i] = ex;
    ex += v[k];
  }
}

__global__ __launch_bounds__(TX_NT) void k_tx_bases(TxArgs a) {
  __shared__ unsigned long long tmp[TX_NT / 64], s_base[2];
  const uint32_t tid = threadIdx.x, g = blockIdx.x * TX_NT + tid;
  unsigned long long nnew = 0, nodes = 0;
  uint32_t st = 0, t0 = 0;
  if (g < a.G) {
    t0 = a.tok_off[g];
    const uint32_t t1 = a.tok_off[g + 1];
    const unsigned long long tot = a.cnt_p[t1] - a.cnt_p[t0];
    if (a.flag[g]) st = (uint32_t)CW_STATUS_TX_MALFORMED;
    else if (tot > (1ull << a.site_shift)) st = (uint32_t)CW_STATUS_KEY_RANGE;
    if (!st) {
      nnew = a.new_p[t1] - a.new_p[t0];
      nodes = tot + (a.nl_p[t1] - a.nl_p[t0]);
    }
    a.o_status[g] = st;
  }
  unsigned long long t_new, t_nodes;
  const unsigned long long e_new = tx_scan<unsigned long long>(nnew, tmp, &t_new);
  const unsigned long long e_nodes = tx_scan<unsigned long long>(nodes, tmp, &t_nodes);
  if (tid < 64) {
    if (tid == 0) {
      tx_lb_publish(a.lb, blockIdx.x, a.epoch, t_new);
      tx_lb_publish(a.lb + gridDim.x, blockIdx.x, a.epoch, t_nodes);
    }
    const unsigned long long b0 = tx_lb_exclusive(a.lb, blockIdx.x, a.epoch, t_new);
    const unsigned long long b1 = tx_lb_exclusive(a.lb + gridDim.x, blockIdx.x, a.epoch, t_nodes);
    if (tid == 0) {
      s_base[0] = b0;
      s_base[1] = b1;
    }
  }
  __syncthreads();
  if (g >= a.G) return;
  const unsigned long long bn = s_base[0] + e_new;
  a.bnew[g] = bn;
  a.bnode[g] = s_base[1] + e_nodes;
  if (g == a.G - 1) {
    a.bnew[a.G] = bn + nnew;
    a.bnode[a.G] = s_base[1] + e_nodes + nodes;
  }
  uint32_t root = TX_NONE;
  const uint32_t rt = a.root_tok[g];
  if (!st && rt && rt <= a.T) root = (uint32_t)(a.D + bn + (a.new_p[rt - 1] - a.new_p[t0]));
  a.o_root[g] = root;
}

__global__ __launch_bounds__(TX_NT) void k_tx_runs(TxArgs a) {
  __shared__ unsigned long long tmp[TX_NT / 64], s_base;
  const uint32_t tid = threadIdx.x, t = blockIdx.x, g0 = t * TX_TILE;
  uint32_t v[TX_IPT], gb[TX_IPT];
  unsigned long long sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < TX_IPT; k++) {
    const uint32_t s = g0 + tid * TX_IPT + k;
    v[k] = 0;
    gb[k] = TX_NONE;
    if (s < a.T) {
      const uint32_t g = tx_key_base(a, a.skey[s]);
      if (!a.o_status[g]) {
        gb[k] = g;
        v[k] = a.es[s];
      }
    }
    sum += v[k];
  }
  unsigned long long tot;
  unsigned long long ex = tx_scan<unsigned long long>(sum, tmp, &tot);
  if (tid < 64) {
    if (tid == 0) tx_lb_publish(a.lb, t, a.epoch, tot);
    const unsigned long long b = tx_lb_exclusive(a.lb, t, a.epoch, tot);
    if (tid == 0) {
      s_base = b;
      if (t + 1 == a.tiles) {
        const unsigned long long all = b + tot < TX_SAT ? b + tot : TX_SAT;
        a.W[a.T] = (uint32_t)all;
        a.ctl[0] = all;
      }
    }
  }
  __syncthreads();
  ex += s_base;
  for (uint32_t k = 0; k < TX_IPT; k++) {
    const uint32_t s = g0 + tid * TX_IPT + k;
    if (s >= a.T) break;
    const uint32_t w = (uint32_t)ex;  // (exact whenever the call goes on: the total is checked against 2^32)
    a.W[s] = w;
    ex += v[k];
    const uint32_t g = gb[k];
    if (g == TX_NONE) continue;  // a flagged base
    const uint32_t i = a.sval[s];
    if (i >= a.T) continue;
    const uint32_t t0 = a.tok_off[g], t1 = a.tok_off[g + 1], kd = a.kind[i];
    if (tx_new(kd)) {
      const unsigned long long c = a.bnew[g] + (a.new_p[i] - a.new_p[t0]);
      if (c < a.T) a.new_tok[c] = i;
    }
    const uint32_t r = a.gr[i];
    if (r >= a.T) continue;
    const uint64_t key = a.skey[s];
    const bool first = s == t0 || s == 0 || a.skey[s - 1] != key;
    bool head = first;
    if (!head) {
      const uint32_t pi = a.sval[s - 1];
      head = pi < a.T && a.kind[pi] == CW_TX_CLOSE;
    }
    if (head) a.w_start[r] = w;
    if (kd == CW_TX_CLOSE) a.w_close[r] = w;
    const uint32_t o = a.op[r];
    if (o < a.T && a.kind[o] == CW_TX_PART) {
      const uint32_t d = a.arg[o];
      if (d < a.D) {
        if (first) a.doc_w0[d] = w;
        if (s + 1 == t1 || s + 1 >= a.T || a.skey[s + 1] != key) a.doc_w1[d] = w + v[k];
      }
    }
  }
}

__global__ __launch_bounds__(TX_NT) void k_tx_docoff(TxArgs a) {
  __shared__ unsigned long long tmp[TX_NT / 64], s_base;
  const uint32_t tid = threadIdx.x, k = blockIdx.x * TX_NT + tid;
  const unsigned long long C = a.bnew[a.G];
  unsigned long long n = 0;
  if (k < a.D) {
    n = a.doc_w1[k] - a.doc_w0[k];
  } else if (k < a.K - 1 && (unsigned long long)(k - a.D) < C) {  // (K - 1 = D + min(new_cap, T))
    const uint32_t i = a.new_tok[k - a.D];
    if (i < a.T) {
      const uint32_t r = a.own[i];
      if (r < a.T) n = (unsigned long long)(a.w_close[r] - a.w_start[r]) + (tx_new_list(a.kind[i]) ? 1u : 0u);
    }
  }
  unsigned long long tot;
  const unsigned long long ex = tx_scan<unsigned long long>(n, tmp, &tot);
  if (tid < 64) {
    if (tid == 0) tx_lb_publish(a.lb, blockIdx.x, a.epoch, tot);
    const unsigned long long b = tx_lb_exclusive(a.lb, blockIdx.x, a.epoch, tot);
    if (tid == 0) s_base = b;
  }
  __syncthreads();
  if (k < a.K) a.noff[k] = s_base + ex;
}

// The tx-index of the last node that the child at sorted position s makes.
__device__ __forceinline__ unsigned long long tx_last(const TxArgs &a, uint32_t s, uint32_t t0) {
  const uint32_t i = a.sval[s];
  if (i >= a.T) return 0;
  const uint32_t kd = a.kind[i];
  if (kd == CW_TX_OPEN_LIST || kd == CW_TX_OPEN_MAP) {  // its ref, made by its CLOSE
    const uint32_t r = a.own[i], m = r < a.T ? a.close_tok[r] : i;
    return a.cnt_p[m < a.T ? m : i] - a.cnt_p[t0];
  }
  return a.cnt_p[i] - a.cnt_p[t0] + (a.W[s + 1] - a.W[s]) - 1;
}

__global__ __launch_bounds__(TX_NT) void k_tx_expand(TxArgs a) {
  __shared__ uint32_t s_lo, s_hi;
  const uint32_t tid = threadIdx.x, g0 = blockIdx.x * TX_TILE;  // (g0 < V)
  const uint32_t n = a.V - g0 < TX_TILE ? a.V - g0 : TX_TILE;
  if (tid == 0) s_lo = in_doc_of(a.W, 0u, a.T - 1, g0);
  if (tid == 64) s_hi = in_doc_of(a.W, 0u, a.T - 1, g0 + n - 1);
  __syncthreads();
  const uint32_t slo = s_lo, shi = s_hi;
  for (uint32_t k = 0; k < TX_IPT; k++) {
    const uint32_t x = k * TX_NT + tid, v = g0 + x;
    if (x >= n) break;
    const uint32_t s = in_doc_of(a.W, slo, shi, v);  // the child that makes virtual node v
    const uint32_t i = a.sval[s];
    if (i >= a.T) continue;
    const uint32_t j = v - a.W[s], g = tx_key_base(a, a.skey[s]), t0 = a.tok_off[g];
    const uint32_t kd = a.kind[i], r = a.gr[i];
    if (r >= a.T) continue;
    const uint32_t o = a.op[r];
    if (o >= a.T) continue;
    const uint32_t ok = a.kind[o], q = v - a.w_start[r];
    // the group's document, the node's place in it
    unsigned long long pos;
    bool gmap;
    if (ok == CW_TX_PART) {
      const uint32_t d = a.arg[o];
      if (d >= a.D) continue;
      gmap = a.is_map[d] != 0;
      pos = a.noff[d] + (v - a.doc_w0[d]);
    } else {
      const unsigned long long c = a.bnew[g] + (a.new_p[o] - a.new_p[t0]);
      if (a.D + c + 1 >= a.K) continue;
      gmap = ok == CW_TX_OPEN_MAP || ok == CW_TX_ROOT_MAP;
      pos = a.noff[a.D + c] + (gmap ? 0u : 1u) + q;
    }
    // the token that makes it, its tx-index
    uint32_t mk = i, ref = TX_NONE;
    unsigned long long txi;
    if (kd == CW_TX_OPEN_LIST || kd == CW_TX_OPEN_MAP) {
      const uint32_t ro = a.own[i];
      mk = ro < a.T ? a.close_tok[ro] : i;
      if (mk >= a.T) mk = i;
      txi = a.cnt_p[mk] - a.cnt_p[t0];
      ref = (uint32_t)(a.D + a.bnew[g] + (a.new_p[i] - a.new_p[t0]));
    } else {
      txi = a.cnt_p[i] - a.cnt_p[t0] + j;
    }
    const uint64_t tx0 = a.new_tx[g], id = tx0 + txi;
    uint64_t ca;
    uint8_t ci = 1;
    if (gmap) {
      ca = a.cause[i];
      ci = a.cii[i];
    } else if (q == 0) {
      ca = ok == CW_TX_OPEN_LIST ? 0ull : a.cause[o];
    } else if (j > 0) {
      ca = id - 1;
    } else {  // the last node of the child before it
      const uint32_t s2 = in_doc_of(a.W, v - 1 >= g0 ? slo : 0u, s, v - 1);
      ca = tx0 + tx_last(a, s2, t0);
    }
    if (pos >= a.M || pos >= a.node_cap) continue;
    a.o_id[pos] = id;
    a.o_cause[pos] = ca;
    a.o_cii[pos] = ci;
    a.o_kind[pos] = kd == CW_TX_LEAF && a.vkind ? a.vkind[i] : (uint8_t)CW_KIND_NORMAL;
    a.o_src[pos] = mk;
    a.o_sub[pos] = kd == CW_TX_STR ? j : 0u;
    a.o_ref[pos] = ref;
    a.o_run[pos] = q == 0 ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_tx_news(TxArgs a, uint32_t C) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C || a.D + c + 1 >= a.K) return;
  const uint32_t i = a.new_tok[c];
  if (i >= a.T) return;
  const uint32_t kd = a.kind[i];
  a.o_is_map[c] = tx_new_list(kd) ? 0 : 1;
  a.o_open[c] = i;
  if (!tx_new_list(kd)) return;
  const unsigned long long pos = a.noff[a.D + c];
  if (pos >= a.M || pos >= a.node_cap) return;
  a.o_id[pos] = 0;  // new-causal-list's root node
  a.o_cause[pos] = CW_NIL;
  a.o_cii[pos] = 1;
  a.o_kind[pos] = (uint8_t)CW_KIND_ROOT;
  a.o_src[pos] = i;
  a.o_sub[pos] = 0;
  a.o_ref[pos] = TX_NONE;
  a.o_run[pos] = 0;
}

namespace {

// base_doc_offsets or tok_offsets: they start at 0 and do not decrease; *most: the largest step.
int tx_check_offsets(cw_ctx *c, const char *what, const uint64_t *off, uint64_t G, uint64_t *most) {
  if (off[0] != 0) return fail(c, "%s[0] must be 0", what);
  uint64_t mx = 0;
  for (uint64_t g = 0; g < G; g++) {
    if (off[g + 1] < off[g]) return fail(c, "%s not monotone", what);
    mx = std::max(mx, off[g + 1] - off[g]);
  }
  *most = mx;
  return 0;
}

int transact_impl(cw_ctx *c, const cw_transact_batch *b, cw_transact_result *r, int memspace) {
  if (!b || !r) return fail(c, "null batch/result");
  if (memspace != CW_MEM_HOST && memspace != CW_MEM_DEVICE) return fail(c, "bad memspace");
  const bool dev = memspace == CW_MEM_DEVICE;
  const uint64_t D = b->n_docs, G = b->n_bases;
  if (!b->base_doc_offsets || !b->tok_offsets || !r->base_new_offsets || !r->base_node_offsets || !r->node_offsets)
    return fail(c, "base_doc_offsets, tok_offsets, base_new_offsets, base_node_offsets and node_offsets are "
                   "required (host memory)");
  if (b->site_bits < 1 || b->site_bits > 10) return fail(c, "site_bits %u outside 1..10", b->site_bits);
  if (b->site_shift > 63 || b->ts_shift > 63) return fail(c, "bad key layout");
  if (b->reserved) return fail(c, "reserved must be 0");
  if (G >= 0xFFFFFFFFull) return fail(c, "batch too large: %llu bases (limit 2^32-1)", (unsigned long long)G);
  uint64_t most_docs, most_toks;
  if (tx_check_offsets(c, "base_doc_offsets", b->base_doc_offsets, G, &most_docs) ||
      tx_check_offsets(c, "tok_offsets", b->tok_offsets, G, &most_toks))
    return -1;
  if (b->base_doc_offsets[G] != D)
    return fail(c, "base_doc_offsets[n_bases] = %llu, n_docs = %llu", (unsigned long long)b->base_doc_offsets[G],
                (unsigned long long)D);
  const uint64_t T = b->tok_offsets[G];
  if (T >= 0xFFFFFFFFull || D + T >= 0xFFFFFFFFull)
    return fail(c, "batch too large: %llu tokens, %llu documents (limit 2^32-1 together)", (unsigned long long)T,
                (unsigned long long)D);
  if (D && !b->doc_is_map) return fail(c, "null doc_is_map");
  if (T && (!b->tok_kind || !b->tok_arg || !b->tok_cause || !b->tok_cause_is_id)) return fail(c, "null token columns");
  if (G && (!b->new_tx || !r->root_doc || !r->base_status)) return fail(c, "null new_tx, root_doc or base_status");
  const int given = (r->node_id != nullptr) + (r->node_cause != nullptr) + (r->node_cause_is_id != nullptr) +
                    (r->node_kind != nullptr) + (r->node_src != nullptr) + (r->node_sub != nullptr) +
                    (r->node_ref != nullptr) + (r->node_run != nullptr) + (r->new_is_map != nullptr) +
                    (r->new_open != nullptr);
  if (given != 0 && given != 10) return fail(c, "the node_* and new_* arrays go together");
  const bool full = given == 10;
  const uint32_t gbits = ceil_log2(std::max<uint64_t>(G, 1)), lbits = ceil_log2(most_toks + 1);
  const uint32_t tbits = std::max(1u, ceil_log2(most_docs + most_toks + 1));
  if (gbits + lbits + tbits > 63)
    return fail(c, "batch too large for the sort key: %u + %u + %u bits (limit 63)", gbits, lbits, tbits);
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t capC = std::min<uint64_t>(r->new_cap, T), K = D + capC + 1;
  if (T == 0 || G == 0) {  // no tokens: nothing is made
    for (uint64_t g = 0; g <= G; g++) r->base_new_offsets[g] = r->base_node_offsets[g] = 0;
    for (uint64_t k = 0; k < K; k++) r->node_offsets[k] = 0;
    if (!dev) {
      if (G) memset(r->base_status, 0, G * 4);
      if (G) memset(r->root_doc, 0xFF, G * 4);
      return 0;
    }
    if (G) HIPCHK(c, hipMemsetAsync(r->base_status, 0, G * 4, c->stream));
    if (G) HIPCHK(c, hipMemsetAsync(r->root_doc, 0xFF, G * 4, c->stream));
    if (!c->async) HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  }
  auto &st = c->transact;
  const uint32_t tiles = (uint32_t)((T + TX_TILE - 1) / TX_TILE), fblocks = (uint32_t)((T + 255) / 256);
  const uint32_t gblocks = (uint32_t)((G + TX_NT - 1) / TX_NT), kblocks = (uint32_t)((K + TX_NT - 1) / TX_NT);
  if (!grid_ok(fblocks, 256) || !grid_ok(gblocks, TX_NT) || !grid_ok(kblocks, TX_NT))
    return fail(c, "batch too large for one dispatch");

  TxArgs a{};
  a.T = (uint32_t)T;
  a.D = (uint32_t)D;
  a.G = (uint32_t)G;
  a.tiles = tiles;
  a.K = (uint32_t)K;
  a.node_cap = r->node_cap;
  a.site_shift = b->site_shift;
  a.tbits = tbits;
  a.lbits = lbits;
  a.is_map = b->doc_is_map;
  a.kind = b->tok_kind;
  a.arg = b->tok_arg;
  a.cause = b->tok_cause;
  a.cii = b->tok_cause_is_id;
  a.vkind = b->tok_vkind;
  a.new_tx = b->new_tx;
  if (!dev) {  // uploads
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (upload(c, "tx_ismap", b->doc_is_map, (size_t)D, &a.is_map) || upload(c, "tx_kind", b->tok_kind, (size_t)T, &a.kind) ||
        upload(c, "tx_arg", b->tok_arg, (size_t)T * 4, &a.arg) || upload(c, "tx_cause", b->tok_cause, (size_t)T * 8, &a.cause) ||
        upload(c, "tx_cii", b->tok_cause_is_id, (size_t)T, &a.cii) || upload(c, "tx_newtx", b->new_tx, (size_t)G * 8, &a.new_tx))
      return -1;
    if (a.vkind && upload(c, "tx_vkind", b->tok_vkind, (size_t)T, &a.vkind)) return -1;
  }
  // the two layouts on the device, each cached while it repeats
  const char *n_toff = "tx_toff", *n_doff = "tx_doff";
  bool miss;
  if (device_layout(c, st.toks, G, b->tok_offsets, nullptr, &n_toff, nullptr, &a.tok_off, &miss) ||
      device_layout(c, st.docs, G, b->base_doc_offsets, nullptr, &n_doff, nullptr, &a.bdoc_off, &miss))
    return -1;
  // the route: every base within transact_cap -> a workgroup a base sorts its keys in LDS;
  // one base above it -> the stable key sort over all bases at once (its tables: one array of T keys)
  const bool small = most_toks <= std::min(c->transact_cap, TX_CAP) && grid_ok(G, TX_NT);
  const uint64_t soff[2] = {0, T};
  if (!small && ensure_tables(c, 1, soff)) return -1;

  uint32_t *tz = scratch_t<uint32_t>(c, "tx_tok", 14 * (T + 1));      // fourteen columns of T + 1 words
  uint32_t *dz = scratch_t<uint32_t>(c, "tx_doc", 2 * D);              // doc_w0, doc_w1 (zero)
  uint32_t *gz = scratch_t<uint32_t>(c, "tx_base", 4 * G);             // flag, root_tok (zero), status, root_doc
  a.key = scratch_t<uint64_t>(c, "tx_key", T);
  uint64_t *kA = scratch_t<uint64_t>(c, "tx_kA", T), *kB = scratch_t<uint64_t>(c, "tx_kB", T);
  uint32_t *vA = scratch_t<uint32_t>(c, "tx_vA", T), *vB = scratch_t<uint32_t>(c, "tx_vB", T);
  a.cnt_p = scratch_t<unsigned long long>(c, "tx_cntp", T + 1);
  a.bnew = scratch_t<unsigned long long>(c, "tx_bnew", 2 * (G + 1));
  a.noff = scratch_t<unsigned long long>(c, "tx_noff", K);
  a.ctl = scratch_t<unsigned long long>(c, "tx_ctl", 4);
  if (!tz || !dz || !gz || !a.key || !kA || !kB || !vA || !vB || !a.cnt_p || !a.bnew || !a.noff || !a.ctl)
    return fail(c, "out of device memory (transact)");
  {
    uint32_t **cols[14] = {&a.lvl_p, &a.part_p, &a.new_p, &a.part_tok, &a.gr, &a.own, &a.cnt, &a.o_rank,
                           &a.c_rank, &a.op, &a.close_tok, &a.w_start, &a.w_close, &a.nl_p};
    for (int k = 0; k < 14; k++) *cols[k] = tz + (size_t)k * (T + 1);
  }
  a.es = scratch_t<uint32_t>(c, "tx_es", T);
  a.W = scratch_t<uint32_t>(c, "tx_W", T + 1);
  a.new_tok = scratch_t<uint32_t>(c, "tx_newtok", T);
  if (!a.es || !a.W || !a.new_tok) return fail(c, "out of device memory (transact)");
  a.doc_w0 = dz;
  a.doc_w1 = dz + D;
  a.flag = gz;
  a.root_tok = gz + G;
  a.o_status = gz + 2 * G;
  a.o_root = gz + 3 * G;
  a.bnode = a.bnew + (G + 1);
  if (D) HIPCHK(c, hipMemsetAsync(dz, 0, 2 * D * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(gz, 0, 2 * G * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(a.ctl, 0, 32, c->stream));
  // (a flagged base leaves holes in these; they are read only through checked indices)
  HIPCHK(c, hipMemsetAsync(a.gr, 0xFF, (T + 1) * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(a.own, 0xFF, (T + 1) * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(a.close_tok, 0xFF, (T + 1) * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(a.new_tok, 0xFF, T * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(a.w_start, 0, 2 * (T + 1) * 4, c->stream));  // w_start, w_close

  a.lb = lookback_words(c, st.lb_scan, "tx_lb_scan", 4 * tiles, 1, &a.epoch);
  if (!a.lb) return -1;
  {
    // per token its kind in, three prefixes out; per part its token
    Launch L(c, "k_tx_scan", (double)T * 13 + (double)tiles * 72);
    hipLaunchKernelGGL(k_tx_scan, dim3(tiles), dim3(TX_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_tx_scan")) return -1;
  {
    // per token its kind, argument and three prefixes in, its part's token and prefix, the key out
    Launch L(c, "k_tx_level", (double)T * 41);
    hipLaunchKernelGGL(k_tx_level, dim3(tiles), dim3(TX_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_tx_level")) return -1;
  uint64_t *ko = nullptr;
  uint32_t *vo = nullptr;
  if (small) {
    {
      // per token its key in, key and token out
      Launch L(c, "k_tx_sort_wg", (double)T * 20 + (double)G * 8);
      hipLaunchKernelGGL(k_tx_sort_wg, dim3((uint32_t)G), dim3(TX_NT), 0, c->stream, a, kA, vA);
    }
    if (check_launch(c, "k_tx_sort_wg")) return -1;
    ko = kA;
    vo = vA;
  } else if (radix_sort<uint64_t>(c, "tx_sort", a.key, nullptr, kA, vA, kB, vB, gbits + lbits + tbits, 0, (uint32_t)T,
                                  &ko, &vo)) {
    return -1;
  }
  a.skey = ko;
  a.sval = vo;
  a.lb = lookback_words(c, st.lb_rank, "tx_lb_rank", 2 * tiles, 1, &a.epoch);
  if (!a.lb) return -1;
  {
    // per sorted position its token and kind in, two ranks out; per opener two words
    Launch L(c, "k_tx_rank", (double)T * 17 + (double)tiles * 48);
    hipLaunchKernelGGL(k_tx_rank, dim3(tiles), dim3(TX_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_tx_rank")) return -1;
  {
    // per sorted position its key, token, kind and ranks in, its opener's kind and target; group, count and share out
    Launch L(c, "k_tx_group", (double)T * 46);
    hipLaunchKernelGGL(k_tx_group, dim3(fblocks), dim3(256), 0, c->stream, a);
  }
  if (check_launch(c, "k_tx_group")) return -1;
  a.lb = lookback_words(c, st.lb_count, "tx_lb_count", tiles, 1, &a.epoch);
  if (!a.lb) return -1;
  {
    Launch L(c, "k_tx_count", (double)T * 12 + (double)tiles * 24);
    hipLaunchKernelGGL(k_tx_count, dim3(tiles), dim3(TX_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_tx_count")) return -1;
  a.lb = lookback_words(c, st.lb_bases, "tx_lb_bases", 2 * gblocks, 1, &a.epoch);
  if (!a.lb) return -1;
  {
    Launch L(c, "k_tx_bases", (double)G * 76);
    hipLaunchKernelGGL(k_tx_bases, dim3(gblocks), dim3(TX_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_tx_bases")) return -1;
  a.lb = lookback_words(c, st.lb_runs, "tx_lb_runs", tiles, 1, &a.epoch);
  if (!a.lb) return -1;
  {
    // per sorted position its key, share, token, kind, group and neighbours in, W out; per group and document its marks
    Launch L(c, "k_tx_runs", (double)T * 56 + (double)tiles * 24);
    hipLaunchKernelGGL(k_tx_runs, dim3(tiles), dim3(TX_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_tx_runs")) return -1;
  a.lb = lookback_words(c, st.lb_docs, "tx_lb_docs", kblocks, 1, &a.epoch);
  if (!a.lb) return -1;
  {
    Launch L(c, "k_tx_docoff", (double)K * 28);
    hipLaunchKernelGGL(k_tx_docoff, dim3(kblocks), dim3(TX_NT), 0, c->stream, a);
  }
  if (check_launch(c, "k_tx_docoff")) return -1;

  // the call's one wait: the three offset arrays, with the totals
  // (through a pinned buffer the context keeps: the copies are asynchronous and the caller's arrays stay untouched until the checks)
  const size_t pin_need = (2 * (G + 1) + K) * 8;
  if (st.pin_bytes < pin_need) {
    if (st.pin) (void)hipHostFree(st.pin);
    st.pin = nullptr;
    st.pin_bytes = 0;
    HIPCHK(c, hipHostMalloc(&st.pin, pin_need + pin_need / 8, hipHostMallocDefault));
    st.pin_bytes = pin_need + pin_need / 8;
  }
  const uint64_t *h_b = static_cast<const uint64_t *>(st.pin), *h_n = h_b + 2 * (G + 1);
  HIPCHK(c, hipMemcpyAsync(st.pin, a.bnew, 2 * (G + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(static_cast<uint64_t *>(st.pin) + 2 * (G + 1), a.noff, K * 8, hipMemcpyDeviceToHost, c->stream));
  const uint32_t *ctl32 = read_small(c, a.ctl, 16);
  if (!ctl32) return -1;
  uint64_t ctl[2];
  memcpy(ctl, ctl32, 16);
  const uint64_t C = h_b[G], M = h_b[2 * G + 1], V = ctl[0];
  if (ctl[1] >= TX_SAT || V >= 0xFFFFFFFFull || M >= 0xFFFFFFFFull)
    return fail(c, "batch too large: the transactions make 2^32-1 nodes or more");
  if (full && (C > r->new_cap || M > r->node_cap))
    return fail(c, "capacities too small: %llu new collections (new_cap %llu), %llu nodes (node_cap %llu)",
                (unsigned long long)C, (unsigned long long)r->new_cap, (unsigned long long)M,
                (unsigned long long)r->node_cap);
  if (full && h_n[D + C] != M) return fail(c, "internal: node offsets end at %llu, %llu nodes", (unsigned long long)h_n[D + C], (unsigned long long)M);
  memcpy(r->base_new_offsets, h_b, (G + 1) * 8);
  memcpy(r->base_node_offsets, h_b + G + 1, (G + 1) * 8);
  memcpy(r->node_offsets, h_n, K * 8);
  a.V = (uint32_t)V;
  a.M = (uint32_t)M;
  a.o_id = r->node_id;
  a.o_cause = r->node_cause;
  a.o_cii = r->node_cause_is_id;
  a.o_kind = r->node_kind;
  a.o_src = r->node_src;
  a.o_sub = r->node_sub;
  a.o_ref = r->node_ref;
  a.o_run = r->node_run;
  a.o_is_map = r->new_is_map;
  a.o_open = r->new_open;
  if (full && !dev) {  // the outputs staged
    a.o_id = scratch_t<uint64_t>(c, "tx_oid", M);
    a.o_cause = scratch_t<uint64_t>(c, "tx_oca", M);
    a.o_cii = scratch_t<uint8_t>(c, "tx_oci", M);
    a.o_kind = scratch_t<uint8_t>(c, "tx_okd", M);
    a.o_src = scratch_t<uint32_t>(c, "tx_osrc", M);
    a.o_sub = scratch_t<uint32_t>(c, "tx_osub", M);
    a.o_ref = scratch_t<uint32_t>(c, "tx_oref", M);
    a.o_run = scratch_t<uint8_t>(c, "tx_orun", M);
    a.o_is_map = scratch_t<uint8_t>(c, "tx_oim", C);
    a.o_open = scratch_t<uint32_t>(c, "tx_oop", C);
    if (!a.o_id || !a.o_cause || !a.o_cii || !a.o_kind || !a.o_src || !a.o_sub || !a.o_ref || !a.o_run ||
        !a.o_is_map || !a.o_open)
      return fail(c, "out of device memory (host-mode staging)");
  }
  if (full && V) {
    const uint32_t vtiles = (uint32_t)((V + TX_TILE - 1) / TX_TILE);
    {
      // per node two searches in W, its child's and group's words in, 31 bytes out
      Launch L(c, "k_tx_expand", (double)V * (31 + 40));
      hipLaunchKernelGGL(k_tx_expand, dim3(vtiles), dim3(TX_NT), 0, c->stream, a);
    }
    if (check_launch(c, "k_tx_expand")) return -1;
  }
  if (full && C) {
    {
      Launch L(c, "k_tx_news", (double)C * 48);
      hipLaunchKernelGGL(k_tx_news, dim3((uint32_t)((C + 255) / 256)), dim3(256), 0, c->stream, a, (uint32_t)C);
    }
    if (check_launch(c, "k_tx_news")) return -1;
  }
  if (dev) {
    HIPCHK(c, hipMemcpyAsync(r->base_status, a.o_status, G * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(r->root_doc, a.o_root, G * 4, hipMemcpyDeviceToDevice, c->stream));
    if (!c->async) HIPCHK(c, hipStreamSynchronize(c->stream));
    return c->prof ? collect_prof(c) : 0;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (full && M) {
    HIPCHK(c, hipMemcpy(r->node_id, a.o_id, M * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(r->node_cause, a.o_cause, M * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(r->node_cause_is_id, a.o_cii, M, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(r->node_kind, a.o_kind, M, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(r->node_src, a.o_src, M * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(r->node_sub, a.o_sub, M * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(r->node_ref, a.o_ref, M * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(r->node_run, a.o_run, M, hipMemcpyDeviceToHost));
  }
  if (full && C) {
    HIPCHK(c, hipMemcpy(r->new_is_map, a.o_is_map, C, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(r->new_open, a.o_open, C * 4, hipMemcpyDeviceToHost));
  }
  HIPCHK(c, hipMemcpy(r->base_status, a.o_status, G * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(r->root_doc, a.o_root, G * 4, hipMemcpyDeviceToHost));
  return c->prof ? collect_prof(c) : 0;
}

}  // namespace
