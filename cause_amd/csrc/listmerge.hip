// listmerge.hip -- the union stage of cw_merge_lists (s/merge-trees,
// shared.cljc:300-314; a bulk s/insert, :151-184; CausalList's causal-merge).
// Included by causeweave.hip after mapmerge.hip: it uses the front end's rank
// directory (fr_rank), the general route's kernels (k_merge_concat,
// k_merge_dedup) and mapmerge.hip's union scaffold (union_sort_dedup,
// fused_union_tail).
//
// Per document the two replicas' node bags are united by id: a repeated id with
// the same body (cause, kind, value token) is kept once (the copy with the
// smallest source index, a's before b's), with another body it sets
// CW_STATUS_DUP.  The merged nodes come out per document in id order
// (merged_src says where each came from), dense across documents, and go to
// weave_lists_device as an ordinary list batch; ORPHAN, ROOT, NON_LAMPORT and
// KEY_RANGE come from that weave.
//
// Fused route (every document has na + nb <= LU_MAXDOC): k_list_union, one
// workgroup per document, no sort -- Lamport ids are dense, so a bitmap ranks
// them, as in front_doc:
//   1. two bit-planes in LDS in the rank directory's layout (FR_GROUP_BITS ids
//      and a count word per group): a's ids set bits in plane A, b's in plane B,
//      with non-returning LDS atomics, one coalesced pass over each side;
//   2. group prefix counts over A | B, which then replaces plane B: the
//      document's merged count m, and fr_rank on that plane is an id's merged
//      rank; popcount(A) < na or popcount(B) < nb is an id repeated inside one
//      side;
//   3. m is published at once; the document's first merged position comes
//      from a decoupled look-back over the documents (lookback.h; the stage's
//      own words and epochs);
//   4. the merged ids are written straight from plane A | B (a group's set
//      bits are its ids, ranked from its count word on).  The other outputs
//      are placed in LDS first: plane A is done with, and its place plus 64 KiB
//      behind it hold the source index (u16) of every merged rank.  a's nodes
//      fill their slots; after a barrier a b node whose slot is filled has met
//      a's copy of its id and compares the three body fields (DUP), every other
//      b node fills its slot; then cause, kind and merged_src go out in rank
//      order, coalesced, the causes and kinds gathered by source index.  (The
//      first version scattered id, cause, kind and source from the input order
//      to base + rank, four partial-line stores a node into a megabyte a
//      document: 2.88 ms against 1.72 ms at config 2)  53,248
//      ranks fit; a larger document takes two rounds;
//   5. the merged offsets (device u64[D+1]) and the union status.
// Anything outside the scheme -- an id past the planes' range (sparse or wide
// ids, ids >= 2^63) or an id repeated inside one side -- sets a bit in a
// control word and the host reruns the whole call on the general route.
// LDS: 256 B of reduction scratch, 2 planes of FRONT_FUSED_SG groups x 16 B
// (80 KiB) and the 64 KiB of slots: 144.25 KiB, one workgroup of 1,024 threads
// a CU.
//
// General route (a larger document, list_merge_fused = 0, or the control
// word): a then b per document into capacity slots, the segmented radix sort by
// id, k_merge_dedup's count pass, host offsets, its write pass.

constexpr uint32_t LU_NT = 1024;
constexpr uint32_t LU_SG = FRONT_FUSED_SG;              // groups per plane: ids < 245,760
constexpr uint32_t LU_MISC = 256;                       // reduction scratch in front of the planes
constexpr uint32_t LU_SLOTS = 64 * 1024;                // LDS behind the planes for step 4's slots
constexpr uint32_t LU_LDS = LU_MISC + 2 * LU_SG * 16 + LU_SLOTS;  // 144.25 KiB
constexpr uint32_t LU_CHUNK = (LU_SG * 16 + LU_SLOTS) / 2;        // 53,248 ranks a round of step 4
constexpr uint32_t LU_MAXDOC = 0xFFFFu;                 // most input nodes (na + nb) of a document
constexpr uint32_t LU_CTL_FAR = 1, LU_CTL_REPEAT = 2;   // control word: general route instead

struct LuSide {
  const uint64_t *id, *cause, *val;
  const uint8_t *kind;
  const uint32_t *off;  // device [D+1]
};

struct LuOut {
  uint64_t *id, *cause;
  uint8_t *kind;
  uint32_t *src;
  uint64_t *off;     // device [D+1] merged offsets
  uint32_t *status;  // [D] union status
};

// one side's ids into its plane; returns the side's largest id, *far: an id
// past the plane
template <uint32_t U>
__device__ __forceinline__ uint64_t lu_set_bits(const uint64_t *__restrict__ ids, uint32_t n,
                                                uint32_t *sw, bool *far) {
  const uint64_t lim = (uint64_t)LU_SG * FR_GROUP_BITS;
  uint64_t mx = 0;
  for (uint32_t i0 = threadIdx.x; i0 < n; i0 += U * LU_NT) {
    uint64_t x[U];
#pragma unroll
    for (uint32_t u = 0; u < U; u++) {
      const uint32_t i = i0 + u * LU_NT;
      x[u] = i < n ? ids[i] : 0ull;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; u++) {
      if (i0 + u * LU_NT >= n) continue;
      mx = max(mx, x[u]);
      if (x[u] >= lim) {
        *far = true;
        continue;
      }
      const uint32_t xi = (uint32_t)x[u];
      const uint32_t g = xi / FR_GROUP_BITS, b = xi - g * FR_GROUP_BITS;
      atomicOr(&sw[g * 4 + 1 + (b >> 5)], 1u << (b & 31));  // (no returned value)
    }
  }
  return mx;
}

__global__ __launch_bounds__(LU_NT) void k_list_union(LuSide sa, LuSide sb, uint32_t D,
                                                      unsigned long long *lb, uint32_t epoch,
                                                      LuOut out, uint32_t *ctl) {
  extern __shared__ __attribute__((aligned(16))) uint4 lu_lds[];
  uint32_t *const misc = reinterpret_cast<uint32_t *>(lu_lds);
  uint4 *const po = lu_lds + LU_MISC / 16, *const pa = po + LU_SG;  // plane B, then A | B; plane A
  uint16_t *const src16 = reinterpret_cast<uint16_t *>(pa);  // (step 4: plane A's place and on)
  uint32_t *const wtot = misc;                                      // [16]
  uint64_t *const rmax = reinterpret_cast<uint64_t *>(misc + 16);  // [16]
  uint32_t *const s_base = misc + 48, *const s_far = misc + 49, *const s_dup = misc + 50;
  uint32_t *const swa = reinterpret_cast<uint32_t *>(pa), *const swo = reinterpret_cast<uint32_t *>(po);

  const uint32_t d = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const uint32_t a0 = sa.off[d], na = sa.off[d + 1] - a0, b0 = sb.off[d], nb = sb.off[d + 1] - b0;
  const uint64_t *const aid = sa.id + a0, *const bid = sb.id + b0;
  for (uint32_t g = tid; g < LU_MISC / 16 + 2 * LU_SG; g += LU_NT) lu_lds[g] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  // 1. the two planes
  bool far = false;
  uint64_t mx = lu_set_bits<8>(aid, na, swa, &far);
  mx = max(mx, lu_set_bits<8>(bid, nb, swo, &far));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint64_t)__shfl_xor(mx, o, 64));
  if (lane == 0) rmax[tid >> 6] = mx;
  // (flags through the scratch words, zeroed above)
  if (far) *s_far = 1;
  __syncthreads();
  const bool any_far = *s_far != 0;
  mx = rmax[0];
#pragma unroll
  for (uint32_t w = 1; w < LU_NT / 64; w++) mx = max(mx, rmax[w]);
  // 2. group prefix counts over A | B (each thread a contiguous run of groups)
  uint32_t tot = 0;
  bool repeat = false;
  const uint32_t G = any_far ? 0u : (uint32_t)(mx / FR_GROUP_BITS) + 1;
  if (!any_far) {
    const uint32_t per = (G + LU_NT - 1) / LU_NT, g0 = min(G, tid * per), g1 = min(G, g0 + per);
    uint32_t co = 0, cab = 0;  // cab: popcount of A | popcount of B << 16 (each <= 65,535)
    for (uint32_t g = g0; g < g1; g++) {
      const uint4 qa = pa[g], qb = po[g];
      cab += __popc(qa.y) + __popc(qa.z) + __popc(qa.w);
      cab += (uint32_t)(__popc(qb.y) + __popc(qb.z) + __popc(qb.w)) << 16;
      co += __popc(qa.y | qb.y) + __popc(qa.z | qb.z) + __popc(qa.w | qb.w);
    }
    uint32_t sides;
    (void)block_exscan<LU_NT>(cab, wtot, &sides);
    uint32_t run = block_exscan<LU_NT>(co, wtot, &tot);
    repeat = (sides & 0xFFFFu) != na || (sides >> 16) != nb;  // an id twice inside one side
    for (uint32_t g = g0; g < g1; g++) {
      const uint4 qa = pa[g], qb = po[g];
      const uint4 q = make_uint4(run, qa.y | qb.y, qa.z | qb.z, qa.w | qb.w);
      po[g] = q;
      run += __popc(q.y) + __popc(q.z) + __popc(q.w);
    }
  }
  const bool bail = any_far || repeat;  // (uniform: the general route takes the call)
  if (bail) tot = 0;
  // 3. publish this document's merged count, then sum the predecessors' (one wave)
  if (tid == 0) {
    lb_publish(lb, d, epoch, tot);
    if (bail) atomicOr(&ctl[0], any_far ? LU_CTL_FAR : LU_CTL_REPEAT);
  }
  if (bail) return;  // (the successors look past this word; the host discards the call)
  if (tid < 64) {
    const uint32_t base = lb_exclusive(lb, d, epoch, tot);
    if (tid == 0) *s_base = base;
  }
  __syncthreads();  // (also: plane A | B is complete)
  const uint32_t base = *s_base;
  // 4. the source index of every merged rank, in LDS: plane A is done with (a
  // collision shows as a slot an a node has filled), so the slots take its
  // place and the LDS behind it -- LU_CHUNK ranks at a time
  constexpr uint32_t U = 8;
  bool dup = false;
  {
    // the merged ids straight from the plane, as front_doc writes its sorted
    // ids: group g's set bits are ids g * FR_GROUP_BITS + b, ranked from its
    // count word on -- no gather of the ids by source index
    const uint32_t per = (G + LU_NT - 1) / LU_NT, g0 = min(G, tid * per), g1 = min(G, g0 + per);
    for (uint32_t g = g0; g < g1; g++) {
      const uint4 q = po[g];
      uint32_t r = q.x;
      const uint32_t wv[3] = {q.y, q.z, q.w};
#pragma unroll
      for (uint32_t k = 0; k < 3; k++)
        for (uint32_t m = wv[k]; m != 0; m &= m - 1)
          out.id[base + r++] = (uint64_t)g * FR_GROUP_BITS + 32 * k + (uint32_t)(__ffs(m) - 1);
    }
  }
  for (uint32_t r0 = 0; r0 < tot; r0 += LU_CHUNK) {
    const uint32_t len = min(LU_CHUNK, tot - r0);
    for (uint32_t j = tid; j < (len + 1) / 2; j += LU_NT) reinterpret_cast<uint32_t *>(src16)[j] = 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t i0 = tid; i0 < na; i0 += U * LU_NT) {  // 4a. a's nodes
      uint64_t k[U];
#pragma unroll
      for (uint32_t u = 0; u < U; u++) k[u] = i0 + u * LU_NT < na ? aid[i0 + u * LU_NT] : 0ull;
#pragma unroll
      for (uint32_t u = 0; u < U; u++) {
        bool pres;
        const uint32_t r = fr_rank(po, (uint32_t)k[u], &pres) - r0;
        if (i0 + u * LU_NT < na && r < len) src16[r] = (uint16_t)(i0 + u * LU_NT);
      }
    }
    __syncthreads();
    // 4b. b's nodes: a filled slot is a's copy of the id -- the bodies must
    // agree -- every other node takes its slot (ids are distinct inside b, so
    // each slot is read and written by one thread)
    for (uint32_t i0 = tid; i0 < nb; i0 += U * LU_NT) {
      uint64_t k[U];
#pragma unroll
      for (uint32_t u = 0; u < U; u++) k[u] = i0 + u * LU_NT < nb ? bid[i0 + u * LU_NT] : 0ull;
#pragma unroll
      for (uint32_t u = 0; u < U; u++) {
        const uint32_t i = i0 + u * LU_NT;
        bool pres;
        const uint32_t r = fr_rank(po, (uint32_t)k[u], &pres) - r0;
        if (i >= nb || r >= len) continue;
        const uint32_t s = src16[r];
        if (s == 0xFFFFu) {
          src16[r] = (uint16_t)(na + i);
        } else {
          const uint32_t ia = a0 + s, ib = b0 + i;
          dup |= sa.cause[ia] != sb.cause[ib] || sa.kind[ia] != sb.kind[ib] || sa.val[ia] != sb.val[ib];
        }
      }
    }
    __syncthreads();
    // 4c. the merged nodes in rank order: gathered by source, written coalesced
    for (uint32_t j0 = tid; j0 < len; j0 += U * LU_NT) {
      uint64_t c[U];
      uint8_t kd[U];
      uint32_t sv[U];
#pragma unroll
      for (uint32_t u = 0; u < U; u++) {
        const uint32_t j = j0 + u * LU_NT;
        const uint32_t s = j < len ? (uint32_t)src16[j] : 0u;
        const bool fa = s < na;
        const uint32_t g = fa ? a0 + s : b0 + (s - na);
        const bool ok = j < len && s < na + nb;  // (every slot of the round is filled)
        sv[u] = s;
        c[u] = ok ? (fa ? sa.cause[g] : sb.cause[g]) : 0ull;
        kd[u] = ok ? (fa ? sa.kind[g] : sb.kind[g]) : (uint8_t)0;
      }
#pragma unroll
      for (uint32_t u = 0; u < U; u++) {
        const uint32_t j = j0 + u * LU_NT;
        if (j >= len) continue;
        const uint32_t o = base + r0 + j;
        out.cause[o] = c[u];
        out.kind[o] = kd[u];
        out.src[o] = sv[u];
      }
    }
    __syncthreads();
  }
  // 5. merged offsets and the union status
  if (dup) *s_dup = 1;
  __syncthreads();
  const bool any_dup = *s_dup != 0;
  if (tid == 0) {
    out.off[d] = base;
    out.status[d] = any_dup ? (uint32_t)CW_STATUS_DUP : 0u;
    if (d == D - 1) out.off[D] = (uint64_t)base + tot;
  }
}

// The union's bits (DUP) join the weave's status; a document whose merged size
// is 0 has no root.
template <typename OT>
__global__ __launch_bounds__(256) void k_merge_status(const uint32_t *__restrict__ ust,
                                                      const OT *__restrict__ moff,
                                                      uint32_t *__restrict__ status, uint32_t D) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d < D) status[d] |= ust[d] | (moff[d + 1] == moff[d] ? (uint32_t)CW_STATUS_ROOT : 0u);
}

__global__ __launch_bounds__(256) void k_fill_u32(uint32_t *__restrict__ p, uint32_t v, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

namespace {

struct LuHost {  // what merge_lists_impl hands the union stage (device pointers)
  uint64_t D, Na, Nb;
  const uint64_t *ao, *bo;  // host offsets
  LuSide a, b;              // (off: g_aoff / g_boff, uploaded by merge_lists_impl)
  const uint32_t *coff;     // device [D+1] capacity offsets (general route)
  uint64_t *mid, *mca;      // merged ids, causes, kinds, sources, union status
  uint8_t *mkd;
  uint32_t *msrc, *mst;
  uint32_t key_bits;        // in: the caller's; out (general route): the one it found
};

// The fused route.  Returns 1 when it does not apply (the caller takes the
// general route), 0 on success with the merged offsets in `mo` (host) and in
// *dmo_out (device u64[D+1]), -1 on error.
int list_union_fused(cw_ctx *c, LuHost &h, uint64_t *mo, const uint64_t **dmo_out) {
  auto &lm = c->lmerge;
  const uint64_t D = h.D;
  if (!lm.fits || LU_LDS > c->lds_max) return 1;
  uint32_t *ctl = scratch_t<uint32_t>(c, "lm_ctl", 4);
  uint64_t *dmo = scratch_t<uint64_t>(c, "lm_moff", D + 1);
  if (!ctl || !dmo) return fail(c, "out of device memory (list merge)");
  uint32_t epoch;
  unsigned long long *lb = lookback_words(c, lm.lb, "lm_lb", (uint32_t)D, 1, &epoch);
  if (!lb) return -1;
  HIPCHK(c, hipMemsetAsync(ctl, 0, 16, c->stream));
  const LuOut out{h.mid, h.mca, h.mkd, h.msrc, dmo, h.mst};
  const uint64_t NC = h.Na + h.Nb;
  size_t rec = NO_REC;
  {
    // 25 B per input node here; 21 B per merged node join once the count is known
    Launch L(c, "list_union", (double)NC * 25, nullptr, &rec);
    hipLaunchKernelGGL(k_list_union, dim3((uint32_t)D), dim3(LU_NT), LU_LDS, c->stream, h.a, h.b,
                       (uint32_t)D, lb, epoch, out, ctl);
  }
  if (check_launch(c, "list_union")) return -1;
  // (1: ids past the planes, or repeated inside one side)
  const int rc = fused_union_tail(c, rec, ctl, dmo, mo, D, 21);
  if (rc == 0) *dmo_out = dmo;
  return rc;
}

// The general route: concatenation, then union_sort_dedup.  The merged
// offsets: `mo` (host) and *dmo_out (device u32[D+1]).
int list_union_general(cw_ctx *c, LuHost &h, uint64_t *mo, const uint32_t **dmo_out) {
  const uint64_t D = h.D, NC = h.Na + h.Nb;
  uint64_t *cid = scratch_t<uint64_t>(c, "g_cid", NC), *cca = scratch_t<uint64_t>(c, "g_cca", NC),
           *cva = scratch_t<uint64_t>(c, "g_cva", NC);
  uint8_t *ckd = scratch_t<uint8_t>(c, "g_ckd", NC);
  if (!cid || !cca || !cva || !ckd) return fail(c, "out of device memory (merge, N=%llu)", (unsigned long long)NC);
  std::vector<uint64_t> cap(D + 1);
  for (uint64_t d = 0; d <= D; d++) cap[d] = h.ao[d] + h.bo[d];
  // union: a then b per document, in capacity slots
  {
    Launch L(c, "merge_concat", (double)NC * 50);
    hipLaunchKernelGGL(k_merge_concat, dim3((uint32_t)D), dim3(256), 0, c->stream, h.a.id, h.a.cause,
                       h.a.kind, h.a.val, h.b.id, h.b.cause, h.b.kind, h.b.val, h.a.off, h.b.off,
                       h.coff, cid, cca, ckd, cva);
  }
  if (check_launch(c, "merge_concat")) return -1;
  const UnionNames nm{"g_skA",  "g_skB",    "g_svA",       "g_svB",      "g_mcnt",
                      "g_moff", "m_idsort", "merge_count", "merge_write"};
  return union_sort_dedup(c, nm, UnionCat{cid, cca, cva, ckd, h.coff, cap.data()}, D, NC, &h.key_bits, mo,
                          dmo_out, h.mid, h.mca, h.mkd, h.msrc, h.mst);
}

}  // namespace
