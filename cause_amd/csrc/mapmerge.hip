// mapmerge.hip -- the union stage of cw_merge_maps (CausalMap causal-merge,
// map.cljc:248-249 = s/merge-trees, shared.cljc:300-314, with the map weave).
// Included by causeweave.hip after mappack.hip (mp_sort, the pack table)
// and the list merge's kernels (k_merge_dedup), which the general route reuses.
//
// Per collection the two replicas' node bags are united by id: a repeated id
// with the same body (cause, cause_is_id, kind, value token) is kept once (a's
// copy), with another body it sets CW_STATUS_DUP; an id cause that names no
// node of the union sets CW_STATUS_ORPHAN.  The merged nodes come out per
// collection in id order (merged_src says where each came from) and go to
// weave_maps_impl as an ordinary map batch.
//
// Fused route (every collection has na + nb <= MPK): k_map_union, one
// workgroup per pack of whole consecutive collections (<= PK input nodes, <=
// MU_MAXCOLL collections), in LDS:
//   1. both replicas' nodes of the pack into registers (wave-blocked), a's
//      first; bodies to LDS by pack-local index;
//   2. a stable radix sort by (collection in pack, id) carrying the pack-local
//      index: stability puts a's copy of a repeated id first;
//   3. keep = the id differs from its predecessor's; a repeat compares bodies
//      with its predecessor (DUP); a kept id-caused node binary-searches its
//      collection's sorted ids (ORPHAN);
//   4. a block scan of the keep flags: merged positions and per-collection
//      merged starts;
//   5. the pack's first merged node by a decoupled look-back over the packs
//      (lookback.h; the stage's own words and epochs);
//   6. merged id / cause / cause_is_id / kind / source, the merged offsets
//      (device u64[D+1]) and the union status at their final places.
// LDS at PK = 2048: sorted keys, causes, values 3 x 16 KiB, sort values /
// merged positions 4 KiB, kind bytes 2 KiB, sort counters 2.3 KiB, plus 8 B a
// collection of the fullest pack (<= 4 KiB): under 64 KiB.  PK = 512: 19 KiB.
//
// General route (a larger collection, sort keys over 63 bits, or
// map_merge_fused = 0): the list merge's scheme -- a then b per collection into
// capacity slots, the segmented radix sort by id, k_merge_dedup's count pass,
// host offsets, its write pass -- with cause_is_id riding in bits 6-7 of the
// kind byte, then k_mm_finish per collection (unpack, orphan search).

constexpr uint32_t MU_MAXCOLL = 512;  // most collections in one pack (LDS: 8 B each)

// body byte: kind (low 6 bits) | cause_is_id << 6 -- both routes compare and
// carry the same byte, so their results are identical
__host__ __device__ __forceinline__ uint8_t mu_body8(uint8_t kind, uint8_t cis) {
  return (uint8_t)((kind & 0x3Fu) | ((cis & 3u) << 6));
}

struct MuSide {
  const uint64_t *id, *cause, *val;
  const uint8_t *cis, *kind;
  const uint64_t *off;    // device [D+1]
  const uint64_t *pack0;  // device [P+1]: each pack's first node of this side
};

struct MuOut {
  uint64_t *id, *cause;
  uint8_t *cis, *kind;
  uint32_t *src;
  uint64_t *off;     // device [D+1] merged offsets
  uint32_t *status;  // [D] union status
};

template <int PK, int NT>
__global__ __launch_bounds__(NT) void k_map_union(MuSide sa, MuSide sb,
                                                  const uint32_t *__restrict__ pack_doc0, uint32_t P,
                                                  uint32_t D, unsigned long long *lb, uint32_t epoch,
                                                  uint32_t nd_max, MuOut out, uint32_t *ctl) {
  constexpr uint32_t IT = PK / NT;
  __shared__ uint64_t A[PK], C[PK], V[PK];
  __shared__ uint16_t VS[PK];
  __shared__ uint8_t K8[PK];
  extern __shared__ uint32_t mu_dyn[];  // dstat[nd_max], astart[nd_max + 1], bstart[nd_max + 1]
  uint32_t *const dstat = mu_dyn;
  uint16_t *const astart = reinterpret_cast<uint16_t *>(mu_dyn + nd_max);
  uint16_t *const bstart = astart + (nd_max + 1);
  __shared__ uint32_t wcnt[NT / 64][SUB_BINS], run[64], wtot[NT / 64];
  __shared__ uint32_t s_base;
  __shared__ unsigned long long s_or;

  const uint32_t pk = blockIdx.x, tid = threadIdx.x;
  const uint32_t d0 = pack_doc0[pk], nd = pack_doc0[pk + 1] - d0;
  const uint64_t a0 = sa.pack0[pk], b0 = sb.pack0[pk];
  const uint32_t la = (uint32_t)(sa.pack0[pk + 1] - a0), len = la + (uint32_t)(sb.pack0[pk + 1] - b0);
  // 1. the pack's nodes, a's then b's: the loads go out first
  uint64_t lid[IT], lc[IT], lv[IT];
  uint8_t lk[IT];
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) {
    const uint32_t j = wb_elem<IT>(u);
    const bool ok = j < len, fa = j < la;
    const uint64_t g = fa ? a0 + j : b0 + (j - la);
    const uint64_t *pi = fa ? sa.id : sb.id, *pc = fa ? sa.cause : sb.cause, *pv = fa ? sa.val : sb.val;
    const uint8_t *pk8 = fa ? sa.kind : sb.kind, *ps = fa ? sa.cis : sb.cis;
    lid[u] = ok ? pi[g] : 0ull;
    lc[u] = ok ? pc[g] : 0ull;
    lv[u] = ok ? pv[g] : 0ull;
    lk[u] = ok ? mu_body8(pk8[g], ps[g]) : (uint8_t)0;
  }
  for (uint32_t i = tid; i <= nd; i += NT) {
    astart[i] = (uint16_t)(sa.off[d0 + i] - a0);
    bstart[i] = (uint16_t)(sb.off[d0 + i] - b0);
  }
  for (uint32_t i = tid; i < nd; i += NT) dstat[i] = 0;
  if (tid == 0) s_or = 0;
  __syncthreads();

  uint64_t ck[IT];
  uint32_t val[IT], dl0[IT];
  unsigned long long oid = 0;
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) {
    const uint32_t j = wb_elem<IT>(u);
    ck[u] = 0;
    val[u] = 0;
    dl0[u] = 0;
    if (j < len) {
      const bool fa = j < la;
      const uint16_t *st = fa ? astart : bstart;
      const uint32_t jj = fa ? j : j - la;
      uint32_t lo = 0, hi = nd;  // the collection of element j
      while (hi - lo > 1) {
        const uint32_t m = (lo + hi) >> 1;
        if (st[m] <= jj) lo = m; else hi = m;
      }
      C[j] = lc[u];
      V[j] = lv[u];
      K8[j] = lk[u];
      ck[u] = lid[u];
      oid |= lid[u];
      val[u] = j;
      dl0[u] = lo;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) oid |= __shfl_xor(oid, o, 64);
  if ((tid & 63) == 0 && oid) atomicOr(&s_or, oid);
  __syncthreads();
  // 2. stable sort by (collection, id); the key widths are this pack's own
  const uint32_t kbits = s_or ? 64 - __builtin_clzll(s_or) : 1;
  const uint32_t dbits = nd > 1 ? 32 - __builtin_clz(nd - 1) : 0;
  const bool fits = kbits + dbits <= 63;  // otherwise the general route (host)
  if (!fits && tid == 0) atomicOr(&ctl[0], 1u);
  const uint32_t ksh = fits ? kbits : 63;  // (keys are 0 then: collection 0)
  const uint64_t imask = (1ull << min(kbits, 63u)) - 1;
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) ck[u] = fits ? (((uint64_t)dl0[u] << kbits) | ck[u]) : 0ull;
  mp_sort<NT, IT>(ck, val, len, fits ? kbits + dbits : 1, A, VS, wcnt, run);

  // 3. keep flags, body conflicts, orphans -- item u is sorted position wb_elem(u)
  bool keep[IT];
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) {
    const uint32_t i = wb_elem<IT>(u);
    keep[u] = false;
    if (i >= len) continue;
    const uint32_t dl = (uint32_t)(ck[u] >> ksh), j = val[u];
    keep[u] = i == 0 || A[i - 1] != ck[u];
    if (!keep[u]) {  // a repeated id: the same body, or edits-not-allowed
      const uint32_t jp = VS[i - 1];
      if (C[jp] != C[j] || V[jp] != V[j] || K8[jp] != K8[j]) atomicOr(&dstat[dl], (uint32_t)CW_STATUS_DUP);
    } else if ((K8[j] >> 6) == 1) {  // an id cause must name a node of the union
      const uint64_t c = C[j], want = ((uint64_t)dl << ksh) | c;
      uint32_t lo = (uint32_t)astart[dl] + bstart[dl];
      const uint32_t e1 = (uint32_t)astart[dl + 1] + bstart[dl + 1];
      uint32_t hi = e1;
      const bool inrange = (c & ~imask) == 0;
      while (inrange && lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        if (A[m] < want) lo = m + 1; else hi = m;
      }
      if (!(inrange && lo < e1 && A[lo] == want)) atomicOr(&dstat[dl], (uint32_t)CW_STATUS_ORPHAN);
    }
  }
  // 4. merged position = kept nodes before me: ballots inside a row of 64, the
  // wave's rows in order, then the waves
  uint32_t pos[IT], rowsum = 0;
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) {
    const uint64_t m = __ballot(keep[u]);
    pos[u] = rowsum + lanes_below(m);
    rowsum += (uint32_t)__popcll(m);
  }
  if ((tid & 63) == 0) wtot[tid >> 6] = rowsum;
  __syncthreads();  // (also: every VS read of step 3 is done)
  uint32_t before = 0, tot = 0;
#pragma unroll
  for (uint32_t w = 0; w < NT / 64; w++) {
    const uint32_t t = wtot[w];
    before += w < (tid >> 6) ? t : 0u;
    tot += t;
  }
  uint16_t *const POS = VS;  // exclusive count of kept nodes at each sorted position
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) {
    pos[u] += before;
    if (wb_elem<IT>(u) < len) POS[wb_elem<IT>(u)] = (uint16_t)pos[u];
  }
  // 5. publish this pack's merged count, then sum the predecessors' (one wave)
  if (tid == 0) lb_publish(lb, pk, epoch, tot);
  if (tid < 64) {
    const uint32_t base = lb_exclusive(lb, pk, epoch, tot);
    if (tid == 0) s_base = base;
  }
  __syncthreads();
  const uint32_t base = s_base;
  // 6. outputs at their final places
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) {
    if (!keep[u]) continue;
    const uint32_t dl = (uint32_t)(ck[u] >> ksh), j = val[u];
    const uint32_t o = base + pos[u];
    const uint8_t k8 = K8[j];
    const uint32_t na = (uint32_t)astart[dl + 1] - astart[dl];
    out.id[o] = ck[u] & imask;
    out.cause[o] = C[j];
    out.cis[o] = (uint8_t)(k8 >> 6);
    out.kind[o] = (uint8_t)(k8 & 0x3Fu);
    out.src[o] = j < la ? j - astart[dl] : na + (j - la - bstart[dl]);
  }
  for (uint32_t dl = tid; dl < nd; dl += NT) {
    const uint32_t cs = (uint32_t)astart[dl] + bstart[dl];
    out.off[d0 + dl] = (uint64_t)base + (cs < len ? (uint32_t)POS[cs] : tot);
    out.status[d0 + dl] = dstat[dl];
  }
  if (pk == P - 1 && tid == 0) out.off[D] = (uint64_t)base + tot;
}

// General route.  Collection d's a-nodes then b-nodes into one capacity slot
// [coff[d], coff[d+1]); the kind byte carries cause_is_id (mu_body8).
__global__ __launch_bounds__(256) void k_mm_concat(MuSide sa, MuSide sb,
                                                   const uint32_t *__restrict__ coff,
                                                   uint64_t *__restrict__ cid,
                                                   uint64_t *__restrict__ ccause,
                                                   uint8_t *__restrict__ ckind,
                                                   uint64_t *__restrict__ cval) {
  const uint32_t d = blockIdx.x;
  const uint64_t a0 = sa.off[d], b0 = sb.off[d];
  const uint32_t na = (uint32_t)(sa.off[d + 1] - a0), nb = (uint32_t)(sb.off[d + 1] - b0);
  const uint32_t c0 = coff[d];
  for (uint32_t i = threadIdx.x; i < na + nb; i += blockDim.x) {
    const bool fa = i < na;
    const uint64_t g = fa ? a0 + i : b0 + (i - na);
    cid[c0 + i] = fa ? sa.id[g] : sb.id[g];
    ccause[c0 + i] = fa ? sa.cause[g] : sb.cause[g];
    ckind[c0 + i] = fa ? mu_body8(sa.kind[g], sa.cis[g]) : mu_body8(sb.kind[g], sb.cis[g]);
    cval[c0 + i] = fa ? sa.val[g] : sb.val[g];
  }
}

// Merged collection d = [moff[d], moff[d+1]), ids ascending: the kind byte is
// unpacked into kind and cause_is_id, and every id cause is searched among the
// collection's ids (a miss: CW_STATUS_ORPHAN).
__global__ __launch_bounds__(256) void k_mm_finish(const uint64_t *__restrict__ mid,
                                                   const uint64_t *__restrict__ mcause,
                                                   const uint32_t *__restrict__ moff,
                                                   uint8_t *__restrict__ mkind,
                                                   uint8_t *__restrict__ mcis,
                                                   uint32_t *__restrict__ mstatus) {
  const uint32_t d = blockIdx.x, m0 = moff[d], m1 = moff[d + 1];
  bool orphan = false;
  for (uint32_t i = m0 + threadIdx.x; i < m1; i += blockDim.x) {
    const uint8_t k8 = mkind[i], cis = (uint8_t)(k8 >> 6);
    mkind[i] = (uint8_t)(k8 & 0x3Fu);
    mcis[i] = cis;
    if (cis != 1) continue;
    const uint64_t want = mcause[i];
    uint32_t lo = m0, hi = m1;
    while (lo < hi) {
      const uint32_t m = (lo + hi) >> 1;
      if (mid[m] < want) lo = m + 1; else hi = m;
    }
    orphan |= !(lo < m1 && mid[lo] == want);
  }
  if (__syncthreads_or(orphan) && threadIdx.x == 0) mstatus[d] |= CW_STATUS_ORPHAN;
}

namespace {

// ---- the union scaffold shared with listmerge.hip ----

// After a fused union kernel (k_map_union, k_list_union): the stage's one
// device-to-host copy -- the control word and the merged offsets (device
// u64[D+1] -> mo) in one wait.  Returns 1 when the kernel handed the call to
// the general route, else 0; the launch's profiling record `rec` gets its
// bytes: none then, else out_bytes more per merged node.
int fused_union_tail(cw_ctx *c, size_t rec, const uint32_t *ctl, const uint64_t *dmo, uint64_t *mo,
                     uint64_t D, double out_bytes) {
  const uint32_t *pc = read_small(c, ctl, 4, NO_WAIT);
  if (!pc) return -1;
  HIPCHK(c, hipMemcpyAsync(mo, dmo, (D + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const bool bail = pc[0] != 0;
  if (rec < c->pending.size()) c->pending[rec].bytes = bail ? 0 : c->pending[rec].bytes + (double)mo[D] * out_bytes;
  return bail;
}

struct UnionNames {  // a caller's scratch and kernel stat names
  const char *skA, *skB, *svA, *svB, *cnt, *moff, *idsort, *count, *write;
};
struct UnionCat {  // the two sides in capacity slots: a's nodes then b's per document
  const uint64_t *id, *cause, *val;
  const uint8_t *kind;
  const uint32_t *coff;  // device [D+1]
  const uint64_t *cap;   // the same on the host
};

// The general route after the concatenation: id order per capacity slot (the
// segmented radix sort), k_merge_dedup's count pass, a host scan of the counts,
// its write pass.  The merged offsets: mo (host) and *dmo_out (device u32[D+1]);
// *key_bits == 0: found here.
int union_sort_dedup(cw_ctx *c, const UnionNames &nm, const UnionCat &cat, uint64_t D, uint64_t NC,
                     uint32_t *key_bits, uint64_t *mo, const uint32_t **dmo_out, uint64_t *mid,
                     uint64_t *mca, uint8_t *mkd, uint32_t *msrc, uint32_t *mst) {
  uint32_t *dmo = scratch_t<uint32_t>(c, nm.moff, D + 1), *mcnt = scratch_t<uint32_t>(c, nm.cnt, D + 1);
  uint64_t *skA = scratch_t<uint64_t>(c, nm.skA, NC), *skB = scratch_t<uint64_t>(c, nm.skB, NC);
  uint32_t *svA = scratch_t<uint32_t>(c, nm.svA, NC), *svB = scratch_t<uint32_t>(c, nm.svB, NC);
  if (!dmo || !mcnt || !skA || !skB || !svA || !svB)
    return fail(c, "out of device memory (merge, N=%llu)", (unsigned long long)NC);
  if (ensure_tables(c, D, cat.cap)) return -1;
  if (*key_bits == 0 && find_key_bits(c, cat.id, (uint32_t)NC, key_bits)) return -1;
  uint64_t *skey;
  uint32_t *sval;
  if (radix_sort<uint64_t>(c, nm.idsort, cat.id, nullptr, skA, svA, skB, svB, *key_bits, 0, (uint32_t)NC,
                           &skey, &sval))
    return -1;
  auto dedup = [&](const char *stat, int pass, double bytes) {
    {
      Launch L(c, stat, bytes);
      hipLaunchKernelGGL((k_merge_dedup<1024>), dim3((uint32_t)D), dim3(1024), 0, c->stream, skey, sval,
                         cat.cause, cat.kind, cat.val, cat.coff, pass, mcnt, dmo, mid, mca, mkd, msrc, mst);
    }
    return check_launch(c, stat);
  };
  if (dedup(nm.count, 0, (double)NC * 12)) return -1;
  if (scan_counts(c, mcnt, D, mo, dmo)) return -1;
  if (dedup(nm.write, 1, (double)NC * 12 + (double)mo[D] * 21)) return -1;
  *dmo_out = dmo;
  return 0;
}

// ---- cw_merge_maps ----

struct MuHost {  // what merge_maps_impl hands the union stage (device pointers)
  uint64_t D, Na, Nb;
  const uint64_t *ao, *bo;  // host offsets
  MuSide a, b;              // (off / pack0 filled in by the routes)
  MuOut out;                // (off filled in by the fused route)
  uint32_t key_bits;
};

// The fused route.  Returns 1 when it does not apply (the caller takes the
// general route), 0 on success with the merged offsets in `mo` (host), -1 on
// error.
int map_union_fused(cw_ctx *c, MuHost &h, uint64_t *mo) {
  const uint64_t D = h.D, *ao = h.ao, *bo = h.bo;
  auto &mm = c->mmerge;
  if (pack_table(c, mm, false, D, ao, bo, MPK, MU_MAXCOLL, 0,
                 PackNames{"mm_doc0", "mm_pa0", "mm_pb0", "mm_aoff", "mm_boff"}))
    return -1;
  if (!mm.ok) return 1;
  const uint32_t P = (uint32_t)mm.doc0.size() - 1;
  const uint64_t NC = h.Na + h.Nb;
  uint32_t *ctl = scratch_t<uint32_t>(c, "mm_ctl", 4);
  uint64_t *dmo = scratch_t<uint64_t>(c, "mm_moff", D + 1);
  if (!ctl || !dmo) return fail(c, "out of device memory (map merge)");
  uint32_t epoch;
  unsigned long long *lb = lookback_words(c, mm.lb, "mm_lb", P, 1, &epoch);
  if (!lb) return -1;
  HIPCHK(c, hipMemsetAsync(ctl, 0, 16, c->stream));
  h.a.off = (const uint64_t *)c->bufs["mm_aoff"].p;
  h.b.off = (const uint64_t *)c->bufs["mm_boff"].p;
  h.a.pack0 = (const uint64_t *)c->bufs["mm_pa0"].p;
  h.b.pack0 = (const uint64_t *)c->bufs["mm_pb0"].p;
  h.out.off = dmo;
  const uint32_t *dp = (const uint32_t *)c->bufs["mm_doc0"].p;
  const size_t dyn = (size_t)mm.dmax * 4 + (size_t)(mm.dmax + 1) * 4;
  size_t rec = NO_REC;
  {
    // 26 B per input node here; 22 B per merged node join once the count is known
    Launch L(c, "map_union", (double)NC * 26, nullptr, &rec);
    CW_PK_LAUNCH(k_map_union, mm.pk, P, dyn, c->stream, h.a, h.b, dp, P, (uint32_t)D, lb, epoch, mm.dmax,
                 h.out, ctl);
  }
  if (check_launch(c, "map_union")) return -1;
  return fused_union_tail(c, rec, ctl, dmo, mo, D, 22);  // (1: a pack's sort keys need more than 63 bits)
}

// The general route: the list merge's scheme with map bodies.
int map_union_general(cw_ctx *c, MuHost &h, uint64_t *mo) {
  const uint64_t D = h.D, *ao = h.ao, *bo = h.bo, NC = h.Na + h.Nb;
  if (!grid_ok(D, 1024)) return fail(c, "batch too large for one dispatch");
  std::vector<uint64_t> cap(D + 1);
  std::vector<uint32_t> h_co(D + 1);
  for (uint64_t d = 0; d <= D; d++) {
    cap[d] = ao[d] + bo[d];
    h_co[d] = (uint32_t)cap[d];
  }
  uint64_t *dao = scratch_t<uint64_t>(c, "mm_aoff", D + 1), *dbo = scratch_t<uint64_t>(c, "mm_boff", D + 1);
  uint32_t *dco = scratch_t<uint32_t>(c, "mm_coff", D + 1);
  uint64_t *cid = scratch_t<uint64_t>(c, "mm_cid", NC), *cca = scratch_t<uint64_t>(c, "mm_cca", NC),
           *cva = scratch_t<uint64_t>(c, "mm_cva", NC);
  uint8_t *ckd = scratch_t<uint8_t>(c, "mm_ckd", NC);
  if (!dao || !dbo || !dco || !cid || !cca || !cva || !ckd)
    return fail(c, "out of device memory (map merge, N=%llu)", (unsigned long long)NC);
  c->mmerge.clear();  // (mm_aoff / mm_boff are rewritten: the fused route's cache is void)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(dao, ao, (D + 1) * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dbo, bo, (D + 1) * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dco, h_co.data(), (D + 1) * 4, hipMemcpyHostToDevice));
  h.a.off = dao;
  h.b.off = dbo;
  // 1. union: a then b per collection, in capacity slots
  {
    Launch L(c, "mm_concat", (double)NC * 52);
    hipLaunchKernelGGL(k_mm_concat, dim3((uint32_t)D), dim3(256), 0, c->stream, h.a, h.b, dco, cid, cca,
                       ckd, cva);
  }
  if (check_launch(c, "mm_concat")) return -1;
  // 2. id sort and dedup (scratch names of its own: weave_maps_impl reuses the lists')
  const UnionNames nm{"mm_skA",    "mm_skB",    "mm_svA",   "mm_svB",  "mm_cnt",
                      "mm_moff32", "mm_idsort", "mm_count", "mm_write"};
  const uint32_t *dmo;
  uint32_t key_bits = h.key_bits;
  if (union_sort_dedup(c, nm, UnionCat{cid, cca, cva, ckd, dco, cap.data()}, D, NC, &key_bits, mo, &dmo,
                       h.out.id, h.out.cause, h.out.kind, h.out.src, h.out.status))
    return -1;
  // 3. kind / cause_is_id apart again, and the orphan search
  {
    Launch L(c, "mm_finish", (double)mo[D] * 19);
    hipLaunchKernelGGL(k_mm_finish, dim3((uint32_t)D), dim3(256), 0, c->stream, h.out.id, h.out.cause, dmo,
                       h.out.kind, h.out.cis, h.out.status);
  }
  return check_launch(c, "mm_finish");
}

}  // namespace
