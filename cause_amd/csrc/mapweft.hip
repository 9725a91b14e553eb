// mapweft.hip -- the select stage of cw_weft_maps (CausalMap weft, map.cljc:
// 246-247 = s/weft, shared.cljc:268-293, with the map weave).  Included by
// causeweave.hip after mapmerge.hip (the pack table helpers of mappack.hip,
// lookback.h).
//
// Per collection the cut table names at most one cut id per site rank
// (cut[(d << site_bits) | rank], 0 = not named).  A node is kept when its site
// is named and either the cut id is no node of the collection (take-while never
// stops: the whole yarn) or its id is <= the cut.  Every named cut that is no
// node adds the one-element node [id]: cause nil (cause_is_id = 2), kind
// normal, kept_src = UINT32_MAX.  The kept nodes come out per collection in
// input order, then its [id] nodes by site rank, and go to weave_maps_impl as
// an ordinary map batch.
//
// Fused route (every collection has <= MPK nodes): k_map_weft, one workgroup
// per pack of whole consecutive collections (<= PK nodes, <= MW_MAXCOLL
// collections, <= MW_SLOTS cut slots = collections << site_bits):
//   1. the pack's ids, causes and body bytes into registers (wave-blocked);
//   2. each element's collection by binary search over the pack's starts (LDS);
//   3. found bits over (collection in pack, site rank): a node sets its bit
//      when its id is its site's cut;
//   4. keep = the site is named and (its cut was not found or id <= cut);
//   5. a block scan of the keep flags, in input order (ballots a row of 64,
//      the wave's rows, the waves);
//   6. a second scan over the pack's cut slots: named and not found, the [id]
//      nodes; each wave takes a run of whole rows of 64 slots;
//   7. the pack's first kept position by a decoupled look-back over the packs
//      (lookback.h; the stage's own words and epochs);
//   8. kept id / cause / cause_is_id / kind / source, the [id] nodes, the kept
//      offsets (device u64[D+1]) and the WEFT word at their final places.
// Nothing is sorted and no node passes through LDS.  LDS at PK = 2048: kept
// positions 4 KiB, found bits 512 B, 8 B a collection of the fullest pack
// (<= 4 KiB), the waves' totals: under 9 KiB (PK = 512: under 6 KiB).
//
// General route (a larger collection, or map_weft_fused = 0): k_mw_select, a
// workgroup per collection: a count pass, a host scan of the counts, a write
// pass -- k_weft_select's scheme carrying cause_is_id.

constexpr uint32_t MW_MAXCOLL = 512;  // most collections in one pack (LDS: 8 B each)
constexpr uint32_t MW_SLOTS = 4096;   // most cut slots in one pack (LDS: the found bits)

struct MwIn {
  const uint64_t *id, *cause;
  const uint8_t *cis, *kind;
  const uint64_t *off;  // device [D+1]
  const uint64_t *cut;  // device [D << site_bits]
  uint32_t site_shift, site_bits;
};

struct MwOut {
  uint64_t *id, *cause;
  uint8_t *cis, *kind;
  uint32_t *src;
  uint64_t *off;   // device [D+1] kept offsets (the fused route)
  uint32_t *weft;  // [D] CW_STATUS_WEFT or 0
};

// one [id] node: (new-node [id nil]) destructured by map.cljc:30 -- cause nil
__device__ __forceinline__ void mw_bogus(const MwOut &out, uint32_t o, uint64_t cutid) {
  out.id[o] = cutid;
  out.cause[o] = 0;
  out.cis[o] = 2;
  out.kind[o] = 0;
  out.src[o] = 0xFFFFFFFFu;
}

template <int PK, int NT>
__global__ __launch_bounds__(NT) void k_map_weft(MwIn in, const uint32_t *__restrict__ pack_doc0,
                                                 const uint64_t *__restrict__ pack_s0, uint32_t P,
                                                 uint32_t D, unsigned long long *lb, uint32_t epoch,
                                                 uint32_t nd_max, MwOut out) {
  constexpr uint32_t IT = PK / NT, NW = NT / 64;
  __shared__ uint16_t POS[PK];  // exclusive count of kept nodes at each pack-local index
  __shared__ uint32_t found[MW_SLOTS / 32];
  extern __shared__ uint32_t mw_dyn[];  // dstart[nd_max + 1], mstart[nd_max + 1]
  uint32_t *const dstart = mw_dyn, *const mstart = mw_dyn + (nd_max + 1);
  __shared__ uint32_t wtotK[NW], wtotM[NW];
  __shared__ uint32_t s_base;

  const uint32_t pk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t d0 = pack_doc0[pk], nd = pack_doc0[pk + 1] - d0;
  const uint64_t s0 = pack_s0[pk];
  const uint32_t len = (uint32_t)(pack_s0[pk + 1] - s0);
  const uint32_t sb = in.site_bits, smask = (1u << sb) - 1, nslot = nd << sb;
  const uint64_t *const crow = in.cut + ((uint64_t)d0 << sb);  // the pack's cut rows are one run
  // 1. the pack's nodes: the loads go out first
  uint64_t lid[IT], lc[IT];
  uint8_t lk[IT], ls[IT];
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) {
    const uint32_t j = wb_elem<IT>(u);
    const bool ok = j < len;
    lid[u] = ok ? in.id[s0 + j] : 0ull;
    lc[u] = ok ? in.cause[s0 + j] : 0ull;
    lk[u] = ok ? in.kind[s0 + j] : (uint8_t)0;
    ls[u] = ok ? in.cis[s0 + j] : (uint8_t)0;
  }
  for (uint32_t i = tid; i <= nd; i += NT) dstart[i] = (uint32_t)(in.off[d0 + i] - s0);
  for (uint32_t i = tid; i < MW_SLOTS / 32; i += NT) found[i] = 0;
  __syncthreads();

  // 2, 3. the collection of each element, its site's cut word, the found bits
  uint32_t dl[IT], slot[IT];
  uint64_t cw[IT];
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) {
    const uint32_t j = wb_elem<IT>(u);
    dl[u] = 0;
    slot[u] = 0;
    cw[u] = 0;
    if (j < len) {
      uint32_t lo = 0, hi = nd;
      while (hi - lo > 1) {
        const uint32_t m = (lo + hi) >> 1;
        if (dstart[m] <= j) lo = m; else hi = m;
      }
      dl[u] = lo;
      slot[u] = (lo << sb) | ((uint32_t)(lid[u] >> in.site_shift) & smask);  // (< nslot)
      cw[u] = crow[slot[u]];
      if (cw[u] != 0 && cw[u] == lid[u]) atomicOr(&found[slot[u] >> 5], 1u << (slot[u] & 31));
    }
  }
  __syncthreads();

  // 4, 5. keep flags and kept position = kept nodes before me: ballots inside
  // a row of 64, the wave's rows in order, then the waves
  bool keep[IT];
  uint32_t pos[IT], rowsum = 0;
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) {
    const bool hit = (found[slot[u] >> 5] >> (slot[u] & 31)) & 1u;
    keep[u] = cw[u] != 0 && (!hit || lid[u] <= cw[u]);  // (cw = 0 past the pack's end)
    const uint64_t m = __ballot(keep[u]);
    pos[u] = rowsum + lanes_below(m);
    rowsum += (uint32_t)__popcll(m);
  }
  // 6. the named cuts that were not found, in slot order: wave w takes the
  // rows [w * rpw, (w + 1) * rpw) of 64 slots; mstart[i] = the count before
  // collection i's first slot, inside its wave for now
  const uint32_t rows = (nslot + 63) >> 6, rpw = (rows + NW - 1) / NW;
  const uint32_t r0 = min(w * rpw, rows), r1 = min(r0 + rpw, rows);
  uint32_t msum = 0;
  for (uint32_t r = r0; r < r1; r++) {
    const uint32_t s = (r << 6) + lane;
    const uint64_t word = s < nslot ? crow[s] : 0ull;
    const bool miss = word != 0 && !((found[s >> 5] >> (s & 31)) & 1u);
    const uint64_t m = __ballot(miss);
    if (s < nslot && (s & smask) == 0) mstart[s >> sb] = msum + lanes_below(m);
    msum += (uint32_t)__popcll(m);
  }
  if (lane == 0) {
    wtotK[w] = rowsum;
    wtotM[w] = msum;
  }
  __syncthreads();
  uint32_t beforeK = 0, totK = 0, beforeM = 0, totM = 0;
#pragma unroll
  for (uint32_t v = 0; v < NW; v++) {
    const uint32_t a = wtotK[v], b = wtotM[v];
    beforeK += v < w ? a : 0u;
    totK += a;
    beforeM += v < w ? b : 0u;
    totM += b;
  }
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) {
    pos[u] += beforeK;
    if (wb_elem<IT>(u) < len) POS[wb_elem<IT>(u)] = (uint16_t)pos[u];
  }
  for (uint32_t i = tid; i < nd; i += NT) {  // the earlier waves' counts join mstart
    const uint32_t wv = ((i << sb) >> 6) / rpw;
    uint32_t add = 0;
#pragma unroll
    for (uint32_t v = 0; v < NW; v++) add += v < wv ? wtotM[v] : 0u;
    mstart[i] += add;
  }
  if (tid == 0) mstart[nd] = totM;
  // 7. publish this pack's kept count, then sum the predecessors' (one wave)
  const uint32_t tot = totK + totM;
  if (tid == 0) lb_publish(lb, pk, epoch, tot);
  if (tid < 64) {
    const uint32_t b = lb_exclusive(lb, pk, epoch, tot);
    if (tid == 0) s_base = b;
  }
  __syncthreads();
  const uint32_t base = s_base;
  // 8. outputs at their final places: a collection's kept nodes, then its [id] nodes
#pragma unroll
  for (uint32_t u = 0; u < IT; u++) {
    if (!keep[u]) continue;
    const uint32_t o = base + pos[u] + mstart[dl[u]];
    out.id[o] = lid[u];
    out.cause[o] = lc[u];
    out.cis[o] = ls[u];
    out.kind[o] = lk[u];
    out.src[o] = wb_elem<IT>(u) - dstart[dl[u]];
  }
  msum = beforeM;
  for (uint32_t r = r0; r < r1; r++) {
    const uint32_t s = (r << 6) + lane;
    const uint64_t word = s < nslot ? crow[s] : 0ull;
    const bool miss = word != 0 && !((found[s >> 5] >> (s & 31)) & 1u);
    const uint64_t m = __ballot(miss);
    if (miss) {
      const uint32_t e = dstart[(s >> sb) + 1];  // kept nodes up to the collection's end
      mw_bogus(out, base + (e < len ? (uint32_t)POS[e] : totK) + msum + lanes_below(m), word);
    }
    msum += (uint32_t)__popcll(m);
  }
  for (uint32_t i = tid; i < nd; i += NT) {
    const uint32_t b = dstart[i];
    out.off[d0 + i] = (uint64_t)base + (b < len ? (uint32_t)POS[b] : totK) + mstart[i];
    out.weft[d0 + i] = mstart[i + 1] != mstart[i] ? (uint32_t)CW_STATUS_WEFT : 0u;
  }
  if (pk == P - 1 && tid == 0) out.off[D] = (uint64_t)base + tot;
}

// General route: collection d alone, of any size.  pass 0 counts (kcount[d],
// the WEFT word), pass 1 writes at koff[d]: the kept nodes in input order,
// then the [id] nodes by site rank.
template <int NT>
__global__ __launch_bounds__(NT) void k_mw_select(MwIn in, int pass, uint32_t *__restrict__ kcount,
                                                  const uint32_t *__restrict__ koff, MwOut out) {
  __shared__ uint32_t wtot[NT / 64];
  __shared__ uint32_t found[1024 / 32];
  const uint32_t d = blockIdx.x;
  const uint64_t base = in.off[d];
  const uint32_t n = (uint32_t)(in.off[d + 1] - base);
  const uint32_t S = 1u << in.site_bits, smask = S - 1;
  const uint64_t *const dc = in.cut + ((uint64_t)d << in.site_bits);
  for (uint32_t i = threadIdx.x; i < 1024 / 32; i += NT) found[i] = 0;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += NT) {  // which cut ids are nodes
    const uint64_t k = in.id[base + i];
    const uint32_t site = (uint32_t)(k >> in.site_shift) & smask;
    if (dc[site] != 0 && k == dc[site]) atomicOr(&found[site >> 5], 1u << (site & 31));
  }
  __syncthreads();
  uint32_t run = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += NT) {
    const uint32_t i = i0 + threadIdx.x;
    bool keep = false;
    uint64_t k = 0;
    if (i < n) {
      k = in.id[base + i];
      const uint32_t site = (uint32_t)(k >> in.site_shift) & smask;
      const uint64_t c = dc[site];
      const bool hit = (found[site >> 5] >> (site & 31)) & 1u;
      keep = c != 0 && (!hit || k <= c);
    }
    uint32_t tot;
    const uint32_t pos = run + block_exscan<NT>(keep ? 1u : 0u, wtot, &tot);
    if (pass == 1 && keep) {
      const uint32_t o = koff[d] + pos;
      out.id[o] = k;
      out.cause[o] = in.cause[base + i];
      out.cis[o] = in.cis[base + i];
      out.kind[o] = in.kind[base + i];
      out.src[o] = i;
    }
    run += tot;
  }
  uint32_t miss = 0;
  for (uint32_t s0 = 0; s0 < S; s0 += NT) {
    const uint32_t s = s0 + threadIdx.x;
    const bool m = s < S && dc[s] != 0 && !((found[s >> 5] >> (s & 31)) & 1u);
    uint32_t tot;
    const uint32_t pos = run + miss + block_exscan<NT>(m ? 1u : 0u, wtot, &tot);
    if (pass == 1 && m) mw_bogus(out, koff[d] + pos, dc[s]);
    miss += tot;
  }
  if (pass == 0 && threadIdx.x == 0) {
    kcount[d] = run + miss;
    out.weft[d] = miss ? (uint32_t)CW_STATUS_WEFT : 0u;
  }
}

namespace {

struct MwHost {  // what weft_maps_impl hands the select stage (device pointers)
  uint64_t D, N;
  const uint64_t *off;  // host offsets
  MwIn in;              // (off filled in by the routes)
  MwOut out;            // (off filled in by the fused route)
};

// The fused route.  Returns 1 when it does not apply (the caller takes the
// general route), 0 on success with the kept offsets in `ko` (host), -1 on
// error.
int map_weft_fused(cw_ctx *c, MwHost &h, uint64_t *ko) {
  const uint64_t D = h.D, *off = h.off;
  const uint32_t sb = h.in.site_bits;
  auto &mw = c->mweft;
  // (a pack's collections << site_bits stay within the found bits)
  if (pack_table(c, mw, false, D, off, nullptr, MPK, std::min<uint64_t>(MW_MAXCOLL, MW_SLOTS >> sb), sb,
                 PackNames{"mw_doc0", "mw_s0", nullptr, "mw_off", nullptr}))
    return -1;
  if (!mw.ok) return 1;
  const uint32_t P = (uint32_t)mw.doc0.size() - 1;
  uint64_t *dko = scratch_t<uint64_t>(c, "mw_koff", D + 1);
  if (!dko) return fail(c, "out of device memory (map weft)");
  uint32_t epoch;
  unsigned long long *lb = lookback_words(c, mw.lb, "mw_lb", P, 1, &epoch);
  if (!lb) return -1;
  h.in.off = (const uint64_t *)c->bufs["mw_off"].p;
  h.out.off = dko;
  const size_t dyn = (size_t)(mw.dmax + 1) * 8;
  size_t rec = NO_REC;
  {
    // per node 18 B and its cut word, per cut slot 8 B, per collection its
    // offset in and out and the WEFT word; 22 B per kept node join once the
    // count is known
    Launch L(c, "map_weft", (double)h.N * 26 + (double)(D << sb) * 8 + (double)D * 20, nullptr, &rec);
    CW_PK_LAUNCH(k_map_weft, mw.pk, P, dyn, c->stream, h.in, (const uint32_t *)c->bufs["mw_doc0"].p,
                 (const uint64_t *)c->bufs["mw_s0"].p, P, (uint32_t)D, lb, epoch, mw.dmax, h.out);
  }
  if (check_launch(c, "map_weft")) return -1;
  // the stage's one device-to-host copy: they are the weave's coll_offsets
  HIPCHK(c, hipMemcpyAsync(ko, dko, (D + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (rec < c->pending.size()) c->pending[rec].bytes += (double)ko[D] * 22;
  return 0;
}

// The general route: count pass, host scan, write pass.
int map_weft_general(cw_ctx *c, MwHost &h, uint64_t *ko) {
  const uint64_t D = h.D;
  const uint32_t sb = h.in.site_bits;
  if (!grid_ok(D, 1024)) return fail(c, "batch too large for one dispatch");
  uint64_t *dof = scratch_t<uint64_t>(c, "mw_off", D + 1);
  uint32_t *kcnt = scratch_t<uint32_t>(c, "mw_kcnt", D), *koff = scratch_t<uint32_t>(c, "mw_koff32", D + 1);
  if (!dof || !kcnt || !koff) return fail(c, "out of device memory (map weft)");
  c->mweft.clear();  // (mw_off is rewritten: the fused route's cache is void)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(dof, h.off, (D + 1) * 8, hipMemcpyHostToDevice));
  h.in.off = dof;
  auto select = [&](const char *stat, int pass, double bytes) {
    {
      Launch L(c, stat, bytes);
      hipLaunchKernelGGL((k_mw_select<1024>), dim3((uint32_t)D), dim3(1024), 0, c->stream, h.in, pass, kcnt,
                         koff, h.out);
    }
    return check_launch(c, stat);
  };
  // ids and their cut words twice, the cut slots once
  if (select("mw_count", 0, (double)h.N * 32 + (double)(D << sb) * 8 + (double)D * 24)) return -1;
  if (scan_counts(c, kcnt, D, ko, koff)) return -1;
  return select("mw_write", 1,
                (double)h.N * 32 + (double)(D << sb) * 8 + (double)D * 20 + (double)ko[D] * 22);
}

}  // namespace
