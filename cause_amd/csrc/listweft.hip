// listweft.hip -- the select stage of cw_weft_lists / cw_weft_lists_dev (s/weft
// on a CausalList, shared.cljc:268-293; k_weft_select in causeweave.hip states
// the rule).  Included by causeweave.hip after listmerge.hip (lookback.h).
//
// Per document the cut table names at most one cut id per site rank
// (cut[(d << site_bits) | rank], 0 = not named).  A node is kept when it is the
// root, or its site is named and either the cut id is no node of the document
// (the whole yarn) or its id is <= the cut.  Every named cut that is no node
// adds the one-element node [id]: cause CW_NIL, kind normal, kept_src =
// UINT32_MAX.  The kept nodes come out per document in input order, then its
// [id] nodes by site rank, and go to weave_lists_device as an ordinary batch.
//
// Fused route (every document has <= LW_MAXDOC nodes): k_list_weft, one
// workgroup of 1,024 threads per document:
//   1. the document's cut row (1 << site_bits words) into LDS, the found bits
//      cleared;
//   2. one pass over the ids: a node whose id is its site's cut sets the site's
//      found bit;
//   3. a second pass over the ids (the workgroup's own lines, at most 512 KiB
//      a document: whatever of them the caches still hold is not read from
//      HBM again; the resident workgroups of a full device hold more than the
//      L2s do): each wave ballots the keep flags of 64 consecutive nodes into one word
//      of a keep bitmap in LDS; the kind is read only where the cut alone does
//      not keep the node (is it the root?);
//   4. a block scan of the bitmap words' popcounts: the kept count, and a
//      node's kept rank = prefix[word] + popcount(bits below);
//   5. a block scan over the cut row: named and not found, the [id] nodes;
//   6. the document's count (kept + [id]) published at once, its first kept
//      position by a decoupled look-back over the documents (lookback.h; the
//      stage's own words and epochs);
//   7. kept id / cause / kind / source of every kept node (cause and kind are
//      read here, for kept nodes only), the [id] nodes, the kept offsets
//      (device u64[D+1]) and the WEFT word at their final places.
// Nothing is sorted and no node's payload passes through LDS.  LDS: cut row
// 8 KiB, bitmap 8 KiB, prefix 4 KiB, found bits and the waves' totals: 20.2 KiB,
// two workgroups a CU.
//
// General route (a larger document, or list_weft_fused = 0): k_weft_select, a
// workgroup per document: a count pass, a host scan of the counts, a write pass.

constexpr uint32_t LW_NT = 1024;
constexpr uint32_t LW_MAXDOC = 0xFFFFu;  // most nodes of a document (k_weave_doc's and k_list_union's bound)
constexpr uint32_t LW_WORDS = (LW_MAXDOC + 64) / 64;  // bitmap words: 1,024

struct LwIn {
  const uint64_t *id, *cause;
  const uint8_t *kind;
  const uint32_t *off;  // device [D+1]
  const uint64_t *cut;  // device [D << site_bits]
  uint32_t site_shift, site_bits;
};

struct LwOut {
  uint64_t *id, *cause;
  uint8_t *kind;
  uint32_t *src;
  uint64_t *off;   // device [D+1] kept offsets (the fused route)
  uint32_t *weft;  // [D] CW_STATUS_WEFT or 0
};

// (8 waves a SIMD = two workgroups a CU: at most 64 VGPRs)
__global__ __launch_bounds__(LW_NT, 8) void k_list_weft(LwIn in, uint32_t D, unsigned long long *lb,
                                                     uint32_t epoch, LwOut out) {
  constexpr uint32_t NW = LW_NT / 64, U = 4, UW = 2;  // loads in flight: id passes, write pass
  __shared__ uint64_t cutrow[1024];
  __shared__ uint64_t bitmap[LW_WORDS];
  __shared__ uint32_t prefix[LW_WORDS];
  __shared__ uint32_t found[1024 / 32];
  __shared__ uint32_t wtot[NW];
  __shared__ uint32_t s_base;

  const uint32_t d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t b0 = in.off[d], n = in.off[d + 1] - b0;  // (n <= LW_MAXDOC: the host's route)
  const uint32_t S = 1u << in.site_bits, smask = S - 1, shift = in.site_shift;
  const uint64_t *const ids = in.id + b0;
  const uint32_t nwords = (n + 63) >> 6;
  // 1. the cut row (S <= 1,024 = LW_NT words)
  if (tid < S) cutrow[tid] = in.cut[((uint64_t)d << in.site_bits) + tid];
  if (tid < 1024 / 32) found[tid] = 0;
  __syncthreads();

  // 2. which cut ids are nodes
  for (uint32_t i0 = tid; i0 < n; i0 += U * LW_NT) {
    uint64_t x[U];
#pragma unroll
    for (uint32_t u = 0; u < U; u++) {
      const uint32_t i = i0 + u * LW_NT;
      x[u] = i < n ? ids[i] : 0ull;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; u++) {
      if (i0 + u * LW_NT >= n) continue;
      const uint32_t site = (uint32_t)(x[u] >> shift) & smask;
      const uint64_t cw = cutrow[site];
      if (cw != 0 && x[u] == cw) atomicOr(&found[site >> 5], 1u << (site & 31));  // (no returned value)
    }
  }
  __syncthreads();

  // 3. the keep bitmap: wave w takes the words w, w + NW, ...
  for (uint32_t w0 = w; w0 < nwords; w0 += U * NW) {
    uint64_t x[U];
#pragma unroll
    for (uint32_t u = 0; u < U; u++) {
      const uint32_t i = ((w0 + u * NW) << 6) + lane;
      x[u] = i < n ? ids[i] : 0ull;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; u++) {
      const uint32_t word = w0 + u * NW, i = (word << 6) + lane;
      bool keep = false;
      if (i < n) {
        const uint32_t site = (uint32_t)(x[u] >> shift) & smask;
        const uint64_t cw = cutrow[site];
        const bool hit = (found[site >> 5] >> (site & 31)) & 1u;
        keep = cw != 0 && (!hit || x[u] <= cw);
        if (!keep) keep = (in.kind[b0 + i] & KIND_ROOT) != 0;
      }
      const uint64_t m = __ballot(keep);
      if (lane == 0 && word < nwords) bitmap[word] = m;
    }
  }
  __syncthreads();

  // 4. kept nodes before each bitmap word; 5. the [id] nodes before each slot
  uint32_t totK, totM;
  const uint32_t pc = tid < nwords ? (uint32_t)__popcll(bitmap[tid]) : 0u;
  prefix[tid] = block_exscan<LW_NT>(pc, wtot, &totK);
  const bool miss = tid < S && cutrow[tid] != 0 && !((found[tid >> 5] >> (tid & 31)) & 1u);
  const uint32_t mpos = block_exscan<LW_NT>(miss ? 1u : 0u, wtot, &totM);

  // 6. publish this document's count, then sum the predecessors' (one wave)
  const uint32_t tot = totK + totM;
  if (tid == 0) lb_publish(lb, d, epoch, tot);
  if (tid < 64) {
    const uint32_t b = lb_exclusive(lb, d, epoch, tot);
    if (tid == 0) s_base = b;
  }
  __syncthreads();  // (prefix[] is complete here as well)
  const uint32_t base = s_base;

  // 7. outputs at their final places (i & 63 == lane: LW_NT is a multiple of 64)
  const uint64_t below = (1ull << lane) - 1;
  for (uint32_t i0 = tid; i0 < n; i0 += UW * LW_NT) {
    bool kp[UW];
    uint32_t o[UW];
    uint64_t kid[UW], kca[UW];
    uint8_t kk[UW];
#pragma unroll
    for (uint32_t u = 0; u < UW; u++) {
      const uint32_t i = i0 + u * LW_NT;
      kp[u] = false;
      o[u] = 0;
      kid[u] = kca[u] = 0;
      kk[u] = 0;
      if (i < n) {
        const uint64_t bits = bitmap[i >> 6];
        kp[u] = (bits >> lane) & 1ull;
        o[u] = base + prefix[i >> 6] + (uint32_t)__popcll(bits & below);
      }
      if (kp[u]) {
        kid[u] = ids[i];
        kca[u] = in.cause[b0 + i];
        kk[u] = in.kind[b0 + i];
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < UW; u++) {
      if (!kp[u]) continue;
      out.id[o[u]] = kid[u];
      out.cause[o[u]] = kca[u];
      out.kind[o[u]] = kk[u];
      out.src[o[u]] = i0 + u * LW_NT;
    }
  }
  if (miss) {  // the [id] nodes, by site rank, after the kept nodes
    const uint32_t o = base + totK + mpos;
    out.id[o] = cutrow[tid];
    out.cause[o] = CW_NIL;
    out.kind[o] = 0;
    out.src[o] = 0xFFFFFFFFu;
  }
  if (tid == 0) {
    out.off[d] = base;
    if (d == D - 1) out.off[D] = (uint64_t)base + tot;
    out.weft[d] = totM ? (uint32_t)CW_STATUS_WEFT : 0u;
  }
}

namespace {

struct LwHost {  // what weft_lists_impl hands the select stage (device pointers)
  uint64_t D, N;
  LwIn in;    // (off: w_off, uploaded by list_weft_layout)
  LwOut out;  // (off filled in by the fused route)
};

// The document layout on the device (u32[D+1]) and whether every document fits
// the fused kernel, cached in the context while doc_offsets repeats.  `largest`:
// the largest document (check_doc_offsets).
int list_weft_layout(cw_ctx *c, const uint64_t *off, uint64_t D, uint64_t largest, const uint32_t **doff) {
  const char *name = "w_off";
  bool miss;
  if (device_layout(c, c->lweft, D, off, nullptr, &name, nullptr, doff, &miss)) return -1;
  if (miss) c->lweft.fits = largest <= LW_MAXDOC;
  return 0;
}

// The fused route.  Returns 1 when it does not apply (the caller takes the
// general route), 0 on success with the kept offsets in `ko` (host), -1 on
// error.
int list_weft_fused(cw_ctx *c, LwHost &h, uint64_t *ko) {
  auto &lw = c->lweft;
  const uint64_t D = h.D;
  if (!lw.fits) return 1;
  uint64_t *dko = scratch_t<uint64_t>(c, "lw_koff", D + 1);
  if (!dko) return fail(c, "out of device memory (list weft)");
  uint32_t epoch;
  unsigned long long *lb = lookback_words(c, lw.lb, "lw_lb", (uint32_t)D, 1, &epoch);
  if (!lb) return -1;
  h.out.off = dko;
  size_t rec = NO_REC;
  {
    // per input node its id once (the later reads are the workgroup's own
    // lines) and its bit of the bitmap, per cut slot 8 B, per document its
    // two offsets, its kept offset and the WEFT word; 9 B in and 21 B out per
    // kept node and the kind byte of every other node join once the count is
    // known
    Launch L(c, "list_weft", (double)h.N * 8.125 + (double)(D << h.in.site_bits) * 8 + (double)D * 20, nullptr,
             &rec);
    hipLaunchKernelGGL(k_list_weft, dim3((uint32_t)D), dim3(LW_NT), 0, c->stream, h.in, (uint32_t)D, lb,
                       epoch, h.out);
  }
  if (check_launch(c, "list_weft")) return -1;
  // the stage's one device-to-host copy: they are the weave's doc_offsets
  HIPCHK(c, hipMemcpyAsync(ko, dko, (D + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (rec < c->pending.size())
    c->pending[rec].bytes += (double)ko[D] * 30 + (double)(h.N - std::min(h.N, ko[D]));
  return 0;
}

// The general route: count pass, host scan, write pass.
int list_weft_general(cw_ctx *c, LwHost &h, uint64_t *ko) {
  const uint64_t D = h.D;
  const uint32_t sb = h.in.site_bits;
  uint32_t *kcnt = scratch_t<uint32_t>(c, "w_kcnt", D + 1), *koff = scratch_t<uint32_t>(c, "w_koff", D + 1);
  if (!kcnt || !koff) return fail(c, "out of device memory (weft)");
  auto select = [&](const char *stat, int pass, double bytes) {
    {
      Launch L(c, stat, bytes);
      hipLaunchKernelGGL((k_weft_select<1024>), dim3((uint32_t)D), dim3(1024), 0, c->stream, h.in.id,
                         h.in.cause, h.in.kind, h.in.off, h.in.cut, h.in.site_shift, sb, pass, kcnt, koff,
                         h.out.id, h.out.cause, h.out.kind, h.out.src, h.out.weft);
    }
    return check_launch(c, stat);
  };
  // ids twice, a cut word three times and the kind per node; the cut slots once
  if (select("weft_count", 0, (double)h.N * 41 + (double)(D << sb) * 8 + (double)D * 16)) return -1;
  if (scan_counts(c, kcnt, D, ko, koff)) return -1;
  return select("weft_write", 1,
                (double)h.N * 41 + (double)(D << sb) * 8 + (double)D * 12 + (double)ko[D] * 30);
}

}  // namespace
