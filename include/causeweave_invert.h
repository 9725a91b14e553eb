/*
 * causeweave_invert.h -- invert- (base/core.cljc:313-343), what CausalBase's undo-
 * (:375-390), redo- (:392-409) and reset- (:345-352) end in: a slice of a base's
 * history becomes the transaction of h.hide / h.show nodes that takes it back.
 * The call makes the nodes; cw_insert_lists / cw_insert_maps / cw_merge_* apply
 * them.  The conventions are causeweave.h's.
 *
 * A batch holds BASES.  Base g is the documents [base_offsets[g],
 * base_offsets[g+1]); a document is one collection of the base, a list or a map,
 * and every document shares one key layout.  Per base, with H the slice:
 *
 *   1. selected    a node whose id lies in [sel_lo[g], sel_hi[g]] (inclusive;
 *                  sel_lo > sel_hi selects nothing) and whose site rank
 *                  ((id >> site_shift) & (2^site_bits - 1)) has its bit set in
 *                  the base's sel_sites mask.  In packed keys subhis (:288-311)
 *                  is such a range: one tx-id is [ts site 0] .. [ts site 2^site_shift - 1].
 *                  A list's root (CW_KIND_ROOT) is never selected.
 *   2. hidden      the documents that the ref_doc of any selected node names
 *                  (:329-332; direct references only, from every selected node,
 *                  those of hidden documents included).  A ref_doc outside the
 *                  node's own base, or >= n_docs, is ignored.  The selected nodes
 *                  of a hidden document make no parts (:335).
 *   3. inverted    a remaining node [id cause kind] becomes (invert-path, :313-320)
 *                    hide, h.hide   -> [cause  h.show]   (cause_is_id as the node's)
 *                    h.show         -> [cause  h.hide]
 *                    anything else  -> [id     h.hide]   (cause_is_id 1)
 *   4. one part    per (document, cause_is_id, cause) (:338-342); a key token and
 *                  a packed id of the same numeric value are different keys; with
 *                  cause_is_id 2 (the nil key) the cause word is ignored and the
 *                  part's inv_cause is 0.  The part that stays is the one made
 *                  from the OLDEST selected node of the key (the reference
 *                  assoc'es newest first).
 *   5. tx-index    the rank of the part among ALL parts of the base (a keyword
 *                  value makes one node, :232-252) by descending id of the
 *                  NEWEST selected node of its key.  Ids are unique across a
 *                  base, so there are no ties.  For up to 8 parts this is the
 *                  reference's order (an array map keeps a key where it first
 *                  appeared); beyond 8 the reference's map is a hash map, its
 *                  order unspecified, and this is the library's choice.  Every
 *                  order gives the same weave: after step 4 no two parts of a
 *                  collection share a cause, so none are siblings.
 *                  inv_id = new_tx[g] + tx-index.
 *
 * A base with more than 2^site_shift parts does not fit the tx field:
 * CW_STATUS_KEY_RANGE on every document of the base, and no parts for it.
 * CW_STATUS_DUP / CW_STATUS_ORPHAN belong to the insert or merge that follows;
 * cw_invert sets neither.
 */
#ifndef CAUSEWEAVE_INVERT_H
#define CAUSEWEAVE_INVERT_H

#include "causeweave.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint64_t n_docs;
  const uint64_t *doc_offsets;   /* HOST [n_docs+1] */
  const uint64_t *id_key;        /* [N] */
  const uint64_t *cause;         /* [N] packed id, key token, or unused (nil key) */
  const uint8_t  *kind;          /* [N] */
  const uint8_t  *cause_is_id;   /* [N] as cw_map_batch (0 key token, 1 id, 2 nil key), or NULL: every cause is an id (lists only) */
  const uint32_t *ref_doc;       /* [N] or NULL: the batch-wide document this node's value refers to, UINT32_MAX = none */
  uint32_t ts_shift;
  uint32_t site_shift;
  uint32_t site_bits;            /* 1..10 */
  uint32_t reserved;             /* 0 */
  uint64_t n_bases;
  const uint64_t *base_offsets;  /* HOST [n_bases+1], over documents; base_offsets[n_bases] = n_docs */
  const uint64_t *sel_lo;        /* [n_bases] */
  const uint64_t *sel_hi;        /* [n_bases] */
  const uint64_t *sel_sites;     /* [n_bases * W], W = (2^site_bits + 63) / 64 words a base: bit r = site rank r */
  const uint64_t *new_tx;        /* [n_bases] the packed id [lamport-ts, local site, 0] of the inverting tx */
} cw_invert_batch;

typedef struct {
  uint64_t *part_offsets;        /* HOST [n_docs+1]: the parts of document d, ascending tx-index */
  uint64_t *inv_id;              /* [N] (sized for N; part_offsets[n_docs] entries written) */
  uint64_t *inv_cause;           /* [N] */
  uint8_t  *inv_cause_is_id;     /* [N]; NULL exactly when the input column is NULL */
  uint8_t  *inv_kind;            /* [N] CW h.hide (2) or h.show (3) */
  uint32_t *inv_src;             /* [N] or NULL: the doc-local input index of the oldest selected node of the part's key */
  uint32_t *base_parts;          /* [n_bases] or NULL: the parts of each base (how far its tx-index ran; 0 after KEY_RANGE) */
  uint32_t *status;              /* [n_docs] 0 or CW_STATUS_KEY_RANGE */
} cw_invert_result;

/* The parts of document d, inv_*[part_offsets[d] .. part_offsets[d+1]), are one
 * side of a cw_list_batch / cw_map_batch of their own with part_offsets as its
 * offsets: side b of cw_merge_lists / cw_merge_maps, or the tx of
 * cw_insert_lists / cw_insert_maps.
 *
 * memspace: where every array lives except doc_offsets, base_offsets and
 * part_offsets (host memory).  A host call stages through the context's
 * scratch.  Under cw_ctx_set_async the call waits once, for the part offsets,
 * and for nothing else; when doc_offsets or base_offsets differ from the
 * previous call's they are also uploaded with blocking copies.  A call that
 * takes the general route (below) waits a second time, for the size of its sort.
 *
 * Routes.  The selected nodes of the documents that are not hidden are
 * compacted in input order (two passes over fixed tiles of node positions).  A
 * base with at most invert_cap of them (context option, default 4,096, range
 * 1..4,096) is finished by one wave (up to 256) or one workgroup in LDS.  One
 * base above invert_cap sends the whole call through the general route: the
 * library's stable key sort over every base at once.  Both give the same arrays.
 *
 * Limits: N < 2^32 - 1, n_docs and n_bases < 2^32 - 1.
 * Errors (< 0, cw_last_error, nothing written): null batch / result; null
 * doc_offsets, base_offsets, part_offsets or status; with N > 0 a null id_key,
 * cause, kind, inv_id, inv_cause or inv_kind; with n_bases > 0 a null sel_lo,
 * sel_hi, sel_sites or new_tx; inv_cause_is_id set without cause_is_id or the
 * reverse; offsets that do not start at 0 or that decrease;
 * base_offsets[n_bases] != n_docs; site_bits outside 1..10; site_shift or
 * ts_shift above 63; N >= 2^32 - 1; a bad memspace. */
int cw_invert(cw_ctx *ctx, const cw_invert_batch *batch, cw_invert_result *result, int memspace);

#ifdef __cplusplus
}
#endif
#endif /* CAUSEWEAVE_INVERT_H */
