/*
 * causeweave_insert.h -- the incremental half of the list weave: c.list/weave's
 * 2/3-arity (list.cljc:29-34) over s/weave-node (shared.cljc:225-241), behind
 * s/insert (shared.cljc:151-184).  One transaction per document, any number of
 * documents per call, without a reweave.  The conventions are causeweave.h's.
 *
 * weave-node is data-parallel.  With nm the first tx node and nr = weave[i]:
 *
 *   later(i) = [special(nr) && id(nm) != cause(nr) && (!special(nm) || nm << nr)]
 *           || [nm << nr && (!special(nm) || special(nr))]
 *   asap(i)  = id(weave[i-1]) == cause(nm) || id(nm) == cause(weave[i])
 *              (weave[-1] is nil; i = n has no nr, only the first term)
 *   a = min{ i in 0..n : asap(i) }
 *   p = min{ i >= a, i < n : !later(i) }, or n when there is none or no a
 *   new weave = weave[0,p) ++ [node] ++ more ++ weave[p,n)
 *
 * (weave-later?'s second clause is its third with one more conjunct, so it and
 * seen-since-asap never change the result.)  The call is two min-reductions
 * over the weave and a splice: no sort, no tree, no list ranking.
 */
#ifndef CAUSEWEAVE_INSERT_H
#define CAUSEWEAVE_INSERT_H

#include "causeweave.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  cw_list_batch docs;           /* the woven documents (doc_offsets: HOST); ts_shift / site_shift /
                                   site_bits as in cw_weave_lists; key_bits unused                   */
  const uint32_t *weave_perm;   /* [N] their weave, as cw_list_result.weave_perm                     */
  const uint32_t *visible_bits; /* [(N+31)/32]                                                       */
  const uint32_t *yarn_perm;    /* [N], or NULL (then result->weave.yarn_perm must be NULL)          */
  const uint64_t *doc_value;    /* [N] value tokens, or NULL                                         */
  const uint64_t *tx_offsets;   /* HOST [n_docs+1]: document d receives tx nodes
                                   [tx_offsets[d], tx_offsets[d+1]): `node`, then `more` in order;
                                   an empty range leaves the document as it is                       */
  const uint64_t *tx_id;        /* [T]                                                               */
  const uint64_t *tx_cause;     /* [T]                                                               */
  const uint8_t *tx_kind;       /* [T] CW_KIND_* (never ROOT)                                        */
  const uint64_t *tx_value;     /* [T] or NULL, together with doc_value                              */
} cw_insert_batch;

typedef struct {
  uint64_t *new_offsets;   /* HOST [n_docs+1]: document d of the result                               */
  uint32_t *insert_pos;    /* [n_docs] doc-local weave position p the tx went to; UINT32_MAX when
                              nothing was inserted.  May be NULL                                      */
  cw_list_result weave;    /* laid out by new_offsets. weave_perm / yarn_perm hold doc-local indices:
                              s < n_d is the old input index s, s >= n_d is tx node s - n_d
                              (cw_merge_result's convention). status: this call's bits only           */
  /* [N+T] each, or NULL: the columns of the result as a cw_list_batch (old nodes in input
     order, then the tx), ready for the next cw_insert_lists / cw_render_lists /
     cw_weft_lists_dev / cw_merge_lists.  id_key, cause_key, kind: all three or none.
     value: only with them and with doc_value */
  uint64_t *id_key;
  uint64_t *cause_key;
  uint8_t *kind;
  uint64_t *value;
} cw_insert_result;

/* Per document, as s/insert and c.list/weave do it:
 *   - the tx is empty: copied unchanged, status 0, insert_pos UINT32_MAX;
 *   - the first tx node's id is a node with the same body (cause, kind, and value
 *     token when values are given): copied unchanged, status 0, insert_pos
 *     UINT32_MAX -- the whole tx is skipped (shared.cljc:166-168);
 *   - the first tx node's id is a node with another body: CW_STATUS_DUP, copied
 *     unchanged (:169-171);
 *   - the first tx node's cause is no id of the document (CW_NIL is one such
 *     cause): CW_STATUS_ORPHAN, copied unchanged (:175-178);
 *   - anything else: all k tx nodes are spliced at p by the formula above,
 *     literally.  That is the reference's result for a document outside the
 *     weave's domain (orphans, non-Lamport causes) as well: s/insert does not
 *     refold such a document, it runs weave-node on the weave as it stands.
 * Only the first tx node is validated, as in the reference.  A later tx node
 * whose id is already present, ids repeated inside a tx and tx nodes of
 * different transactions are caller errors: the document then comes out
 * well-formed but unspecified, and nothing is read or written outside the
 * caller's arrays.  The same holds for a weave_perm that is no permutation of
 * the document (a CW_STATUS_DUP / INTERNAL result of an earlier call).
 *
 * Outputs:
 *   visible_bits   unchanged positions carried over, shifted; positions
 *                  p-1 .. p+k-1 recomputed by hide? (list.cljc:48-55), the last tx
 *                  node looking at the old weave[p];
 *   visible_count  the popcount of the new document;
 *   max_ts         the largest id's ts in the new document (refresh-ts); may be NULL;
 *   yarn_perm      cw_list_result's definition for the new document: the old yarn
 *                  entries keep their order and the tx nodes go to their places
 *                  among them.  It requires the tx ids to ascend strictly (the
 *                  caller's duty; this output's only extra precondition);
 *   new_offsets    new_offsets[d+1] - new_offsets[d] = n_d + k_d for an accepted
 *                  tx and n_d otherwise: refused and empty documents compact the
 *                  layout.  Computed on the device and read back once.
 *
 * memspace: where every array lives except doc_offsets, tx_offsets and
 * new_offsets (host memory).  A host call stages through the context's
 * scratch.  Under cw_ctx_set_async the call waits once for the new offsets and
 * for nothing else; when doc_offsets or tx_offsets differ from the previous
 * call's they are also uploaded with blocking copies.
 * Limits: N + T < 2^32 - 1; a document below 2^29 - 1 nodes with its tx.
 * Four kernels serve every document size (listinsert.hip): tiles of 8,192
 * nodes mark them in input order, tiles of 8,192 weave positions find the
 * places, a wave a document plans the new layout, tiles of 8,192 new positions
 * write it.
 * Errors (< 0, cw_last_error, nothing written): null batch / result / offsets
 * array; offsets that do not start at 0 or decrease; with N > 0 a null
 * weave_perm, visible_bits or node column; with T > 0 a null tx column;
 * doc_value and tx_value not both set or both null; weave.yarn_perm without
 * yarn_perm or with site_bits = 0; a partial set of output columns, or value
 * without doc_value; a null weave_perm, visible_bits, visible_count or status
 * output; a bad memspace.
 * A tx of several nodes goes in as one block, as in the reference: where its
 * later nodes hang under a special node of the same tx the full reweave orders
 * them differently (it defers them behind that node's other children). */
int cw_insert_lists(cw_ctx *ctx, const cw_insert_batch *batch, cw_insert_result *result, int memspace);

#ifdef __cplusplus
}
#endif
#endif /* CAUSEWEAVE_INSERT_H */
