/*
 * causeweave_map_insert.h -- the incremental half of the map weave: c.map/weave's
 * 2/3-arity (map.cljc:29-45) over s/weave-node (shared.cljc:225-241), behind
 * s/insert (shared.cljc:151-184): what assoc, dissoc, transact and undo end in.
 * One transaction per collection, any number of collections per call, without
 * a reweave.  The conventions are causeweave.h's; the formula is
 * causeweave_insert.h's, run on one key weave per tx node.
 *
 * c.map/weave weaves the tx nodes one at a time (map.cljc:43-44 recurses with
 * `more` as single nodes; the list splices them as a block).  Tx node j, in order:
 *
 *   key word        a key cause: its token; a nil cause: CW_NIL; an id cause: looked
 *                   up among the old nodes and every tx node of the collection
 *                   (s/insert has assoc'ed the whole tx before the weave, :179-183):
 *                   that node's token, or CW_MAP_ID_KEY | its cause id, or CW_NIL
 *                   when its cause is nil or when the cause names no node (the root
 *                   id 0 names none) (map.cljc:30-34)
 *   cause-in-weave  the id for an id cause, else the root id 0 (map.cljc:35-37)
 *   key weave       the collection's key weave with that seg_key, or a new one,
 *                   [root], at its place in ascending seg_key order
 *   place           with nm = [id cause-in-weave kind] and the key weave as it
 *                   stands after tx nodes 0 .. j-1 (causeweave_insert.h):
 *                     a = min{ i : id(weave[i-1]) == cause(nm) || id(nm) == cause(weave[i]) }
 *                     p = min{ i >= a, i < n : !later(i) }, or n when there is none
 *                         or no a -- in maps a node whose cause lies in another
 *                         key weave has no a and is appended
 *                   weave[i]'s cause is its cause-in-weave; the root is [0 nil].
 *
 * The kernel (mapinsert.hip) keeps no interim weave: a tx node's place is (key
 * weave, gap in the old key weave, rank among the tx nodes of that gap), step j
 * is three min-reductions over the old key weave and the j earlier tx nodes.
 * Cost per collection: O((n_d + touched key-weave length) * k_d / G) with G = 64
 * lanes (every collection has n_d + k_d <= 2,048) or 256; a bulk load of
 * thousands of nodes into one map is cw_merge_maps' job.
 */
#ifndef CAUSEWEAVE_MAP_INSERT_H
#define CAUSEWEAVE_MAP_INSERT_H

#include "causeweave.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  cw_map_batch colls;            /* the woven collections (coll_offsets: HOST); key_bits / token_bits unused */
  uint64_t n_segs;               /* their cw_map_result as it stands: */
  const uint64_t *seg_offsets;   /* [n_segs+1] */
  const uint32_t *seg_coll;      /* [n_segs] */
  const uint64_t *seg_key;       /* [n_segs] */
  const int64_t  *seg_active;    /* [n_segs] */
  const uint32_t *seg_perm;      /* [N + n_segs] */
  const uint64_t *coll_value;    /* [N] value tokens, or NULL */
  const uint64_t *tx_offsets;    /* HOST [n_colls+1]: collection d receives tx nodes [tx_offsets[d], tx_offsets[d+1]) in order */
  const uint64_t *tx_id;         /* [T] */
  const uint64_t *tx_cause;      /* [T] */
  const uint8_t  *tx_cause_is_id; /* [T] as cw_map_batch */
  const uint8_t  *tx_kind;       /* [T] */
  const uint64_t *tx_value;      /* [T] or NULL, together with coll_value */
} cw_map_insert_batch;

typedef struct {
  uint64_t *new_offsets;  /* HOST [n_colls+1] */
  uint32_t *tx_seg;       /* [T] or NULL: the key weave (index into maps.seg_*) tx node t went to; UINT32_MAX = not inserted */
  uint32_t *tx_pos;       /* [T] or NULL: its position in that key weave (root = 0) in the result */
  cw_map_result maps;     /* cap_segs IN (>= n_segs + T), n_segs OUT; laid out by new_offsets; every index collection-local:
                             s < n_d is the old input index s, s >= n_d is tx node s - n_d; status: this call's bits only */
  uint64_t *id_key;
  uint64_t *cause;
  uint8_t *cause_is_id;
  uint8_t *kind;
  uint64_t *value;
                          /* [N+T] or NULL: the result's columns (old nodes in input order, then the accepted tx), ready for
                             the next cw_insert_maps / cw_render_maps / cw_weft_maps / cw_merge_maps.
                             The four node columns are all set or all null; value only with them and with coll_value */
} cw_map_insert_result;

/* Per collection, as s/insert and c.map/weave do it, in this order:
 *   - the tx is empty: copied unchanged, status 0;
 *   - the first tx node's id is a node with the same body (cause_is_id, cause
 *     unless nil, kind, and value token when values are given): the whole tx is
 *     skipped, copied unchanged, status 0 (shared.cljc:166-168);
 *   - ... with another body: CW_STATUS_DUP, copied unchanged (:169-171);
 *   - the first tx node's cause is an id (cause_is_id = 1) that names no node of
 *     the collection -- the root id 0 names none -- or is nil (cause_is_id = 2):
 *     CW_STATUS_ORPHAN, copied unchanged (:175-178).  The check runs before the
 *     tx joins ::nodes, so a first node caused by a later node of its own tx is
 *     refused too.  A key cause is exempt (:175), the first assoc into an empty
 *     collection (n_d = 0, no key weaves) included;
 *   - a tx node's key token is >= 2^62 (it would collide with CW_MAP_ID_KEY /
 *     CW_NIL): CW_STATUS_MAP_KEY, copied unchanged;
 *   - anything else: every tx node is woven as above.
 * Only the first tx node is validated, as in the reference.  A later tx node
 * whose id is already present, ids repeated inside a tx, and seg arrays that
 * are not a cw_map_result of `colls` are caller errors: the collection then
 * comes out well-formed but unspecified, and nothing is read or written outside
 * the caller's arrays (every index taken from seg_perm, seg_coll and seg_offsets
 * is checked against its bound).
 *
 * Outputs:
 *   maps.seg_*     the key weaves of the result, per collection in ascending
 *                  seg_key order; seg_perm: the root (UINT32_MAX), then indices;
 *   seg_active     of every key weave a tx node went to: active-node
 *                  (map.cljc:47-59) with its quirks -- blank (-1) when the node
 *                  after the root is a hide or h.hide, and a node is passed over
 *                  when ANY hide or h.hide follows it, whichever node that names;
 *                  an untouched key weave keeps its word;
 *   tx_seg/tx_pos  UINT32_MAX for every tx node of a collection copied unchanged;
 *   new_offsets    new_offsets[d+1] - new_offsets[d] = n_d + k_d for an accepted
 *                  tx and n_d otherwise.  Computed on the device and read back
 *                  once, with maps.n_segs.
 *
 * memspace: where every array lives except coll_offsets, tx_offsets and
 * new_offsets (host memory).  A host call stages through the context's
 * scratch.  Under cw_ctx_set_async the call waits once, for the new offsets
 * and n_segs, and for nothing else; when coll_offsets or tx_offsets differ
 * from the previous call's they are also uploaded with blocking copies.
 * Limits: N + T < 2^32 - 1; n_segs + T < 2^32 - 1; maps.cap_segs >= n_segs + T.
 * Context option map_insert_wave (default 1): a wave per collection when every
 * collection has n_d + k_d <= 2,048; 0, or one larger collection: a workgroup
 * per collection for the whole call.  Both give the same arrays.
 * Errors (< 0, cw_last_error, nothing written): null batch / result / offsets
 * array; offsets that do not start at 0 or decrease; with N > 0 or n_segs > 0 a
 * null node column or seg array; with T > 0 a null tx column; coll_value and
 * tx_value not both set or both null; a partial set of output columns, or
 * value without coll_value; a null seg array or status of `maps`; cap_segs
 * below n_segs + T; a bad memspace.
 * Unspecified: the result where insert's arrival-order result is not a
 * function of the inputs above (the caller errors named); the order of the tx
 * nodes is the caller's and is woven as given (non-Lamport arrival included). */
int cw_insert_maps(cw_ctx *ctx, const cw_map_insert_batch *batch, cw_map_insert_result *result, int memspace);

#ifdef __cplusplus
}
#endif
#endif /* CAUSEWEAVE_MAP_INSERT_H */
