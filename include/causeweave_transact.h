/*
 * causeweave_transact.h -- transact- (base/core.cljc:100-252), the write side of
 * CausalBase, for a batch of bases: the nested values of a transaction, given
 * as one depth-first token stream per base, become the nodes of the base's
 * collections -- the tx-index assigned, a collection allocated per nested list
 * or map, a list's nodes chained cause to cause, a string spliced into its list
 * one character at a time.  The inverse of cw_render_bases, which takes
 * collections and writes the stream.  The call makes the nodes; cw_insert_lists
 * / cw_insert_maps / cw_weave_* apply them.  The conventions are causeweave.h's.
 *
 * Base g owns the existing documents [base_doc_offsets[g], base_doc_offsets[g+1])
 * and the tokens [tok_offsets[g], tok_offsets[g+1]).  Its stream is a sequence
 * of PARTS: CW_TX_PART (a tx-part into the existing document tok_arg) or
 * CW_TX_ROOT_LIST / CW_TX_ROOT_MAP (a tx-part without a uuid: a new root
 * collection, :203-208), then the contents, then CW_TX_CLOSE.  Contents are
 * CW_TX_LEAF, CW_TX_STR (tok_arg characters) or CW_TX_OPEN_LIST / CW_TX_OPEN_MAP
 * ... CW_TX_CLOSE, nested to any depth.  A GROUP is a part or an OPEN_*; it is
 * a list or a map: doc_is_map of the target for a PART, the token's own kind
 * otherwise.
 *
 *   1. collections  every ROOT_* and OPEN_* token makes one, numbered within the
 *                   base in the order of these tokens (the order in which
 *                   add-collection-of-this-values-type-to-cb draws uuids); new
 *                   collection c of the batch is document n_docs + c.
 *   2. nodes        LEAF: 1.  STR directly in a map group: 1 (preserve-strings?,
 *                   :134); directly in a list group: tok_arg, 0 included
 *                   (:145-151).  The CLOSE of an OPEN_*: 1, the ref node in the
 *                   group that encloses the OPEN, made after the nested nodes
 *                   (:158-164).  Everything else: 0.
 *   3. tx-index     of a token's first node: the exclusive prefix sum of these
 *                   counts in token order within the base; id = new_tx[g] +
 *                   tx-index.
 *   4. document     a node goes into the document of the group that directly
 *                   encloses the token that makes it (a ref node: the group that
 *                   encloses the OPEN_*).
 *   5. map group    the cause is tok_cause / tok_cause_is_id of the making token,
 *                   as in cw_map_batch; for a ref node those of the OPEN_* token.
 *   6. list group   cause_is_id 1; the cause is the id of the last node that an
 *                   earlier direct child of the group made, else the group's
 *                   initial cause: tok_cause of a PART / ROOT_LIST as it is (0
 *                   for the root id, CW_NIL for nil), 0 for an OPEN_LIST.  The
 *                   characters of a STR chain one after the other; a child that
 *                   makes no node passes the chain through.
 *   7. kind         tok_vkind of a LEAF; CW_KIND_NORMAL for characters and refs.
 *                   A new list begins with its root node (id 0, cause CW_NIL,
 *                   CW_KIND_ROOT), which takes no tx-index.
 *
 * The causes are passed through as given: what s/insert refuses (a scalar into
 * a list with a nil cause) is refused by the insert that follows.
 *
 * base_status[g]: CW_STATUS_TX_MALFORMED -- a CLOSE with no open group, a group
 * still open at the end of the base, a PART / ROOT_* inside a group, a LEAF, STR
 * or OPEN_* outside any group, a PART target outside the base's own documents,
 * a tok_kind out of range.  CW_STATUS_KEY_RANGE -- the base's nodes with a
 * tx-index (roots apart) number more than 2^site_shift.  A flagged base makes no
 * collections and no nodes, and does not disturb its neighbours.
 */
#ifndef CAUSEWEAVE_TRANSACT_H
#define CAUSEWEAVE_TRANSACT_H

#include "causeweave.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { CW_STATUS_TX_MALFORMED = 1u << 10 }; /* base_status: the token stream of the base is not a sequence of parts */

enum {
  CW_TX_LEAF = 0,
  CW_TX_STR = 1,
  CW_TX_OPEN_LIST = 2,
  CW_TX_OPEN_MAP = 3,
  CW_TX_CLOSE = 4,
  CW_TX_PART = 5,
  CW_TX_ROOT_LIST = 6,
  CW_TX_ROOT_MAP = 7
};

typedef struct {
  uint64_t n_docs;                  /* the existing collections of all bases */
  const uint64_t *base_doc_offsets; /* HOST [n_bases+1], over documents; base_doc_offsets[n_bases] = n_docs */
  const uint8_t  *doc_is_map;       /* [n_docs] */
  uint32_t ts_shift;
  uint32_t site_shift;
  uint32_t site_bits;               /* 1..10 */
  uint32_t reserved;                /* 0 */
  uint64_t n_bases;
  const uint64_t *new_tx;           /* [n_bases] the packed id [lamport-ts, local site, 0] of the transaction */
  const uint64_t *tok_offsets;      /* HOST [n_bases+1]; T = tok_offsets[n_bases] */
  const uint8_t  *tok_kind;         /* [T] CW_TX_* */
  const uint32_t *tok_arg;          /* [T] PART: the batch-wide target document; STR: its characters */
  const uint64_t *tok_cause;        /* [T] */
  const uint8_t  *tok_cause_is_id;  /* [T] as cw_map_batch (0 key token, 1 id, 2 nil key) */
  const uint8_t  *tok_vkind;        /* [T] or NULL: a LEAF's CW_KIND_* (never ROOT); NULL: every LEAF is normal */
} cw_transact_batch;

typedef struct {
  uint64_t new_cap;                 /* the new_* arrays hold this many collections */
  uint64_t node_cap;                /* the node_* arrays hold this many nodes */
  uint64_t *base_new_offsets;       /* HOST [n_bases+1]: the new collections of base g; C = base_new_offsets[n_bases] */
  uint64_t *base_node_offsets;      /* HOST [n_bases+1]: the nodes of base g counted, roots included; M = base_node_offsets[n_bases] */
  uint64_t *node_offsets;           /* HOST [n_docs + min(new_cap, T) + 1], all written: the nodes of document d; the entries past n_docs + C repeat M */
  uint64_t *node_id;                /* [node_cap]; M written */
  uint64_t *node_cause;             /* [node_cap] */
  uint8_t  *node_cause_is_id;       /* [node_cap] */
  uint8_t  *node_kind;              /* [node_cap] CW_KIND_* */
  uint32_t *node_src;               /* [node_cap] the batch-wide token that made the node; a root: the opening token */
  uint32_t *node_sub;               /* [node_cap] the character's index within its STR, else 0 */
  uint32_t *node_ref;               /* [node_cap] a ref node: the batch-wide document of the new collection it names, else UINT32_MAX */
  uint8_t  *node_run;               /* [node_cap] 1 on the first node of each insert of the reference (:107-115): the first node of a group */
  uint8_t  *new_is_map;             /* [new_cap]; C written */
  uint32_t *new_open;               /* [new_cap] the token that opens the collection */
  uint32_t *root_doc;               /* [n_bases] the document of the base's last ROOT_*, or UINT32_MAX */
  uint32_t *base_status;            /* [n_bases] 0, CW_STATUS_TX_MALFORMED or CW_STATUS_KEY_RANGE */
} cw_transact_result;

/* Nodes are grouped by document, existing documents first, then the new
 * collections; within a document they are in tx-index order, a new list's root
 * first.  The nodes of document d, node_*[node_offsets[d] .. node_offsets[d+1]),
 * are one side of a cw_list_batch / cw_map_batch with node_offsets as its
 * offsets: for an existing document the tx of cw_insert_lists / cw_insert_maps
 * (one run, node_run, a call), for a new collection a document of cw_weave_*.
 * node_ref is the ref_doc column of cw_invert and the value column that
 * cw_render_lists / cw_render_maps take for cw_render_bases.
 *
 * memspace: where every array lives except base_doc_offsets, tok_offsets,
 * base_new_offsets, base_node_offsets and node_offsets (host memory).  A host
 * call stages through the context's scratch.  Under cw_ctx_set_async the call
 * waits once, for the three offset arrays, and for nothing else; when
 * base_doc_offsets or tok_offsets differ from the previous call's they are also
 * uploaded with blocking copies.
 *
 * The ten node_* and new_* arrays may all be NULL: the count-only call (the
 * three offset arrays, base_status, root_doc).  In a count-only call new_cap
 * only sizes node_offsets: with C > new_cap its n_docs + new_cap + 1 entries
 * are the offsets of the first new_cap collections and the call succeeds (T is
 * always enough).  Exactly M and C elements of the node_* and new_* arrays are
 * written, nothing past them.
 *
 * Path and routes.  The tokens take their depth from a scan and are sorted,
 * stably, by (base, depth, target of their part), which lays the direct
 * children of every group side by side; every node is then written from a fixed
 * tile of output positions, so that one STR of any length and one base of any
 * depth spread over the device.  The sort has two routes.  When every base has
 * at most transact_cap tokens (context option through cw_ctx_set_option,
 * default 4,096, range 1..4,096), one workgroup a base sorts the base's keys in
 * LDS.  One base above transact_cap sends the whole call through the library's
 * stable key sort over all bases at once.  Both give the same arrays; the tok
 * offsets decide, on the host, so neither route adds a wait.
 *
 * Limits: T < 2^32 - 1, M < 2^32 - 1, n_docs + T < 2^32 - 1, n_bases < 2^32 - 1,
 * and bits(n_bases) + bits(most tokens of a base) + bits(most documents + tokens
 * of a base) <= 63 (the sort key).  The node counts of all bases together,
 * those of flagged bases included (a STR in a group counts its tok_arg), must
 * stay below 2^45: above it the call fails as too large, whichever base it was.
 * Errors (< 0, cw_last_error, nothing written): null batch / result; null
 * base_doc_offsets, tok_offsets, base_new_offsets, base_node_offsets or
 * node_offsets; offsets that do not start at 0 or that decrease;
 * base_doc_offsets[n_bases] != n_docs; with n_docs > 0 a null doc_is_map; with
 * T > 0 a null tok_kind, tok_arg, tok_cause or tok_cause_is_id; with
 * n_bases > 0 a null new_tx, root_doc or base_status; only some of the ten node_*
 * and new_* arrays given; site_bits outside 1..10; site_shift or ts_shift above
 * 63; a nonzero reserved; a limit exceeded; in a full call C > new_cap or
 * M > node_cap; a bad memspace. */
int cw_transact(cw_ctx *ctx, const cw_transact_batch *batch, cw_transact_result *result, int memspace);

#ifdef __cplusplus
}
#endif
#endif /* CAUSEWEAVE_TRANSACT_H */
