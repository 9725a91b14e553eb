/*
 * causeweave_render_bases.h -- cb->edn (base/core.cljc:83-96) for a batch of
 * causal bases: the root collection of every base with each
 * :causal.collection.ref/... value replaced by the collection it names,
 * recursively, as one depth-first token stream per base.  cw_render_lists /
 * cw_render_maps make the entries; this call resolves the refs.  The
 * conventions are causeweave.h's.
 *
 * The batch is an ENTRY TABLE over n_docs documents (collections, lists and
 * maps alike): entry e of document d is the (e - ent_offsets[d])-th rendered
 * value of d, in render order, and ent_ref[e] is UINT32_MAX for a scalar, any
 * other value the batch-wide document that the value refers to.  That is what
 * cw_render_lists / cw_render_maps write into rendered_value / entry_value
 * when the value column is the ref_doc column (value_size 4): lists rendered
 * by one call and maps by another become one table by placing the two outputs
 * one after the other (documents numbered lists first, then maps).
 *
 * A base is what its root reaches, not a run of documents: root_doc[g] is the
 * root collection of base g; any value >= n_docs means the base has no root.
 *
 *   claims[d]   the number of entries of the whole batch with ent_ref == d,
 *               plus the number of bases with root_doc == d.
 *   tree ref    an entry whose target t < n_docs has claims[t] == 1.
 *   the stream  of base g is go(root_doc[g], UINT32_MAX), where go(d, via) emits
 *                 1. (CW_TOK_OPEN, d, via)
 *                 2. for each entry e of d, in order:
 *                      a scalar                 (CW_TOK_LEAF, d, e)
 *                      a ref, target >= n_docs  (CW_TOK_NIL, d, e)   (get-in gives nil)
 *                      a tree ref               go(target, e)
 *                 3. (CW_TOK_CLOSE, d, via)
 *               with e the batch-wide entry index.
 *   flagged     base_status[g] = CW_STATUS_REF_SHARED when the root has
 *               claims >= 2, or when any entry of a document the base reaches
 *               through tree refs refers to a document with claims >= 2: a
 *               reference cycle, a collection referred to twice, a root that
 *               is referred to.  A flagged base emits no tokens; the host
 *               renders it.  Claims from documents that no base reaches count:
 *               the result does not depend on which referrer is met first.
 *
 * A base without a root emits nothing and has status 0.  An empty root
 * collection emits two tokens (nil and [] differ).
 */
#ifndef CAUSEWEAVE_RENDER_BASES_H
#define CAUSEWEAVE_RENDER_BASES_H

#include "causeweave.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { CW_STATUS_REF_SHARED = 1u << 9 }; /* base_status: a collection the base reaches is claimed twice */

enum { CW_TOK_OPEN = 0, CW_TOK_CLOSE = 1, CW_TOK_LEAF = 2, CW_TOK_NIL = 3 };

typedef struct {
  uint64_t n_docs;
  const uint64_t *ent_offsets;   /* HOST [n_docs+1]; E = ent_offsets[n_docs] */
  const uint32_t *ent_ref;       /* [E] UINT32_MAX = a scalar, else the document referred to */
  uint64_t n_bases;
  const uint32_t *root_doc;      /* [n_bases] the base's root document; >= n_docs: none */
} cw_render_bases_batch;

typedef struct {
  uint64_t *base_tok_offsets;    /* HOST [n_bases+1]: the tokens of base g; T = base_tok_offsets[n_bases] */
  uint8_t  *tok_kind;            /* [E + 2 * n_docs] CW_TOK_*; T elements written */
  uint32_t *tok_doc;             /* [E + 2 * n_docs] the document the token belongs to */
  uint32_t *tok_entry;           /* [E + 2 * n_docs] LEAF / NIL: the entry; OPEN / CLOSE: via (UINT32_MAX for a root) */
  uint32_t *base_status;         /* [n_bases] 0 or CW_STATUS_REF_SHARED */
  uint32_t *doc_base;            /* [n_docs] or NULL: the base that reaches d; UINT32_MAX if none or flagged */
  uint32_t *doc_open;            /* [n_docs] or NULL: the global token position of d's OPEN; unspecified where doc_base is UINT32_MAX */
} cw_render_bases_result;

/* memspace: where every array lives except ent_offsets and base_tok_offsets
 * (host memory).  A host call stages through the context's scratch.  Under
 * cw_ctx_set_async the call waits once, for the base offsets, and for nothing
 * else; when ent_offsets differ from the previous call's they are also
 * uploaded with blocking copies.
 *
 * tok_kind, tok_doc and tok_entry may all three be NULL: the count-only call
 * (offsets, status, doc_base; doc_open as it would be).  Exactly T elements of
 * each are written, nothing past them.
 *
 * Limits: E + 2 * n_docs < 2^32 - 1, n_docs < 2^31 - 1, n_bases < 2^32 - 1.
 * Errors (< 0, cw_last_error, nothing written): null batch / result; null
 * ent_offsets; offsets that do not start at 0 or that decrease; a null ent_ref
 * with E > 0; with n_bases > 0 a null root_doc or base_status; a null
 * base_tok_offsets; only some of the three token arrays given; a limit
 * exceeded; a bad memspace. */
int cw_render_bases(cw_ctx *ctx, const cw_render_bases_batch *batch, cw_render_bases_result *result, int memspace);

#ifdef __cplusplus
}
#endif
#endif /* CAUSEWEAVE_RENDER_BASES_H */
