/*
 * causeweave_sync.h -- what a replica needs before a merge: its version vector
 * and the nodes a peer lacks.  The per-site heads are (peek yarn) of every yarn
 * of s/spin (shared.cljc:96-108, what refresh-ts and the caller of s/weft read);
 * the delta is the complement of what s/weft (shared.cljc:268-293) keeps, the
 * diff that merge-trees' own comment (shared.cljc:295-299) asks for.  Both calls
 * read ids only, so one batch type serves lists and maps.  The conventions are
 * causeweave.h's.
 *
 * The site rank of a node is (id_key >> site_shift) & (2^site_bits - 1); every
 * comparison of ids is unsigned 64-bit.
 */
#ifndef CAUSEWEAVE_SYNC_H
#define CAUSEWEAVE_SYNC_H

#include "causeweave.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint64_t n_docs;
  const uint64_t *doc_offsets;   /* HOST [n_docs+1] */
  const uint64_t *id_key;        /* [N] */
  const uint64_t *cause;         /* [N] or NULL (only gathered, never interpreted) */
  const uint8_t  *kind;          /* [N] or NULL (only gathered) */
  const uint8_t  *cause_is_id;   /* [N] or NULL (maps; only gathered) */
  uint32_t ts_shift;
  uint32_t site_shift;
  uint32_t site_bits;            /* 1..10 */
  uint32_t reserved;             /* 0 */
} cw_sync_batch;

typedef struct {
  uint64_t *ver;                 /* [n_docs << site_bits] ver[(d << site_bits) | r]: the largest id_key of site rank r in document d; 0: none, or only id 0 (the root) */
  uint32_t *yarn_len;            /* [n_docs << site_bits] or NULL: the nodes of that rank, (count yarn); the root counts in its own rank */
  uint64_t *max_ts;              /* [n_docs] or NULL: largest id >> ts_shift, 0 for an empty document (refresh-ts) */
} cw_version_result;

/* Every word of ver (and of yarn_len, max_ts when given) is written.  ver is a
 * cut table of cw_weft_lists_dev / cw_weft_maps as it stands (0 = not named):
 * the weft at a document's own version keeps every node.
 *
 * memspace: where id_key and the three outputs live; doc_offsets is host memory.
 * A device-memory call reads nothing back and, under cw_ctx_set_async, waits for
 * nothing, except that doc_offsets which differ from the previous call's are
 * uploaded with blocking copies.
 *
 * Routes, by the largest document of the batch; all give the same arrays:
 *   wave       <= 256 nodes (CW_SYNC_WAVE_CAP): a wave per document, four
 *              documents a workgroup (stat "sync_ver_wave");
 *   workgroup  <= 65,535 nodes: a workgroup per document ("sync_ver_wg");
 *   tiled      anything larger: fixed tiles of 8,192 node positions, 64-bit
 *              atomics onto the zeroed table ("sync_ver_tiled").
 * Context options (0/1, default 1): sync_wave = 0 sends small documents to the
 * workgroup route, sync_fused = 0 every call to the tiled route.
 *
 * Limits and errors: as cw_delta's, below. */
int cw_version(cw_ctx *ctx, const cw_sync_batch *batch, cw_version_result *result, int memspace);

#define CW_SYNC_WAVE_CAP 256

typedef struct {
  uint64_t *delta_offsets;       /* HOST [n_docs+1] */
  uint32_t *delta_src;           /* [N] (sized for N; delta_offsets[n_docs] entries written): the doc-local input index of each delta node, per document in input order */
  uint64_t *delta_id;            /* [N] or NULL */
  uint64_t *delta_cause;         /* [N]; NULL exactly when cause is NULL */
  uint8_t  *delta_kind;          /* [N]; NULL exactly when kind is NULL */
  uint8_t  *delta_cause_is_id;   /* [N]; NULL exactly when cause_is_id is NULL */
  uint32_t *ahead;               /* [n_docs] or NULL: the site ranks with have > ver, the peer holds nodes this side lacks */
} cw_delta_result;

/* have[(d << site_bits) | r] (in memspace): the peer's head for that site, 0 =
 * the peer has nothing of it; the format of ver above.  A node is in the delta
 * iff id_key > have[its site rank], and by nothing else: the kind is not read,
 * so a root with id 0 is never in a delta; a have word need not be a node of the
 * document; a have word whose site field is not its own rank is still just a
 * number to compare with.
 *
 * The delta of document d, delta_*[delta_offsets[d] .. delta_offsets[d+1]), is
 * one side of a cw_list_batch / cw_map_batch of its own with delta_offsets as
 * its offsets: side b of cw_merge_lists / cw_merge_maps.  Nothing is written
 * past delta_offsets[n_docs] entries of any per-node output.
 *
 * memspace: where every array lives except doc_offsets and delta_offsets (host
 * memory).  Under cw_ctx_set_async the call waits once, for the offsets (and
 * uploads doc_offsets when they changed).
 *
 * Routes: the wave and workgroup routes of cw_version, one kernel with the first
 * output position of a workgroup found by look-back ("sync_delta_wave",
 * "sync_delta_wg"; with ahead the kernel makes the version row in LDS); a
 * larger document, or sync_fused = 0, takes the general route: a count pass, a
 * host scan, a write pass ("sync_delta_count", "sync_delta_write"; with ahead,
 * the tiled version and "sync_ahead" first).
 *
 * Limits: N < 2^32 - 1, n_docs << site_bits < 2^32 - 1, n_docs < 2^22 (a
 * workgroup of 1,024 threads a document must fit one dispatch, on every route).
 * Errors (< 0, cw_last_error, nothing written): null batch / result / have
 * (cw_delta); null doc_offsets or
 * delta_offsets; a null ver with n_docs > 0; with N > 0 a null id_key or
 * delta_src; delta_cause, delta_kind or delta_cause_is_id set without its input
 * column or the reverse; offsets that do not start at 0 or that decrease;
 * site_bits outside 1..10; site_shift or ts_shift above 63; N >= 2^32 - 1;
 * n_docs << site_bits >= 2^32 - 1; n_docs >= 2^22; a bad memspace. */
int cw_delta(cw_ctx *ctx, const cw_sync_batch *batch, const uint64_t *have, cw_delta_result *result, int memspace);

#ifdef __cplusplus
}
#endif
#endif /* CAUSEWEAVE_SYNC_H */
