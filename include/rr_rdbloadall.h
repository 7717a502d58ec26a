/*
 * rr_rdbloadall.h — RDB value payloads -> ONE rock blob batch on the GPU: the three load stages of
 * rr_rdbload.h, rr_rdbconvert.h and rr_rdbzset.h, merged.
 *
 * The stages each write a blob batch of their own; a value has size 0 in the two batches that do not
 * hold it.  rr_rdbmerge_batch gathers the three into one batch that rr_decode_batch takes as it is;
 * rr_rdbloadall_batch runs the stages into a caller-owned device workspace and merges, so that
 * payloads -> blobs is one workspace, one call, and one decode behind it.  The stage calls stay as
 * they are; nothing here changes what they write.
 *
 * The selection rule.  The first stage that holds value i wins, in the order 1, 2, 3 (s1, s2, s3 the
 * stages' statuses of the value, E_CONVERT = RR_RDBLOAD_E_CONVERT):
 *
 *   stage statuses                                   merged status          size       bytes
 *   s1 == 0                                          0                      stage 1's  stage 1's blob
 *   s1 == RR_E_CAPACITY                              RR_E_CAPACITY          stage 1's  none
 *   s1 == E_CONVERT, s2 == 0                         0                      stage 2's  stage 2's blob
 *   s1 == E_CONVERT, s2 == RR_E_CAPACITY             RR_E_CAPACITY          stage 2's  none
 *   s1 == s2 == E_CONVERT, s3 == 0                   0                      stage 3's  stage 3's blob
 *   s1 == s2 == E_CONVERT, s3 == RR_E_CAPACITY       RR_E_CAPACITY          stage 3's  none
 *   s1 == E_CONVERT, anything else behind it         RR_RDBLOAD_E_CONVERT   0          none
 *   any other s1                                     s1                     0          none
 *
 * Only the statuses decide: s1 == 0 with s2 == 0 takes stage 1.  A size "of stage k" is
 * ink->offsets[i+1] - ink->offsets[i], which the stages write even under RR_E_CAPACITY, so the merged
 * offsets[n] of a sizing run (every data_cap 0) is the full run's, LZF strings included.  A holding
 * slice with offsets[i] > offsets[i+1], or, for status 0, with offsets[i+1] > ink->data_cap, gives
 * RR_RDBMERGE_E_SLICE and size 0; it is never read.  A value that would end past out->data_cap gets
 * RR_E_CAPACITY: its size still counts in the offsets and nothing of it is written.  Bytes of
 * out->data that belong to no written value keep what they held.
 *
 * out_types[i] is the blob's type byte by the holding stage (types[i], conv_types[i],
 * RR_TYPE_ZSET_ZIPLIST) for merged status 0 and RR_E_CAPACITY, and 0xFF for every other status.
 *
 * rr_totals: bytes = offsets[n]; n_bad the values with nonzero merged status; payload the bytes
 * written to out->data; n_elems the values with merged status 0 taken from stage 2 or 3.
 *
 * Nothing outside the three input batches' [data, data + data_cap) is read.
 *
 * The one call's workspace, every part 16-byte aligned, in this order (a16 rounds up to 16):
 *   3 x u64[n + 1]      the stages' offsets              a16(24 (n + 1)) bytes
 *   3 x rr_totals       the stages' totals               96 bytes
 *   4 x u8[n]           s1, s2, s3, conv_types           a16(4 n) bytes
 *   3 data areas        of a16(stage_cap[k]) bytes
 * rr_rdbloadall_ws_bytes is that sum.  stage_cap all zero is the sizing run: the stages run at
 * data_cap 0, and the caller reads d_stage_bytes[0..3) and out->offsets[n] (or d_totals->bytes),
 * allocates, and calls again.  Without LZF strings rr_rdbloadall_caps gives the three bounds
 * (rr_rdbload_bound, rr_rdbconvert_bound, rr_rdbzset_bound), and 24 n + 8 payload_bytes bounds the
 * merged batch (a value's blob is at most 5 + 8 p from stage 1 and 24 + 4 p from stages 2 and 3).
 */
#ifndef RR_RDBLOADALL_H
#define RR_RDBLOADALL_H

#include "rr_rdbzset.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RR_RDBMERGE_E_SLICE 57   /* the holding stage's slice is reversed or past that batch's data_cap; not read */

#define RR_RDBMERGE_SPAN      8192u   /* bytes of out->data a wave of the emit kernel owns at a time */
#define RR_RDBMERGE_MAX_WAVES 8192u   /* waves of the emit launch at most, a grid stride over the spans beyond */

/* The primitive.  Device-resident: every pointer on ctx's device.  in1 / in2 / in3 and s1 / s2 / s3 are
 * the out batches and status arrays of rr_rdbload_batch, rr_rdbconvert_batch and rr_rdbzset_batch for
 * the same n values (in1->n == in2->n == in3->n == out->n); types is the loader's input, conv_types
 * rr_rdbconvert_batch's out_types.  Writes out->offsets[0..n] (complete whatever out->data_cap is),
 * out->data (16-byte aligned; may be NULL when out->data_cap is 0), status[0..n), out_types[0..n) when
 * not NULL, and *d_totals.  Three launches on `stream` (sizes, scan, emit), no host synchronisation;
 * scratch comes from the context, so rr_ctx_reserve or a warm call comes before a graph capture, as
 * for every call. */
int rr_rdbmerge_batch(rr_ctx *ctx, const rr_blob_batch *in1, const uint8_t *s1, const rr_blob_batch *in2, const uint8_t *s2,
                      const uint8_t *conv_types, const rr_blob_batch *in3, const uint8_t *s3, const uint8_t *types,
                      rr_blob_batch *out, uint8_t *out_types, uint8_t *status, rr_totals *d_totals, void *stream);

/* stage_cap[0..3) = rr_rdbload_bound, rr_rdbconvert_bound, rr_rdbzset_bound of (n, payload_bytes) */
void rr_rdbloadall_caps(uint64_t n, uint64_t payload_bytes, uint64_t stage_cap[3]);
/* the workspace's size for n values and these stage capacities (the layout above) */
uint64_t rr_rdbloadall_ws_bytes(uint64_t n, const uint64_t stage_cap[3]);

/* One call: the three stages, through their public entry points with the same opts, into ws, then
 * the merge.  in, types and opts as for rr_rdbload_batch (opts is checked first, as there); ws is
 * device memory, 16-byte aligned, of at least rr_rdbloadall_ws_bytes(n, stage_cap) bytes (else
 * RR_API_EINVAL); out, out_types, status and d_totals as for rr_rdbmerge_batch.  d_stage_bytes[0..3)
 * (device) receives each stage's offsets[n], complete whatever stage_cap is.  A value a stage could
 * not fit into its area is RR_E_CAPACITY in the merge, its size kept.  The context's scratch is sized
 * for the largest of the four steps before the first launch, so one warm call is enough before a
 * graph capture.  No host synchronisation. */
int rr_rdbloadall_batch(rr_ctx *ctx, const rr_blob_batch *in, const uint8_t *types, void *ws, uint64_t ws_bytes,
                        const uint64_t stage_cap[3], rr_blob_batch *out, uint8_t *out_types, uint8_t *status,
                        uint64_t *d_stage_bytes, rr_totals *d_totals, const rr_rdbload_opts *opts, void *stream);

/* The same over host pointers, staged through the context's device buffers; blocks.  Runs the sizing
 * run first and sizes the workspace from it, so LZF strings need no bound.  out receives
 * min(out_offsets[n], out_cap) bytes; out_types and stage_bytes[0..3) may be NULL. */
int rr_rdbloadall_batch_host(rr_ctx *ctx, const uint8_t *data, const uint64_t *offsets, const uint8_t *types, uint64_t n,
                             const rr_rdbload_opts *opts, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                             uint8_t *out_types, uint8_t *status, uint64_t *stage_bytes, rr_totals *totals);

#ifdef __cplusplus
}
#endif
#endif
