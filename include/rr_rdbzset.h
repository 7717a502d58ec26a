/*
 * rr_rdbzset.h — small ZSets with fractional scores as ziplists, built on the GPU: the third stage of
 * rr_rdbload.h, behind rr_rdbconvert.h.
 *
 * rr_rdbconvert_batch builds a ZSET_2 value's ziplist only when d2string (util.c:517-552) prints every
 * score without snprintf("%.17g"); one score such as 1.5 leaves the value at RR_RDBLOAD_E_CONVERT.
 * This call takes the same input and the status rr_rdbconvert_batch wrote, and writes the ziplist blob
 * for those values, the score's text from rr_d2string.h's exact %.17g.  The caller decodes the three
 * blob batches and merges by status.
 *
 * Value i is ATTEMPTED only when types[i] == 5 (ZSET_2) and convert_status[i] == RR_RDBLOAD_E_CONVERT.
 * Every other value gets status[i] = RR_RDBZSET_SKIP and size 0; nothing of it is read.  An attempted
 * value ends in
 *   0                     the blob 12 (ZSET_ZIPLIST) | lru & RR_LRU_MASK | u64 L | ziplist, which
 *                         desObject turns into rdbLoadObject's object under opts.  The type is always
 *                         12, so there is no out_types
 *   RR_RDBLOAD_E_CONVERT  still the CPU path's (below); size 0, nothing written
 *   RR_E_CAPACITY         the blob would end past out->data_cap; nothing written
 *
 * The rule is rr_rdbconvert.h's ZSET_2 -> ZSET_ZIPLIST with its first deviation removed: the same
 * thresholds (n <= zset_max_ziplist_entries, the longest member <= zset_max_ziplist_value), the same
 * order (zslInsert, t_zset.c:132-151: scores compared as doubles, -0 == 0, ties by sdscmp), a member
 * that is there twice kept twice, member then score pushed at the tail (zzlInsertAt :1029-1038).  The
 * score's text is d2string's for every score that is not a NaN, the integer-valued ones included, and
 * is pushed like any string, so zipTryEncoding (ziplist.c:480-504) applies: "17", "4503599627370496"
 * and "10000000000000000" pass string2ll and are integer entries; "1.5", "1e+17", "-0" and "inf" stay
 * strings.  A value with integer scores only, handed to this stage, gives rr_rdbconvert_batch's bytes.
 *
 * What stays RR_RDBLOAD_E_CONVERT [deviations]
 *   a NaN score (the reference asserts, t_zset.c:137); a member in the LZF form (the sort compares
 *   member bytes in place); more than RR_RDBCONVERT_MAX_N members; a ziplist of 0x7FFFFFF0 bytes or
 *   more; thresholds not met; a malformed payload or a bad slice.  The walk reads through a buffer
 *   resource over the value's own slice: a value that is not what its status claims reads zeros,
 *   never a neighbour.
 *
 * rr_totals as in rr_rdbconvert.h: bytes = offsets[n]; n_bad the attempted values not converted; over
 * the values written, payload = the ziplists' bytes and n_elems = the members.
 */
#ifndef RR_RDBZSET_H
#define RR_RDBZSET_H

#include "rr_rdbconvert.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RR_RDBZSET_SKIP 55     /* not attempted: not a ZSET_2 that rr_rdbconvert_batch left at RR_RDBLOAD_E_CONVERT */

/* Upper bound on offsets[n] for n ZSET_2 payloads of payload_bytes in all: 24 * n + 4 * payload_bytes,
 * rounded up to 16 (rr_rdbconvert_bound's figure).  A blob has 5 + 8 + 11 fixed bytes; the count
 * byte becomes nothing.  A member of len bytes costs len_bytes + len and becomes at most prevlen +
 * header + len with a header of the length prefix's size, prevlen 1 (a score's entry is at most 30
 * bytes); 0xC0 + 1 byte becomes 1 + 0xFE + 1, 0xC1 + 2 becomes 4, 0xC2 + 4 becomes 6.  The 8 score
 * bytes become at most prevlen + 1 + 24, prevlen 5 only behind a member of 250 bytes or more.  The
 * worst case is the empty member with a 24-byte score: 1 + 8 bytes become 2 + 26 (9 -> 28). */
uint64_t rr_rdbzset_bound(uint64_t n, uint64_t payload_bytes);

/* Device-resident: every pointer on ctx's device.  in, types and opts are what rr_rdbload_batch and
 * rr_rdbconvert_batch were given, convert_status[0..n) the status rr_rdbconvert_batch wrote.  out->n ==
 * in->n; writes out->offsets[0..n] (complete whatever out->data_cap is), out->data (may be NULL when
 * out->data_cap is 0), status[0..n) and *d_totals.  Six launches on `stream` (flags, scan, compaction,
 * sizes, scan, emit), a wave per attempted value and at most RR_RDBCONVERT_MAX_WAVES waves a launch, no
 * host synchronisation; scratch comes from the context, so rr_ctx_reserve or a warm call comes before
 * a graph capture, as for every call.  Option checks and error texts are rr_rdbload_batch's. */
int rr_rdbzset_batch(rr_ctx *ctx, const rr_blob_batch *in, const uint8_t *types, const uint8_t *convert_status,
                     rr_blob_batch *out, uint8_t *status, rr_totals *d_totals, const rr_rdbload_opts *opts, void *stream);

/* The same over host pointers, staged through the context's device buffers; blocks.  out receives
 * min(out_offsets[n], out_cap) bytes. */
int rr_rdbzset_batch_host(rr_ctx *ctx, const uint8_t *data, const uint64_t *offsets, const uint8_t *types,
                          const uint8_t *convert_status, uint64_t n, const rr_rdbload_opts *opts, uint8_t *out,
                          uint64_t out_cap, uint64_t *out_offsets, uint8_t *status, rr_totals *totals);

#ifdef __cplusplus
}
#endif
#endif
