/*
 * rr_rdbconvert.h — the small encodings rdbLoadObject picks, built on the GPU: the second stage of
 * rr_rdbload.h.
 *
 * rdbLoadObject re-decides a value's encoding from the thresholds (rdb.c:1476-1600).  Where it builds
 * another encoding than the type byte names, rr_rdbload_batch stops with RR_RDBLOAD_E_CONVERT.  This
 * call takes the same input and the status rr_rdbload_batch wrote, and writes for those values the
 * rock blob (rr_format.h: u8 type | u32 lru | body) of the object the reference ends up with.  The
 * caller decodes both blob batches and merges by status.
 *
 * Value i is ATTEMPTED only when load_status[i] == RR_RDBLOAD_E_CONVERT.  Every other value gets
 * status[i] = RR_RDBCONVERT_SKIP and size 0; nothing of it is read.  An attempted value ends in
 *   0                     out_types[i] is the new type byte, the blob out_types[i] | lru & RR_LRU_MASK
 *                         | body, and desObject turns it into rdbLoadObject's object under opts
 *   RR_RDBLOAD_E_CONVERT  still the CPU path's (below); size 0, nothing written
 *   RR_E_CAPACITY         the blob would end past out->data_cap; nothing written
 * out_types[i] is the new type byte for status 0 and RR_E_CAPACITY, else 0.
 *
 * The three conversions
 *   SET 2 -> SET_INTSET 11 (rdb.c:1481-1506).  n <= set_max_intset_entries and every member passes
 *     string2ll (isSdsRepresentableAsLongLong :1501).  The body is the intset intsetAdd
 *     (intset.c:204-231) leaves after the members in payload order, starting from intsetNew (:97-102,
 *     enc 2, length 0): u32 enc | u32 length | values, little-endian, the values ascending (intsetSearch
 *     :115-154 finds the slot), a value already there dropped (:219-221), so length may be below n; enc
 *     the narrowest of 2 / 4 / 8 that holds every value (_intsetValueEncoding :45-52; intsetUpgradeAndAdd
 *     :157-180 never narrows, and the order of the adds does not matter for the widest).  n == 0: 8 bytes.
 *   HASH 4 -> HASH_ZIPLIST 13 (rdb.c:1567-1596).  n <= hash_max_ziplist_entries and every field and
 *     value has loaded length <= hash_max_ziplist_value.  The body is u64 L | ziplist, the ziplist
 *     ziplistPush(.., ZIPLIST_TAIL) (ziplist.c:956-960, __ziplistInsert :743-839) builds from field,
 *     value, field, value ... in payload order on ziplistNew (:578-586).  An entry is prevlen |
 *     encoding | data.  prevlen (zipStorePrevEntryLength :408-419): the previous entry's whole size,
 *     one byte below 254, else 0xFE | u32 LE.  zipTryEncoding (:480-504): a string of 1..31 bytes
 *     that passes string2ll is an integer entry, 0xF1 + v for 0..12, else 0xFE i8 | 0xC0 i16 | 0xF0
 *     i24 | 0xD0 i32 | 0xE0 i64 little-endian (zipSaveInteger :507-534).  Any other string
 *     (zipStoreEntryEncoding :332-364): len <= 63 one byte; <= 16383 0x40 | len >> 8, len; else 0x80 |
 *     u32 BE.  The header is u32 zlbytes | u32 zltail (the last entry's offset, 10 when empty) | u16
 *     zllen (2n; n <= 32767 keeps it below 0xFFFF), the end byte 0xFF.  n == 0: the 11 bytes of
 *     ziplistNew.  Fields and values in the LZF form are taken: their length is in the header, the
 *     bytes are decompressed into their place, those of up to 20 bytes through the LDS window for
 *     the integer test (a longer string cannot pass string2ll).
 *   ZSET_2 5 -> ZSET_ZIPLIST 12 (rdb.c:1553-1555).  n <= zset_max_ziplist_entries and the longest
 *     member <= zset_max_ziplist_value.  zsetConvert (t_zset.c:1210-1235) walks the skiplist from its
 *     head and zzlInsertAt (:1029-1038) pushes ele, then the score's text, at the tail.  The
 *     skiplist's order (zslInsert :132-151): ascending by score compared as doubles (-0 == 0), ties by
 *     sdscmp (sds.c:792-802: memcmp over the shorter length, then the shorter first).  The score's
 *     text is d2string's (util.c:517-552), pushed like any string: "17" becomes an integer entry;
 *     "-0", "inf" and "-inf" stay strings.  A member that is there twice is kept twice: the
 *     reference's skiplist holds both (its dictAdd fails unnoticed, rdb.c:1549), and rejecting such a
 *     value is rr_decode_batch's business.
 *
 * What stays RR_RDBLOAD_E_CONVERT [deviations]
 *   a ZSet with a score d2string hands to snprintf("%.17g") (util.c:548): any score other than
 *     +-inf, +-0 or an integer-valued double strictly between -(2^52 - 1) and 2^52 (:542-545);
 *     with a NaN score (the reference asserts, t_zset.c:137); with a member in the LZF form (the
 *     sort compares member bytes in place);
 *   a Set or ZSet of more than RR_RDBCONVERT_MAX_N members (the per-wave sort arrays in LDS).  A Hash
 *     needs no sort: its only limit is the 32767 of the options;
 *   a ziplist of 0x7FFFFFF0 bytes or more;
 *   the reverse conversions (a stored intset or ziplist above the loader's thresholds, or zllen ==
 *     0xFFFF: rdb.c:1683-1699) and the List values of rr_rdbload.h (an oversize LZF node);
 *   a value whose load_status the loader would not have given: another type, a malformed payload,
 *     a bad slice, thresholds not met.  The walk reads through a buffer resource over the value's
 *     own slice and never outside it.
 *
 * rr_totals: bytes = offsets[n]; n_bad the attempted values not converted (RR_RDBLOAD_E_CONVERT or
 * RR_E_CAPACITY); over the values written, payload = the bytes of the intset blob or the ziplist (what
 * rr_rdbload.h counts for a value stored in that form) and n_elems = the strings read (members; fields
 * and values; members).
 */
#ifndef RR_RDBCONVERT_H
#define RR_RDBCONVERT_H

#include "rr_rdbload.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RR_RDBCONVERT_SKIP      45     /* not attempted: load_status[i] != RR_RDBLOAD_E_CONVERT */

#define RR_RDBCONVERT_MAX_N     512u   /* the most members of a Set or ZSet that is sorted (both default thresholds fit) */
#define RR_RDBCONVERT_MAX_WAVES 16384u /* a wave an attempted value; a launch has at most this many, a grid stride beyond */

/* Upper bound on offsets[n] for n payloads of payload_bytes in all that hold NO LZF string:
 * 24 * n + 4 * payload_bytes, rounded up to 16.  A ziplist blob has 5 + 8 + 11 fixed bytes (header, L,
 * the ziplist's header and end byte), an intset blob 5 + 8; the count byte becomes nothing.  What
 * follows grows by at most 4 bytes per payload byte:
 *   a Set member costs at least 2 payload bytes ("5", or 0xC0 + 1) and becomes at most 8 (2 -> 8);
 *   a plain string of len bytes costs len_bytes + len and becomes an entry of at most prevlen +
 *   header + len, where the header has the length prefix's own size (the breakpoints 64 and 16384
 *   are the same) and prevlen is 1, or 5 behind an entry of 254 bytes or more, whose own payload was
 *   at least 250 bytes (1 -> 2 for the empty string, the worst case; 250 -> 256);
 *   0xC0 + 1 byte becomes prevlen + 0xFE + 1 (2 -> 3), 0xC1 + 2 becomes 4, 0xC2 + 4 becomes 6;
 *   the 8 score bytes become at most prevlen + 0xE0 + 8 (8 -> 10).
 * An LZF string can expand 88-fold: callers with LZF strings ask for the size with data_cap 0. */
uint64_t rr_rdbconvert_bound(uint64_t n, uint64_t payload_bytes);

/* Device-resident: every pointer on ctx's device.  in, types and opts are what rr_rdbload_batch was
 * given, load_status[0..n) the status it wrote.  out->n == in->n; writes out->offsets[0..n] (complete
 * whatever out->data_cap is), out->data (may be NULL when out->data_cap is 0), out_types[0..n),
 * status[0..n) and *d_totals.  Six launches on `stream` (flags, scan, compaction, sizes, scan, emit),
 * no host synchronisation; scratch comes from the context, so rr_ctx_reserve or a warm call comes
 * before a graph capture, as for every call. */
int rr_rdbconvert_batch(rr_ctx *ctx, const rr_blob_batch *in, const uint8_t *types, const uint8_t *load_status,
                        rr_blob_batch *out, uint8_t *out_types, uint8_t *status, rr_totals *d_totals,
                        const rr_rdbload_opts *opts, void *stream);

/* The same over host pointers, staged through the context's device buffers; blocks.  out receives
 * min(out_offsets[n], out_cap) bytes. */
int rr_rdbconvert_batch_host(rr_ctx *ctx, const uint8_t *data, const uint64_t *offsets, const uint8_t *types,
                             const uint8_t *load_status, uint64_t n, const rr_rdbload_opts *opts, uint8_t *out,
                             uint64_t out_cap, uint64_t *out_offsets, uint8_t *out_types, uint8_t *status,
                             rr_totals *totals);

#ifdef __cplusplus
}
#endif
#endif
