/*
 * rr_rdbload.h — RDB value payloads -> rock blobs on the GPU: the load direction of rr_rdbsave.h.
 *
 * Whoever holds RDB value payloads (a dump.rdb at start-up, a full sync, RESTORE, MIGRATE) and wants
 * them in the store would run rdbLoadObject (rdb.c:1450-1700) and then serObject per key, building a
 * robj whose only use is to be serialized and freed.  These calls write, for value i with RDB type
 * byte types[i] and payload data[offsets[i] .. offsets[i+1]) — exactly the shape rr_rdbsave_batch
 * writes — the rock blob (rr_format.h: u8 type | u32 lru | body) that desObject turns into the
 * object rdbLoadObject builds from that payload.  The RDB type numbers (rdb.h:75-92) equal the rock
 * tags, so the blob's type byte is types[i].  rr_decode_batch takes the blobs from there, with every
 * acceptance rule it has (duplicates, NaN scores, skiplist order, ziplist checks): none of those is
 * repeated here.
 *
 * Primitives
 *   rdbLoadLen (rdb.c:190-234): the first byte's top two bits choose the form: 00 the low 6 bits;
 *     01 14 bits, (b0 & 0x3F) << 8 | b1; 0x80 then u32 big-endian; 0x81 then u64 big-endian;
 *     0x82..0xBF: "Unknown length encoding" (:219), RR_RDBLOAD_E_LEN.  11 (0xC0..0xFF) is an
 *     "encoded" value, the low 6 bits (:197-200).  At a COUNT site (the element counts :1478, :1523,
 *     :1561, :1620 and the two lengths of an LZF string :376-377) the reference passes isencoded ==
 *     NULL and takes those 6 bits as the number: 0xC5 is a count of 5.  This is followed exactly.
 *   strings (rdbGenericLoadStringObject, rdb.c:487-540), three forms:
 *     plain    rdbLoadLen(len) then len bytes;
 *     integer  0xC0 i8 | 0xC1 i16 | 0xC2 i32, little-endian, sign-extended: the string is the
 *              decimal text ll2string gives (rdbLoadIntegerObject :266-302);
 *     LZF      0xC3 | len(clen) | len(len) | clen stream bytes (rdbLoadLzfStringObject :369-407);
 *              the stream is what lzf_decompress reads (lzf_d.c:68-184, restated in rr_rdbsave.h);
 *     an encoding byte 0xC4..0xFF: "Unknown RDB string encoding type" (:512), RR_RDBLOAD_E_LEN.
 *   Anything that runs past the value's slice: RR_RDBLOAD_E_TRUNC (the reference's rioRead fails).
 *   An LZF stream that does not decompress to exactly len bytes: RR_RDBLOAD_E_LZF.  That is what
 *   makes lzf_decompress return 0 (an empty stream, a back reference before the string's start
 *   :139, input overrun :83/:113/:123, output overrun :76/:133), where the reference exits
 *   (rdb.c:390-392), and [stricter] a stream that ends with fewer than len bytes, which the
 *   reference loads with an uninitialised tail, and a len of 0x7FFFFFF0 or more.
 *   Bytes left over after the value: RR_RDBLOAD_E_EXTRA.
 *
 * Per type (a type byte other than these eight, the legacy types 1, 3, 9, 10, streams and modules
 * included: RR_RDBLOAD_E_TYPE)
 *   STRING 0           the integer form gives enc INT + i64.  Otherwise tryObjectEncoding
 *                      (rdb.c:1458, object.c:431-508): len <= 20 and string2l gives INT (:458);
 *                      len <= 44 EMBSTR (:489); else RAW
 *   LIST_QUICKLIST 14  a count of nodes, then a string per node, each a ziplist (rdb.c:1619-1630).
 *                      Every node is walked by the decoder's strict ziplist rule (RR_E_ZL_CORRUPT,
 *                      ziplist.c:300-447: zlbytes, zltail, zllen, the prevlen chain, the encodings,
 *                      the end byte) and every entry written as u32 len | bytes, integer entries as
 *                      sdsll2str renders them (what serList writes).  A node that fails, or is shorter
 *                      than 11 bytes: RR_RDBLOAD_E_ZIPLIST [stricter]: the reference appends nodes
 *                      blind (quicklistAppendZiplist).  An empty node contributes nothing
 *   SET 2              count, strings      -> u64 n | {u64 len, bytes}*
 *   HASH 4             count, 2 * strings  -> u64 n | {u64 fl, f, u64 vl, v}*
 *   ZSET_2 5           count, {string, 8 score bytes} -> u64 n | {u64 l, ele, f64}*, the score bytes
 *                      copied in payload order (rdbLoadBinaryDoubleValue)
 *   SET_INTSET 11      one string, the intset blob, which is the body as it is.  Shorter than 8
 *                      bytes, enc not 2 / 4 / 8, or length != 8 + enc * n: RR_RDBLOAD_E_ZIPLIST
 *   HASH_ZIPLIST 13    one string -> u64 L | bytes.  Fewer than 11 bytes: RR_RDBLOAD_E_ZIPLIST.  The
 *   ZSET_ZIPLIST 12    entries are not walked here: decode does that, strictly or under RR_CTX_ZL_RAW
 *   Order, duplicates and NaN are rr_decode_batch's business.
 *
 * Encoding conversions.  rdbLoadObject re-decides the encoding from the thresholds (rdb.c:1481-1506,
 * :1553-1555, :1567-1596, :1683-1699).  A value for which it would build another encoding than its
 * type byte names gets RR_RDBLOAD_E_CONVERT and is left for the caller's CPU path; every value with
 * status 0 is therefore exactly the reference's object:
 *   SET           n <= set_max_intset_entries and every member passes string2ll (n == 0 included)
 *   HASH          n <= hash_max_ziplist_entries and every field and value has loaded length
 *                 <= hash_max_ziplist_value (n == 0 included)
 *   ZSET_2        n <= zset_max_ziplist_entries and the longest member <= zset_max_ziplist_value
 *   SET_INTSET    the header's n > set_max_intset_entries
 *   the ziplists  zllen / 2 above their *_entries; zllen == 0xFFFF always (the reference then counts
 *                 the entries, and *_entries <= 32767 makes "always" exact)
 * Deviation: a List node in the LZF form whose len is above RR_RDBLOAD_LZF_NODE_MAX also gets
 * RR_RDBLOAD_E_CONVERT: a node has to be decompressed before it can be walked, and the kernels do
 * that in on-chip memory.  (rr_rdbsave_batch writes nodes raw; the reference's own snapshots hold
 * nodes of up to 8 KiB under the default list-max-ziplist-size -2.)
 *
 * Status.  The first defect the walk meets decides; RR_RDBLOAD_E_EXTRA comes after the walk and
 * RR_RDBLOAD_E_CONVERT last.  A slice with offsets[i] > offsets[i+1] or offsets[i+1] > in->data_cap
 * is RR_RDBLOAD_E_TRUNC and a payload of 0x7FFFFFF0 bytes or more RR_RDBLOAD_E_LEN; neither is read.
 * A value with nonzero status has size 0 and writes nothing.  A value that would end past
 * out->data_cap gets RR_E_CAPACITY (rr_format.h) and writes nothing; out->offsets[0..n] are complete
 * whatever data_cap is, so a caller with LZF strings and no bound calls once with data_cap 0, reads
 * offsets[n] and calls again.  Nothing outside a value's own payload slice is read.
 *   rr_totals: bytes = offsets[n]; n_bad the values with nonzero status; and over the values
 * written, payload = the string bytes placed in blobs (members, fields, values, List entries, the
 * bytes of a RAW / EMBSTR String, an intset blob, a ziplist) and n_elems = the strings read plus the
 * List entries walked.
 */
#ifndef RR_RDBLOAD_H
#define RR_RDBLOAD_H

#include "rr_serdes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-value status beside RR_OK and RR_E_CAPACITY (rr_format.h) */
#define RR_RDBLOAD_E_TYPE     32   /* not one of the eight types */
#define RR_RDBLOAD_E_LEN      33   /* unknown length or string encoding byte */
#define RR_RDBLOAD_E_TRUNC    34   /* runs past the value's slice */
#define RR_RDBLOAD_E_LZF      35   /* the stream does not decompress to exactly len bytes */
#define RR_RDBLOAD_E_EXTRA    36   /* bytes left over after the value */
#define RR_RDBLOAD_E_ZIPLIST  37   /* List node / intset blob / ziplist string malformed [stricter] */
#define RR_RDBLOAD_E_CONVERT  38   /* the reference would build another encoding: the CPU path's */

#define RR_RDBLOAD_LZF_NODE_MAX 10240u   /* the longest List node taken in the LZF form */

typedef struct rr_rdbload_opts {
    uint32_t lru;                       /* written into every blob, & RR_LRU_MASK (createObject's LRU_CLOCK(), object.c:41-53) */
    uint32_t set_max_intset_entries;    /* 512  config.c:2262 */
    uint32_t hash_max_ziplist_entries;  /* 512  :2261 */
    uint32_t hash_max_ziplist_value;    /* 64   :2265 */
    uint32_t zset_max_ziplist_entries;  /* 128  :2263 */
    uint32_t zset_max_ziplist_value;    /* 64   :2267 */
    uint32_t flags;                     /* 0; any bit: RR_API_EINVAL */
} rr_rdbload_opts;                      /* NULL: the defaults, lru 0.  An *_entries above 32767: RR_API_EINVAL */

/* Upper bound on offsets[n] for n payloads of payload_bytes in all that hold NO LZF string:
 * 5 * n + 8 * payload_bytes, rounded up to 16.  Every blob has the 5-byte header; what follows grows
 * by at most 8 bytes per payload byte:
 *   a count byte becomes the u64 count (Set, Hash, ZSet: 1 -> 8) or nothing (List); the length byte
 *   of a ziplist string becomes its u64 L (1 -> 8), that of an intset blob nothing;
 *   a one-byte empty string becomes an 8-byte length (1 -> 8, the worst case); a plain string of
 *   len bytes costs at least 1 + len and becomes 8 + len;
 *   0xC0 + 1 byte becomes 8 + at most 4 digits ("-128": 2 -> 12), 0xC1 + 2 becomes 8 + 6 (3 -> 14),
 *   0xC2 + 4 becomes 8 + 11 (5 -> 19); as a String they become enc + i64 (2 -> 9);
 *   a String's length byte becomes its enc byte (1 -> 1);
 *   a List node's header and end byte (11 bytes) become nothing; a 2-byte small-integer entry becomes
 *   4 + 1 or 4 + 2 ("12"), a 3-byte int8 entry 4 + 4, an 10-byte int64 entry 4 + 20, a string entry
 *   of len bytes (at least 2 + len) 4 + len.
 * An LZF string can expand 88-fold (a 3-byte sequence gives 264 bytes): callers with LZF strings
 * ask for the size with data_cap 0. */
uint64_t rr_rdbload_bound(uint64_t n, uint64_t payload_bytes);

/* Device-resident: every pointer on ctx's device.  out->n == in->n; reads in->data[0, in->data_cap),
 * in->offsets[0..n] and types[0..n); writes out->offsets[0..n], out->data, status[0..n) and
 * *d_totals.  out->data may be NULL when out->data_cap is 0.  opts may be NULL.  Three launches on
 * `stream` (sizes, scan, emit), no host synchronisation; scratch comes from the context, so
 * rr_ctx_reserve or a warm call comes before a graph capture, as for every call. */
int rr_rdbload_batch(rr_ctx *ctx, const rr_blob_batch *in, const uint8_t *types, rr_blob_batch *out,
                     uint8_t *status, rr_totals *d_totals, const rr_rdbload_opts *opts, void *stream);

/* The same over host pointers, staged through the context's device buffers; blocks.  out receives
 * min(out_offsets[n], out_cap) bytes. */
int rr_rdbload_batch_host(rr_ctx *ctx, const uint8_t *data, const uint64_t *offsets, const uint8_t *types,
                          uint64_t n, const rr_rdbload_opts *opts, uint8_t *out, uint64_t out_cap,
                          uint64_t *out_offsets, uint8_t *status, rr_totals *totals);

#ifdef __cplusplus
}
#endif
#endif
