/*
 * rr_rdbsave.h — flat batch -> RDB value payloads on the GPU.
 *
 * In the reference a snapshot child that meets an evicted value fetches its blob, builds a robj
 * with desObject (rock.c:527-550) and uses that object once: rdbSaveObjectType + rdbSaveObject
 * (rdb.c:1017-1073), then frees it.  These calls write what rdbSaveObject would write straight from
 * the flat form of rr_format.h, so the child needs no object: it copies type | key | payload.
 *
 * For value i the call gives a type byte types[i] and a payload data[offsets[i] .. offsets[i+1]).
 * The payload is what rdbSaveObject (rdb.c:761-900) writes, with `rdbcompression no` (with
 * RR_RDBSAVE_LZF: with the LZF string form of `rdbcompression yes`, see "LZF" below), for the object
 * desObject builds from the blob rr_encode_batch writes for that value.  types[i] is
 * rdbSaveObjectType's byte (rdb.c:632-670); the RDB numbers (rdb.h:75-92) equal the rock tags the
 * flat form carries — STRING 0, SET 2, HASH 4, ZSET_2 5, SET_INTSET 11, ZSET_ZIPLIST 12,
 * HASH_ZIPLIST 13, LIST_QUICKLIST 14 — so types[i] is rr_value.type, copied for every value.
 *
 * Primitives
 *   rdbSaveLen (rdb.c:147-178): len < 64: one byte; len < 16384: 0x40 | len >> 8, len & 0xFF;
 *     len <= UINT32_MAX: 0x80 then u32 big-endian; else 0x81 then u64 big-endian.  rr_elem.len and
 *     every count are 32-bit, so the 64-bit form cannot occur for a string, a count or a List node
 *     of valid ziplist size; the one length that can pass 2^32 is the intset blob of more than 2^29
 *     8-byte members, and the 64-bit form is written for it.
 *   rdbSaveRawString (rdb.c:411-441): when len <= 11 and the bytes are the canonical decimal of a
 *     value in int32 range (rdbTryIntegerEncoding :307-321: strtoll, then ll2string must give the
 *     same bytes) it writes rdbEncodeInteger's form (:241-261): 0xC0 i8 | 0xC1 i16 | 0xC2 i32, the
 *     integer little-endian.  Otherwise rdbSaveLen(len) then the bytes.
 *   rdbSaveLongLongAsStringObject (rdb.c:444-460): the integer forms when the value is in int32
 *     range, otherwise rdbSaveLen(digits) then the decimal text.
 *
 * Per type
 *   STRING          INT: rdbSaveLongLongAsStringObject; RAW / EMBSTR: rdbSaveRawString
 *   SET_INTSET      rdbSaveRawString of the intset blob: u32 enc | u32 n | n * enc bytes, little-endian
 *                   ints in the flat order (its first byte is 2, 4 or 8: never the integer form)
 *   HASH_ZIPLIST    rdbSaveRawString of the ZLRAW bytes; only descriptor 0 is read, as in
 *   ZSET_ZIPLIST    rr_encode_batch, so RR_CTX_ZL_RAW batches work unchanged.  An L <= 11 ziplist
 *                   that reads as a decimal integer is integer-encoded, as the reference would
 *   SET_HT          rdbSaveLen(n) then rdbSaveRawString per member
 *   HASH_HT         rdbSaveLen(n / 2) then field, value per pair
 *   ZSET_SKIPLIST   rdbSaveLen(n / 2) then per pair rdbSaveRawString(member) and the score's 8 bytes
 *                   little-endian (rdbSaveBinaryDoubleValue :605-608), in the flat order, which is the
 *                   tail -> head order rdbSaveObject walks (:844-856)
 *   LIST_QUICKLIST  rdbSaveLen(nodes) then rdbSaveRawString(node ziplist) per node (:770-788); an
 *                   empty List is rdbSaveLen(0).  The nodes are the ones desList's quicklistPushTail
 *                   loop builds (rock_serdes.c:197-210, quicklist.c:503-520); list_compress_depth is
 *                   0, so no node is compressed.  An entry joins the tail node exactly when
 *                   _quicklistNodeAllowInsert (quicklist.c:420-450) says so:
 *                     sz      the pushed string's length (an INT descriptor: its decimal digits)
 *                     new_sz  (unsigned int) node->sz + sz + (sz < 254 ? 1 : 5)
 *                             + (sz < 64 ? 1 : sz < 16384 ? 2 : 5); node->sz the node's real
 *                             ziplist size
 *                     fill < 0: allowed when new_sz <= {4096, 8192, 16384, 32768, 65536}[-fill - 1]
 *                     fill >= 0: allowed when new_sz <= 8192 (SIZE_SAFETY_LIMIT) and count < fill
 *                     a new node always takes its first entry
 *                   Each node is a real ziplist (ziplist.c:743-839): u32 zlbytes | u32 zltail | u16
 *                   zllen | entries | 0xFF.  An entry is prevlen (1 byte, or 0xFE + u32 when the
 *                   entry before it is 254 bytes or more, :408-419) | encoding | body.  Strings:
 *                   len <= 63 one byte, <= 16383 0x40 | two bytes big-endian, else 0x80 + u32
 *                   big-endian (:332-364).  An entry that passes zipTryEncoding (:480-504: 1..31
 *                   bytes, string2ll) is an integer: 0..12 0xF1 + v; int8 0xFE; int16 0xC0; int24
 *                   0xF0; int32 0xD0; else 0xE0, little-endian (:507-534).  A STR descriptor whose
 *                   bytes pass zipTryEncoding is such an entry too, as it is after desList.
 *
 * LZF (rr_rdbsave_opts.flags & RR_RDBSAVE_LZF; the reference's default, config.c:2153
 * server.rdb_compression = 1).  Under `rdbcompression yes` rdbSaveRawString sends every string of
 * more than 20 bytes through rdbSaveLzfStringObject first (rdb.c:426-431, :348-364).  With the flag
 * the same happens at every rdbSaveRawString site whose bytes lie in the arena: the STR descriptor of
 * a RAW or EMBSTR String, SET_HT members, HASH_HT fields and values, ZSET_SKIPLIST members (not the
 * scores), the ZLRAW bytes of a HASH_ZIPLIST or ZSET_ZIPLIST.  The integer attempt comes first, as
 * without the flag; it applies to len <= 11 only, so the two never meet.  If len > 20 the string is
 * compressed, and if the stream has clen != 0 && clen <= len - 4 the string is written as
 *     0xC3 | rdbSaveLen(clen) | rdbSaveLen(len) | stream
 * (rdbSaveLzfBlob, rdb.c:323-346; 0xC3 = (RDB_ENCVAL << 6) | RDB_ENC_LZF), otherwise raw as above.
 *   The stream is what lzf_decompress (lzf_d.c:68-184) reads: a control byte c < 32 is followed by
 * c + 1 literal bytes; otherwise l = c >> 5, plus the next byte when l == 7, the offset is
 * ((c & 0x1f) << 8 | next byte) + 1, and l + 2 bytes are copied from op - offset one at a time
 * (overlap allowed).  So a match is 3..264 bytes at distance 1..8192 and a literal run 1..32 bytes.
 *   The contract is that of rr_lz4.h: a valid stream, deterministic, not the CPU compressor's bytes.
 * lzf_decompress(stream, clen, buf, len) returns len and gives the string back.  A string's stream
 * depends on its bytes and length only: not on its arena address or alignment, its output address,
 * its neighbours in the batch, the grid, or the run.  lzf_c.c's own bytes cannot be the goal: it
 * compresses over an uninitialised table (lzfP.h:95, INIT_HTAB 0), so they are not reproducible, and
 * its out-of-space tests (lzf_c.c:167-168, :259, :272) are conservative by a few bytes.  Which
 * strings take the LZF form may so differ from a given reference run; every loader takes either.
 * A string of 0x7FFFFFF0 bytes or more is written raw.
 *   These stay raw with the flag set: INT Strings (rdbSaveLongLongAsStringObject), the intset blob
 * and the quicklist nodes (both assembled by the kernels, not in the arena).
 *   The SAVE request of the pipe mode below keeps the default options, without LZF: carrying options
 * over the pipe needs a new entry point on the child's side, which is a change of its own.
 *
 * Deviations, all loadable by every RDB loader:
 *   - LZF: none without RR_RDBSAVE_LZF (the output is the reference's under `rdbcompression no`);
 *     with it, intset blobs and List nodes of more than 20 bytes stay raw where the reference
 *     would try LZF, and the streams are this library's, not lzf_c.c's;
 *   - SET_HT and HASH_HT are written in the flat form's order.  The reference writes dictNext order
 *     under a per-process random hash seed, so its order is not reproducible; any order loads to
 *     the same object.
 *
 * Unsaveable values follow rr_encode_batch's rule (rr_serdes.h, tests/encode_expect.py): status != 0,
 * descriptors or payload outside the caller's buffers, kinds that do not fit the type.  Such a value
 * has size 0, status[i] = RR_E_ENCODE, counts in rr_totals.n_bad and writes nothing.  A value whose
 * payload would end past out->data_cap gets RR_E_CAPACITY, counts in n_bad and writes nothing;
 * offsets[0..n] are complete whatever data_cap is.  Nothing outside [elems, elems + elem_cap) or
 * [arena, arena + arena_cap) is read.  rr_totals: n_elems the sum of every value's n_elems field,
 * bytes = offsets[n], payload the STR / ZLRAW bytes of the values written.
 */
#ifndef RR_RDBSAVE_H
#define RR_RDBSAVE_H

#include "rr_serdes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RR_RDBSAVE_DEFAULT_FILL (-2)   /* OBJ_LIST_MAX_ZIPLIST_SIZE, server.h */
#define RR_RDBSAVE_LZF 1u              /* rr_rdbsave_opts.flags: the LZF string form ("LZF" above) */

typedef struct rr_rdbsave_opts {
    int32_t list_fill;      /* list-max-ziplist-size; clamped to [-5, 32767] as quicklistSetFill
                               does for its 16-bit field (quicklist.c:117-124, quicklist.h:78) */
    uint32_t flags;         /* 0 or RR_RDBSAVE_LZF; any other bit: RR_API_EINVAL from both calls.
                               0 gives the bytes of opts == NULL but for list_fill */
} rr_rdbsave_opts;

/* Upper bound on the bytes of a batch of n values with n_elems descriptors whose STR / ZLRAW
 * lengths sum to payload_bytes: 17 * n + 26 * n_elems + payload_bytes, rounded up to 16.
 *   per value      at most 9 bytes of rdbSaveLen (a count, or the intset blob's length) and the
 *                  intset blob's 8-byte header: 17
 *   per descriptor a string costs at most 5 + len; an integer String at most 1 + 20 digits; a score
 *                  or an intset member 8.  A List entry is at most prevlen 5 + header 5 + len as a
 *                  string and prevlen 5 + 1 + 8 = 14 as an integer.  A node's rdbSaveLen (5) and
 *                  ziplist header and end byte (11) are charged to its first entry, whose prevlen
 *                  is always 1 byte: 16 + 1 + 5 + len = 22 + len as a string, 16 + 1 + 9 = 26 as
 *                  an integer; every later entry costs at most 10 + len or 14.  So 26 + len holds
 *                  for every entry
 * The bound holds with RR_RDBSAVE_LZF too: an LZF string costs 1 + rdbSaveLen(clen) +
 * rdbSaveLen(len) + clen <= 1 + 5 + 5 + (len - 4) = len + 7, within the 26 + len of its descriptor. */
uint64_t rr_rdbsave_bound(uint64_t n, uint64_t n_elems, uint64_t payload_bytes);

/* Device-resident: every pointer on ctx's device.  out->n == in->n; out->data 16-byte aligned;
 * writes out->offsets[0..n], out->data, types[0..n), status[0..n) and *d_totals.  opts may be NULL
 * (list_fill -2, flags 0).  Five launches on `stream` (sizes, scan, emit, two for the Lists), no host
 * synchronisation.  With RR_RDBSAVE_LZF the context's scratch also holds 4 bytes per descriptor
 * (in->elem_cap), so rr_ctx_reserve or a warm call comes before a graph capture, as for every call. */
int rr_rdbsave_batch(rr_ctx *ctx, const rr_flat_batch *in, rr_blob_batch *out, uint8_t *types,
                     uint8_t *status, rr_totals *d_totals, const rr_rdbsave_opts *opts, void *stream);

/* The same over host pointers, staged through the context's device buffers; blocks.  data receives
 * min(offsets[n], data_cap) bytes. */
int rr_rdbsave_batch_host(rr_ctx *ctx, const rr_value *values, const rr_elem *elems, uint64_t n_elems,
                          const uint8_t *arena, uint64_t arena_bytes, uint64_t n,
                          const rr_rdbsave_opts *opts, uint8_t *data, uint64_t data_cap,
                          uint64_t *offsets, uint8_t *types, uint8_t *status, rr_totals *totals);

/* ---- pipe mode: the child side of rr_rdb_serve's RR_RDB_SAVE_TAG request (rr_rdb.h) ---------
 * The request has the FLAT request's shape; the service multi-gets the keys, decodes them and
 * saves them with the default options on its context, and answers
 *   u64 n | u64 bytes | types[n] | status[n] | offsets[n + 1] | data[bytes]. */
typedef struct rr_rdbsave_result {
    uint64_t  n;
    uint64_t  bytes;        /* offsets[n] */
    uint8_t  *types;        /* n */
    uint8_t  *status;       /* n: 0, RR_E_ENCODE (the key's value did not decode) */
    uint64_t *offsets;      /* n + 1 */
    uint8_t  *data;         /* bytes */
} rr_rdbsave_result;

/* Ask for the payloads of k keys over the pipes, arguments as rr_rdb_request_flat's (rr_rdb.h).
 * RR_API_OK, or an error when the service went away (a missing key ends it, as in every mode);
 * *out is malloc'd and released with rr_rdbsave_result_free. */
int  rr_rdbsave_request(int fd_req, int fd_resp, const int *dbis, const char *const *keys,
                        const size_t *key_lens, size_t k, rr_rdbsave_result *out);
void rr_rdbsave_result_free(rr_rdbsave_result *r);

#ifdef __cplusplus
}
#endif
#endif
