/*
 * rr_rdbread.h — reading a complete RDB stream (a dump.rdb, a full-sync payload): the load side of
 * rr_rdbfile.h.  The host walks the framing and finds every record's extent; the GPU checks the
 * CRC-64 of the whole stream, decodes each record's prefix opcodes and key, and compacts the value
 * payloads into the input shape of rr_rdbload_batch (rr_rdbload.h) and rr_rdbconvert_batch.
 *
 * The rule is rdbLoadRio's (rdb.c:2044-2312):
 *   "REDIS" and four digits; a signature other than REDIS or a version below 1 or above 9 ends the
 *   load (:2052-2064).  Then a loop over one-byte opcodes (:2072-2242):
 *     0xFD EXPIRETIME     4 bytes little-endian, a signed 32-bit number of seconds, times 1000 (:2079-2086)
 *     0xFC EXPIRETIME_MS  8 bytes little-endian, signed (:2087-2092)
 *     0xF9 FREQ           one byte (:2093-2098)
 *     0xF8 IDLE           rdbLoadLen (:2099-2104)
 *       these four belong to the key that follows; a repeated one overwrites the earlier one
 *     0xFF EOF            the loop ends (:2105-2107)
 *     0xFE SELECTDB       rdbLoadLen: the db of the keys that follow (:2108-2119)
 *     0xFB RESIZEDB       two rdbLoadLen (:2120-2130)
 *     0xFA AUX            two strings (:2131-2190)
 *     0xF7 MODULE_AUX     (:2191-2230) not taken here
 *     anything else       the value's type: a key string, then the value (:2231-2242, rdbLoadObject)
 *   and behind the 0xFF, from version 5 on, the CRC-64 of every byte in front of it, 8 bytes
 *   little-endian; a stored 0 means "saved with checksum disabled" and is not compared (:2298-2311).
 * A string is rdbGenericLoadStringObject's (:487-540): rdbLoadLen, then the bytes; or 0xC0 / 0xC1 /
 * 0xC2 and a 1 / 2 / 4 byte little-endian integer that loads as its decimal text (ll2string); or 0xC3,
 * the compressed length, the length, and an LZF stream (rr_rdbload.h states the LZF rule).
 * rdbLoadLen (:190-234): 00xxxxxx; 01xxxxxx and a byte; 0x80 and 4 bytes big-endian; 0x81 and 8 bytes
 * big-endian; 11xxxxxx the encoded form.  Where a plain number is wanted (a count, a db id, an idle
 * time) the encoded form is taken as its low six bits, as rr_rdbload.h states.
 *
 * The division.  Finding where a record ends is a serial chain of length reads and skips: the host
 * does it (rr_rdbread_index), from cache, and decodes nothing.  Everything else is per-byte or
 * per-record work over bytes the loader needs in device memory anyway: the checksum
 * (rr_rdbread_verify), the prefix opcodes, the key with its integer and LZF forms, and the
 * compaction of the payloads (rr_rdbread_split).
 *
 * Deviations
 *   - the index finds a value's end by lengths only; nothing is decompressed or validated, so a value
 *     whose inner lengths lie ends where they say, and rr_rdbload_batch then refuses its content;
 *   - types 6, 7 (modules), 15 (streams), 0xF7 and every unknown type byte stop the index: their
 *     extent cannot be found by lengths alone;
 *   - a stream is read on a little-endian host and device; the version changes nothing else here
 *     (rdbLoadMillisecondTime's version test only matters on a big-endian machine);
 *   - an LZF key is refused unless its stream decompresses to exactly its stated length;
 *   - a record that the buffer holds only in part is walked again from its start on the next call.
 */
#ifndef RR_RDBREAD_H
#define RR_RDBREAD_H

#include "rr_rdbfile.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rr_rdbread_index and rr_rdbread_string return one of these */
#define RR_RDBREAD_DONE           0   /* the 0xFF was reached (and, from version 5 on, its 8 checksum bytes are there) */
#define RR_RDBREAD_MORE           1   /* the buffer ends inside the header, an item or a record */
#define RR_RDBREAD_FULL           2   /* max_recs or max_items reached */
/* per-record status of rr_rdbread_split beside RR_OK and RR_E_CAPACITY (rr_format.h); the numbering
 * continues rr_rdbfile.h's (45 is rr_rdbconvert.h's) */
#define RR_RDBREAD_E_SLICE       46   /* the record slice is reversed, past data_cap or 0x7FFFFFF0 bytes or more */
#define RR_RDBREAD_E_TRUNC       47   /* the prefix, the type or the key runs past rec_end */
#define RR_RDBREAD_E_OPCODE      48   /* 0xF7, 0xFA, 0xFB, 0xFE or 0xFF where the type is expected, or an IDLE
                                         length of unknown form */
#define RR_RDBREAD_E_KEY         49   /* the key has an unknown string encoding, or its LZF stream does not
                                         decompress to exactly its length */
/* rr_rdbread_verify's verdict beside RR_OK and RR_RDBDUMP_E_CRC */
#define RR_RDBREAD_NO_CKSUM      50   /* the stored checksum is 0: saved with checksum disabled (:2304) */
/* errors of rr_rdbread_index and rr_rdbread_string */
#define RR_RDBREAD_E_MAGIC       51   /* the first five bytes are not "REDIS" */
#define RR_RDBREAD_E_VERSION     52   /* the four digits are not a number from 1 to 9 */
#define RR_RDBREAD_E_UNSUPPORTED 53   /* a module or stream value, 0xF7, or an unknown type byte */
#define RR_RDBREAD_E_LEN         54   /* an unknown length or string-encoding byte */

/* rr_rdbread_split's shape (mirrored in the Python binding; the tests take their sizes from it): a
 * wave a record, at most RR_RDBREAD_MAX_WAVES waves a launch; a payload is copied 16 bytes a lane,
 * RR_RDBREAD_WAVE_STEP bytes a wave and step. */
#define RR_RDBREAD_MAX_WAVES   16384u
#define RR_RDBREAD_LANE_BYTES  16u
#define RR_RDBREAD_WAVE_STEP   (64u * RR_RDBREAD_LANE_BYTES)

/* ---- the record index: host, no GPU ----------------------------------------------------------- */
typedef struct rr_rdbread_state {
    uint32_t version;   /* 0: the header has not been read yet; else 1..9 */
    uint32_t rsv;
    uint64_t db;        /* the db of the next record (the last SELECTDB) */
    uint64_t pos;       /* where the walk goes on, an offset into buf */
} rr_rdbread_state;     /* zeroed before the first call */

typedef struct rr_rdbread_item {
    uint32_t opcode;    /* 0xFA, 0xFE or 0xFB */
    uint32_t rsv;
    uint64_t at, end;   /* [at, end) in buf; at is the opcode byte */
} rr_rdbread_item;

typedef struct rr_rdbread_index_result {
    uint64_t n_recs, n_items;   /* reported by this call */
    uint64_t eof_at;            /* RR_RDBREAD_DONE: the offset of the 0xFF */
    uint64_t cksum;             /* RR_RDBREAD_DONE with has_cksum: the 8 bytes behind it, little-endian */
    uint64_t err_at;            /* an error: where the item or the record (its first prefix opcode) starts */
    uint32_t has_cksum;         /* RR_RDBREAD_DONE: version >= 5 (:2298) */
    uint32_t rsv;
} rr_rdbread_index_result;

/* Walks buf[st->pos, bytes).  Every offset reported is relative to buf.
 *   A record is  prefix | type | key string | value, and starts at the first of its 0xFD / 0xFC / 0xF8 /
 *   0xF9 opcodes, or at its type byte when it has none: rec_start[i], rec_end[i], rec_db[i].  The
 *   value's end is found by lengths only:
 *     types 0, 11, 12, 13, 9, 10   one string
 *     types 2, 14, 1               a count, then count strings
 *     type 4                       a count, then 2 * count strings
 *     type 5                       a count, then count x (string, 8 bytes)
 *     type 3                       a count, then count x (string, an old-style double: one length byte,
 *                                  then that many bytes unless the byte is 253, 254 or 255; rdb.c:583-598)
 *   A string is skipped by its rdbLoadLen: the integer forms are 1, 2 or 4 bytes, the LZF form is its
 *   compressed length behind its two lengths.  The legacy types 1, 3, 9 and 10 are indexed
 *   (rr_rdbload_batch answers RR_RDBLOAD_E_TYPE for them).
 *   Each 0xFA, 0xFE and 0xFB is reported as an item; 0xFE also sets st->db.
 * Returns
 *   RR_RDBREAD_DONE   at the 0xFF: res->eof_at, res->has_cksum, res->cksum; st->pos is behind the
 *                     checksum (behind the 0xFF before version 5).
 *   RR_RDBREAD_MORE   the buffer ends inside the header, an item, a record or the checksum; st->pos is
 *                     where that one starts.  The caller keeps the bytes from there, appends more and
 *                     calls again (with st->pos set to where those bytes now are in its buffer).  A
 *                     caller who knows the stream is complete treats it as truncation.  A declared
 *                     length larger than what is left gives this, never a read past bytes: every
 *                     comparison is made against the bytes that remain, so no length or count wraps.
 *   RR_RDBREAD_FULL   the next one is a record and max_recs are reported, or an item and max_items
 *                     are; st->pos is behind the last one reported.
 *   RR_RDBREAD_E_MAGIC, RR_RDBREAD_E_VERSION   the header (st->version stays 0).
 *   RR_RDBREAD_E_UNSUPPORTED, RR_RDBREAD_E_LEN   res->err_at and st->pos are the start of the record or
 *                     item that holds the byte; everything reported before it stays valid.
 *   RR_API_EINVAL     a NULL argument, st->pos past bytes.
 * Reads buf[st->pos, bytes) only; no GPU, no allocation. */
int rr_rdbread_index(rr_rdbread_state *st, const uint8_t *buf, uint64_t bytes, uint64_t *rec_start, uint64_t *rec_end,
                     uint64_t *rec_db, uint64_t max_recs, rr_rdbread_item *items, uint64_t max_items,
                     rr_rdbread_index_result *res);

/* One string at buf[at] on the host, in its plain, integer (as decimal text) or LZF form: *len its
 * loaded length, *end the offset behind it, out[0, *len) its bytes when *len <= out_cap (out may be
 * NULL with out_cap 0: the length alone).  The AUX items' fields are read with it.
 * Returns RR_RDBREAD_DONE; RR_E_CAPACITY (*len and *end set, nothing written); RR_RDBREAD_MORE (the
 * string runs past bytes); RR_RDBREAD_E_LEN; RR_RDBREAD_E_KEY (an LZF stream that does not decompress
 * to exactly its length); RR_API_EINVAL. */
int rr_rdbread_string(const uint8_t *buf, uint64_t bytes, uint64_t at, uint8_t *out, uint64_t out_cap, uint64_t *len,
                      uint64_t *end);
/* One rdbLoadLen number at buf[at] (SELECTDB's db id, RESIZEDB's two sizes; the encoded form is its
 * low six bits).  Returns RR_RDBREAD_DONE, RR_RDBREAD_MORE, RR_RDBREAD_E_LEN or RR_API_EINVAL. */
int rr_rdbread_len(const uint8_t *buf, uint64_t bytes, uint64_t at, uint64_t *val, uint64_t *end);

#ifndef RR_RDBREAD_HOST_ONLY
/* ---- the split: GPU ------------------------------------------------------------------------------ */
typedef struct rr_rdbread_out {
    rr_blob_batch keys;       /* n compacted key slices: the integer forms as ll2string text, LZF keys
                                 decompressed.  data may be NULL when data_cap is 0 */
    rr_blob_batch payloads;   /* n contiguous slices, [end of key, rec_end) as it is: what
                                 rr_rdbload_batch takes.  data may be NULL when data_cap is 0 */
    uint8_t  *types;          /* n */
    int64_t  *expires;        /* n: milliseconds, -1: none */
    uint64_t *idle;           /* n: seconds, UINT64_MAX: none */
    int16_t  *freq;           /* n: 0..255, -1: none */
    uint8_t  *status;         /* n */
} rr_rdbread_out;

/* Device-resident: every pointer on ctx's device.  data[0, data_cap) holds the stream (or the part of
 * it the records lie in), rec_start[n] / rec_end[n] are rr_rdbread_index's, version the stream's
 * (1..9, else RR_API_EINVAL); out->keys.n == out->payloads.n == n.
 *   status[i]  RR_OK; RR_RDBREAD_E_SLICE (nothing of the record is read); RR_RDBREAD_E_TRUNC;
 *              RR_RDBREAD_E_OPCODE; RR_RDBREAD_E_KEY; RR_E_CAPACITY: the key would end past
 *              keys.data_cap or the payload past payloads.data_cap.
 *   A record with nonzero status writes nothing to keys.data and payloads.data; but for
 *   RR_E_CAPACITY its key and payload have size 0, types[i] is 0, expires[i] -1, idle[i] UINT64_MAX,
 *   freq[i] -1.  Both offsets[0..n] are complete whatever the capacities are (a call with data_cap 0
 *   sizes the buffers: LZF keys need that).
 *   d_result   bytes = payloads.offsets[n]; n_bad; status RR_E_CAPACITY when keys.offsets[n] >
 *              keys.data_cap or payloads.offsets[n] > payloads.data_cap, else RR_OK.
 * Nothing outside [rec_start[i], rec_end[i]) is read for record i.  Three launches on `stream`
 * (sizes, one scan over both size arrays, emit), no host synchronisation; scratch comes from the
 * context, so rr_ctx_reserve or a warm call comes before a graph capture, as for every call. */
int rr_rdbread_split(rr_ctx *ctx, const uint8_t *data, uint64_t data_cap, const uint64_t *rec_start, const uint64_t *rec_end,
                     uint64_t n, uint32_t version, rr_rdbread_out *out, rr_rdbfile_result *d_result, void *stream);

/* The same over host pointers (every pointer of *out too), staged through the context's device
 * buffers; blocks.  data[0, data_cap) is uploaded whole. */
int rr_rdbread_split_host(rr_ctx *ctx, const uint8_t *data, uint64_t data_cap, const uint64_t *rec_start,
                          const uint64_t *rec_end, uint64_t n, uint32_t version, rr_rdbread_out *out,
                          rr_rdbfile_result *result);

/* The checksum's verdict, device-resident.  d_state[0] = crc64(d_state[0], data[0, eof_at + 1)) by
 * rr_crc64_device's two kernels (a stream uploaded in pieces chains through d_state, as
 * rr_rdbfile_section's sections do: earlier pieces go through rr_crc64_device, the last one, whose
 * data[eof_at] is the 0xFF, through this call); d_state[1] = eof_at + 1.  Then one small kernel
 * compares it with the 8 little-endian bytes data[eof_at + 1, eof_at + 9) (data_cap >= eof_at + 9,
 * else RR_API_EINVAL) and writes d_result: status RR_OK for a match, RR_RDBDUMP_E_CRC for a mismatch,
 * RR_RDBREAD_NO_CKSUM when the stored value is 0; bytes = eof_at + 9; n_bad 0 or 1 (a mismatch).
 * Three launches, no host synchronisation. */
int rr_rdbread_verify(rr_ctx *ctx, const uint8_t *data, uint64_t data_cap, uint64_t eof_at, uint64_t *d_state,
                      rr_rdbfile_result *d_result, void *stream);
/* The same over host pointers; state[2] is read and written; blocks. */
int rr_rdbread_verify_host(rr_ctx *ctx, const uint8_t *data, uint64_t data_cap, uint64_t eof_at, uint64_t *state,
                           rr_rdbfile_result *result);
#endif /* RR_RDBREAD_HOST_ONLY */

#ifdef __cplusplus
}
#endif
#endif
