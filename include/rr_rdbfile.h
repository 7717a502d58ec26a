/*
 * rr_rdbfile.h — complete RDB streams and DUMP payloads on the GPU, with their CRC-64: the framing
 * around the value payloads of rr_rdbsave.h, and the verifier in front of rr_rdbload.h.
 *
 * rr_rdbsave_batch writes what rdbSaveObject writes.  A snapshot (rdbSaveRio, rdb.c:1171-1262) is
 *     "REDIS0009" | aux fields | per db: SELECTDB, RESIZEDB, records | 0xFF | crc64, 8 bytes LE
 * where a record (rdbSaveKeyValuePair, rdb.c:1017-1073) is
 *     [0xFC | expire, 8 bytes little-endian]   when the key has an expire       (:1030-1034, :115-119)
 *     [0xF8 | rdbSaveLen(idle seconds)]        maxmemory-policy LRU             (:1037-1042)
 *     [0xF9 | freq byte]                       maxmemory-policy LFU             (:1045-1054)
 *     type | rdbSaveRawString(key) | payload                                    (:1057-1059)
 * and the checksum covers every byte before it (rioGenericUpdateChecksum; :1249-1255: the running
 * value is taken after the 0xFF and written little-endian; `rdbchecksum no` writes eight zero bytes).
 * A DUMP / MIGRATE payload (createDumpPayload, cluster.c:4817-4844) is
 *     type | payload | 0x09 0x00 (RDB_VERSION, little-endian) | crc64 of all of that, 8 bytes LE
 * and RESTORE (verifyDumpPayload, cluster.c:4850-4867) refuses fewer than 10 bytes, a footer version
 * above RDB_VERSION, and a CRC that does not match.
 *
 * Primitives
 *   rdbSaveLen (rdb.c:147-178): len < 64: one byte; len < 16384: 0x40 | len >> 8, len & 0xFF;
 *     len <= UINT32_MAX: 0x80 then u32 big-endian; else 0x81 then u64 big-endian (an idle time of
 *     2^32 seconds or more takes this 9-byte form).
 *   rdbSaveRawString (rdb.c:411-441), as rr_rdbsave.h states it: when len <= 11 and the bytes are the
 *     canonical decimal of a value in int32 range (rdbTryIntegerEncoding :307-321) the integer form
 *     0xC0 i8 | 0xC1 i16 | 0xC2 i32, little-endian (rdbEncodeInteger :241-261); otherwise
 *     rdbSaveLen(len) then the bytes.  Keys and aux fields are written this way.
 *   Opcodes (rdb.h:94-102): 0xFA AUX, 0xFB RESIZEDB, 0xFC EXPIRETIME_MS, 0xF8 IDLE, 0xF9 FREQ,
 *     0xFE SELECTDB, 0xFF EOF.
 *
 * The checksum is "Jones" CRC-64 (crc64.c:1-12): polynomial 0xad93d23594c935a9, reflected in and
 * out (the reflected constant is 0x95ac9329ac4bc9b5), initial value 0, no final xor;
 * crc64(0, "123456789") = 0xe9c6d914c4b8d9ca.  Every table here is generated from the polynomial.
 *   With init 0 and no xor-out it is linear over GF(2):
 *     crc(0, A || B) = shift(crc(0, A), |B|) ^ crc(0, B)        crc(c, B) = crc(0, B) ^ shift(c, |B|)
 *     shift(c, n) = c * x^(8n) mod P  (= crc(c, n zero bytes))
 *   so zero bytes in FRONT of a run with state 0 change nothing.  The kernels cut a stream into pieces
 *   of RR_CRC64_PIECE bytes counted from its END (only the first piece is short: it is a full piece
 *   with zero bytes in front), a piece into RR_CRC64_RUN bytes a lane; the incoming value goes into
 *   the state of the lane that owns the stream's first byte.  Every combine is then a multiplication
 *   by a constant x^(8k) mod P; no shift by a run-time length is needed.
 *
 * Deviations
 *   - keys are never LZF-compressed.  `rdbcompression yes` would try keys of more than 20 bytes;
 *     every loader takes either form (payloads take the LZF form under RR_RDBSAVE_LZF, rr_rdbsave.h);
 *   - rr_rdbdump_verify_batch refuses fewer than 11 bytes, not 10: the reference accepts 10 and then
 *     fails on the missing type byte;
 *   - a record or a DUMP value whose value is not saveable is skipped (status below), where the
 *     reference has no such value: it is the caller's CPU path's.
 */
#ifndef RR_RDBFILE_H
#define RR_RDBFILE_H

#include "rr_serdes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rr_rdbfile_section flags; any other bit: RR_API_EINVAL */
#define RR_RDBFILE_IDLE      1u   /* write 0xF8 | rdbSaveLen(idle[i]) */
#define RR_RDBFILE_FREQ      2u   /* write 0xF9 | freq[i] */
#define RR_RDBFILE_EOF       4u   /* end the section with 0xFF and the checksum */
#define RR_RDBFILE_NO_CKSUM  8u   /* rdbchecksum no: the state stays as it came in */

/* per-record / per-value status beside RR_OK and RR_E_CAPACITY (rr_format.h) */
#define RR_RDBFILE_E_VALUE    40   /* status[i] != 0 on entry, or the payload slice is reversed, past
                                      data_cap or 0x7FFFFFF0 bytes or more: the caller's CPU path's */
#define RR_RDBFILE_E_KEY      41   /* the key slice is reversed, past data_cap or 0x7FFFFFF0 bytes or more */
#define RR_RDBDUMP_E_SHORT    42   /* fewer than 11 bytes (or a slice that is reversed, past data_cap
                                      or 0x7FFFFFF0 bytes or more: nothing of it is read) */
#define RR_RDBDUMP_E_VERSION  43   /* footer version above 9 */
#define RR_RDBDUMP_E_CRC      44

#define RR_RDB_VERSION 9           /* rdb.h:41 */

/* The CRC kernels' shape (mirrored in the Python binding; the tests take their sizes from them):
 * a wave takes one piece a step, a lane one run of it; at most RR_CRC64_MAX_WAVES waves a launch,
 * so one grid stride of the stream pass is RR_CRC64_MAX_WAVES * RR_CRC64_PIECE bytes. */
#define RR_CRC64_RUN        256u
#define RR_CRC64_PIECE      (64u * RR_CRC64_RUN)
#define RR_CRC64_MAX_WAVES  2048u
/* rr_rdbdump_batch / rr_rdbdump_verify_batch: a wave a value, at most this many waves a launch */
#define RR_RDBDUMP_MAX_WAVES 16384u

typedef struct rr_rdbfile_in {
    rr_blob_batch  payloads;    /* rr_rdbsave_batch's out: data, offsets[n + 1], n, data_cap */
    rr_blob_batch  keys;        /* n slices; keys.n == payloads.n */
    const uint8_t *types;       /* n: rr_rdbsave_batch's types */
    const uint8_t *status;      /* n: rr_rdbsave_batch's status */
    const int64_t *expires;     /* n, milliseconds, -1: none; NULL: none for every key */
    const uint64_t *idle;       /* n, seconds; read under RR_RDBFILE_IDLE */
    const uint8_t *freq;        /* n; read under RR_RDBFILE_FREQ */
    const uint8_t *head;        /* head_bytes bytes copied in front of the first record (rr_rdbfile_head,
                                   rr_rdbfile_selectdb, or anything else: scripts, module aux) */
    uint64_t       head_bytes;
} rr_rdbfile_in;

typedef struct rr_rdbfile_result {
    uint64_t bytes;     /* the section's bytes (what d_state[1] holds); UINT64_MAX: device-side failure */
    uint64_t n_bad;     /* records / values with nonzero status */
    uint32_t status;    /* RR_OK, or RR_E_CAPACITY: the section does not fit out_cap, nothing written */
    uint32_t rsv;
} rr_rdbfile_result;

/* Upper bound on a section's bytes for n records whose keys hold key_bytes and whose payloads hold
 * payload_bytes in all: head_bytes + 27 * n + key_bytes + payload_bytes + 9, rounded up to 16.
 *   per record  0xFC and 8 bytes of expire: 9; 0xF8 and at most 9 bytes of rdbSaveLen: 10; 0xF9 and
 *               the freq byte: 2; the type byte: 1; the key's rdbSaveLen: at most 5 (a key is shorter
 *               than 2^31; the integer forms are shorter than rdbSaveLen + bytes): 27
 *   once        0xFF and the checksum: 9 */
uint64_t rr_rdbfile_bound(uint64_t n, uint64_t key_bytes, uint64_t payload_bytes, uint64_t head_bytes);

/* One section of a stream, device-resident: every pointer on ctx's device; out 16-byte aligned.
 * Writes out[0, section bytes): head, then for every key i in order the record above (types[i], key i
 * by rdbSaveRawString, payload i), then under RR_RDBFILE_EOF 0xFF and the checksum.
 *   rec_status[n]   0 written; RR_RDBFILE_E_VALUE; RR_RDBFILE_E_KEY.  Such a record has size 0 and
 *                   writes nothing.
 *   rec_offsets[n + 1]  the records' starts in the section (rec_offsets[0] == head_bytes,
 *                   rec_offsets[n] the end of the last record); complete whatever out_cap is.
 *   d_state, u64[2] [0] the running checksum: read on entry, replaced by the checksum of what came
 *                   before plus every byte this section writes in front of its checksum field (the head
 *                   and the 0xFF included), so sections of successive calls, concatenated, carry the
 *                   checksum of one rdbSaveRio run.  Under RR_RDBFILE_NO_CKSUM it stays as it came in,
 *                   and that value is what RR_RDBFILE_EOF writes (a caller who starts from 0 gets the
 *                   eight zero bytes of `rdbchecksum no`).  [1] receives the section's bytes.
 *   d_result        bytes, n_bad, status.
 * When the section would end past out_cap nothing of out is written, d_state[0] is unchanged,
 * d_state[1] and d_result->bytes hold the bytes needed and d_result->status is RR_E_CAPACITY.
 * Nothing outside the callers' slices is read.  Five launches on `stream` (sizes, scan, emit, the CRC
 * over the assembled section, its combine), no host synchronisation; scratch comes from the context,
 * so rr_ctx_reserve or a warm call comes before a graph capture, as for every call. */
int rr_rdbfile_section(rr_ctx *ctx, const rr_rdbfile_in *in, uint32_t flags, uint8_t *out, uint64_t out_cap,
                       uint64_t *rec_offsets, uint8_t *rec_status, uint64_t *d_state, rr_rdbfile_result *d_result,
                       void *stream);

/* The same over host pointers (every pointer of *in too), staged through the context's device
 * buffers; blocks.  out receives the section when it fits; state[2] is read and written. */
int rr_rdbfile_section_host(rr_ctx *ctx, const rr_rdbfile_in *in, uint32_t flags, uint8_t *out, uint64_t out_cap,
                            uint64_t *rec_offsets, uint8_t *rec_status, uint64_t *state, rr_rdbfile_result *result);

/* d_state[0] = crc64(d_state[0], data[0, bytes)) on the device (the section's CRC pass alone: two
 * launches); d_state[1] = bytes. */
int rr_crc64_device(rr_ctx *ctx, const uint8_t *data, uint64_t bytes, uint64_t *d_state, void *stream);

/* DUMP payloads.  in / types / status: rr_rdbsave_batch's outputs.  Value i of out is
 * types[i] | payload i | 0x09 0x00 | crc64 of all of that, little-endian: payload + 11 bytes.
 * out_status[i]: 0; RR_RDBFILE_E_VALUE (size 0, nothing written); RR_E_CAPACITY for a value that would
 * end past out->data_cap (rr_rdbsave_batch's rule: it writes nothing, out->offsets[0..n] are complete).
 * d_result: bytes = out->offsets[n], n_bad.  A wave a value; three launches (sizes, scan, emit). */
int rr_rdbdump_batch(rr_ctx *ctx, const rr_blob_batch *in, const uint8_t *types, const uint8_t *status,
                     rr_blob_batch *out, uint8_t *out_status, rr_rdbfile_result *d_result, void *stream);
int rr_rdbdump_batch_host(rr_ctx *ctx, const uint8_t *data, const uint64_t *offsets, const uint8_t *types,
                          const uint8_t *status, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                          uint8_t *out_status, rr_rdbfile_result *result);

/* verifyDumpPayload for a batch, and the payloads compacted into rr_rdbload_batch's input shape.
 * status[i]: 0; RR_RDBDUMP_E_SHORT; RR_RDBDUMP_E_VERSION; RR_RDBDUMP_E_CRC (checked in this order, as
 * the reference does); RR_E_CAPACITY.  For status 0 types[i] is the value's first byte and
 * out[offsets[i], offsets[i + 1]) its payload; every other value has size 0 (types[i] is then its
 * first byte when it has one, else 0).  out->offsets[0..n] are complete whatever data_cap is; out->data
 * may be NULL when data_cap is 0.  Three launches (check, scan, copy). */
int rr_rdbdump_verify_batch(rr_ctx *ctx, const rr_blob_batch *in, rr_blob_batch *out, uint8_t *types,
                            uint8_t *status, rr_rdbfile_result *d_result, void *stream);
int rr_rdbdump_verify_batch_host(rr_ctx *ctx, const uint8_t *data, const uint64_t *offsets, uint64_t n, uint8_t *out,
                                 uint64_t out_cap, uint64_t *out_offsets, uint8_t *types, uint8_t *status,
                                 rr_rdbfile_result *result);

/* ---- host helpers, no GPU ------------------------------------------------------------------- */
typedef struct rr_rdbfile_repl {
    int32_t     stream_db;      /* repl-stream-db */
    const char *replid;         /* repl-id, NUL-terminated (40 characters in the reference) */
    int64_t     offset;         /* repl-offset */
} rr_rdbfile_repl;

/* "REDIS0009" and rdbSaveInfoAuxFields (rdb.c:1101-1122), each field 0xFA | rdbSaveRawString(name) |
 * rdbSaveRawString(value), integers as their decimal text first (rdbSaveAuxFieldStrInt :1093-1098:
 * so redis-bits 64 is C0 40): redis-ver, redis-bits (64), ctime, used-mem, then with repl != NULL
 * repl-stream-db, repl-id, repl-offset, then aof-preamble.  Returns the bytes needed and writes
 * only when they fit cap. */
uint64_t rr_rdbfile_head(uint8_t *buf, uint64_t cap, const char *ver, int64_t ctime, uint64_t used_mem,
                         const rr_rdbfile_repl *repl, int aof_preamble);
/* 0xFE rdbSaveLen(dbid) | 0xFB rdbSaveLen(db_size) rdbSaveLen(expires_size) (rdb.c:1193-1205), the
 * sizes trimmed to UINT32_MAX as there.  Returns the bytes needed; writes only when they fit. */
uint64_t rr_rdbfile_selectdb(uint8_t *buf, uint64_t cap, uint64_t dbid, uint64_t db_size, uint64_t expires_size);
/* crc64.c's crc64() over tables generated from the polynomial at first use (slice-by-8) */
uint64_t rr_crc64(uint64_t crc, const void *ptr, uint64_t len);
/* shift(c, n) = c * x^(8n) mod P, and the product of two residues (in the reflected bit order) */
uint64_t rr_crc64_shift(uint64_t crc, uint64_t n);
uint64_t rr_crc64_mul(uint64_t a, uint64_t b);

#ifdef __cplusplus
}
#endif
#endif
