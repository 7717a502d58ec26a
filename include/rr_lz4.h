/*
 * rr_lz4.h — GPU LZ4 block compression of RocksDB data blocks, beside rr_snappy.h (SURVEY.md
 * §8f row f3).
 *
 * The reference's store setup names two compressors: kSnappyCompression and, commented out one
 * line above it, kLZ4Compression (rocksdbapi.cc:159-160); it vendors LZ4 1.9.2 (deps/lz4).  A
 * compressed block here is what RocksDB's LZ4_Compress writes at compress_format_version 2 and
 * LZ4_Uncompress reads:
 *
 *   varint32 N (the uncompressed length), then one raw LZ4 block of N bytes
 *   (deps/lz4/doc/lz4_Block_format.md; deps/lz4/lib/lz4.c).
 *
 * RocksDB's source is not in the reference tree (deps/rocksdb is an empty submodule): this framing
 * is restated from RocksDB's documentation and is not pinned by a file here.  The varint32 is read
 * by the rule of the snappy preamble (at most 5 bytes, the 5th below 16).
 *
 * Compression.  LZ4 has no canonical encoder: rr_lz4_compress_batch writes a valid block (the
 * rule below accepts it, and so does every LZ4 decoder), not the bytes of any CPU LZ4.  The same
 * input gives the same bytes on every run and at every batch position.  The last 5 bytes of a
 * block are literals and the last match starts at least 12 bytes before the end
 * (lz4_Block_format.md "End of block restrictions"); a block of fewer than 13 bytes is one
 * literal run.
 *
 * Decompression: the acceptance rule.  A block with announced length N is accepted exactly when
 * LZ4_decompress_safe of 1.9.2 (lz4.c:2078; LZ4_decompress_generic with endOnInputSize, full
 * block, noDict, lz4.c:1658-2072), given a destination of exactly N bytes, returns N; the engine
 * then writes those N bytes.  With S the raw block's size, ip / op the input / output positions:
 *
 *   - N == 0: accepted only when the block is the single byte 00 (lz4.c:1701-1705);
 *     S == 0 is rejected (lz4.c:1707).
 *   - A sequence is token, literal length (token >> 4, 15: extended by bytes added up while they
 *     are 255), the literals, a 2-byte little-endian offset, match length (token & 15, 15:
 *     extended the same way, then + 4).
 *   - Literal-length extension: rejected when the first extension byte would be at or past
 *     S - 15 (read_variable_length's initial check, lz4.c:1634, lencheck lz4.c:1898); the sum
 *     stops, without an error, after the byte that reaches S - 15 (lz4.c:1642, 1899).
 *   - Match-length extension: rejected when an extension byte is read at or past S - 5, that is
 *     once ip reaches S - 4 after it (lz4.c:1972-1973).
 *   - A literal run that ends within 12 bytes of the output's end (op + len > N - 12) or within 8
 *     of the input's end (ip + len > S - 8) must be the last one: it must end exactly at the
 *     input's end and not past the output's (lz4.c:1910, 1945); the block ends there.
 *   - The shortcut (lz4.c:1863-1888): a literal length below 15 whose token has more than 16
 *     bytes after it (ip < S - 16), with op <= N - 32, skips the two end tests of the previous
 *     point; if the match length is also below 15, the offset at least 8 and inside the output,
 *     the match is copied without the test of the next point (it cannot pass N).
 *   - A match may not end within the last 5 output bytes (op + len > N - 5, lz4.c:2047).
 *   - An offset may not reach before the output's start (lz4.c:1981).
 *   While N - op >= 64 LZ4 runs its fast loop (lz4.c:1711-1843), which gives the same verdicts as
 *   the rules above with the shortcut's input-side exception (ip <= S - 17, lz4.c:1751) and leaves
 *   it for good at the first sequence that comes within 64 bytes of the output's end.
 *
 * Two deviations, both stricter:
 *   - offset 0: 1.9.2 does not check it and copies garbage; the engine returns RR_LZ4_E_OFFSET;
 *   - early end: a block that ends cleanly after fewer than N bytes makes LZ4 return a smaller
 *     count; the engine returns RR_LZ4_E_LENGTH.
 *
 * Whatever the verdict, a block's writes stay inside its own [out->offsets[i], out->offsets[i+1]).
 *
 * Conventions as rr_snappy.h: device pointers, the caller's stream, no host synchronisation in
 * the device entry points (a context's scratch grows between calls, not under capture).
 */
#ifndef RR_LZ4_H
#define RR_LZ4_H

#include <stdint.h>
#include "rr_serdes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-block decompression status (0 = OK), parallel to RR_SNAPPY_* */
#define RR_LZ4_OK          0
#define RR_LZ4_E_HEADER    1   /* bad varint32 length preamble */
#define RR_LZ4_E_TRUNC     2   /* the block ends inside a sequence, or a run that must be the last one is not */
#define RR_LZ4_E_OFFSET    3   /* match offset 0 or before the start of the output */
#define RR_LZ4_E_OVERFLOW  4   /* output past N, or a match / non-final run inside the protected end of the output */
#define RR_LZ4_E_LENGTH    5   /* the block ends cleanly with less output than the preamble announced */
#define RR_LZ4_E_CAPACITY  6   /* the block's output does not fit out->data_cap (batch API only) */

/* 5 + n + n / 255 + 16: the varint32 plus LZ4_COMPRESSBOUND (lz4.h) */
uint64_t rr_lz4_max_compressed_length(uint64_t n);
/* out->data_cap rr_lz4_compress_batch needs for n_blocks blocks of data_bytes in all: the sum of
 * the per-block bounds can not exceed 21 n_blocks + data_bytes + data_bytes / 255 (+ 16) */
uint64_t rr_lz4_compress_bound(uint64_t n_blocks, uint64_t data_bytes);

/* Both directions: in->data 16-byte aligned, in->data_cap a multiple of 16 covering every block.
 * Compress in's n blocks into out->data, packed: block i's compressed bytes at
 * [out->offsets[i], out->offsets[i+1]).  out->data_cap must be at least
 * rr_lz4_compress_bound(n, in->data_cap).  The context's scratch holds per-block output slots. */
int rr_lz4_compress_batch(rr_ctx *ctx, const rr_blob_batch *in, rr_blob_batch *out, void *stream);

/* Decompress in's n blocks into out->data, packed in block order by the lengths their preambles
 * announce (out->offsets[n+1] written by the call); status[i] (device, n bytes) is RR_LZ4_OK or
 * an RR_LZ4_E_* code, and a failed block's output bytes are unspecified (inside its own range).
 * out->data_cap bounds the output: a block past it gets RR_LZ4_E_CAPACITY and writes nothing. */
int rr_lz4_decompress_batch(rr_ctx *ctx, const rr_blob_batch *in, rr_blob_batch *out, uint8_t *status,
                            void *stream);

/* Host-pointer forms (stage through the context's device buffers; synchronous).
 * compress: out_cap >= rr_lz4_compress_bound(n, offsets[n]); out_offsets[n+1] written.
 * decompress: out_offsets[n+1] and status[n] written; returns RR_API_EINVAL if out_cap is
 * smaller than the sum of the announced lengths (nothing is decompressed then). */
int rr_lz4_compress_batch_host(rr_ctx *ctx, const uint8_t *data, const uint64_t *offsets, uint64_t n,
                               uint8_t *out, uint64_t out_cap, uint64_t *out_offsets);
int rr_lz4_decompress_batch_host(rr_ctx *ctx, const uint8_t *data, const uint64_t *offsets, uint64_t n,
                                 uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, uint8_t *status);

#ifdef __cplusplus
}
#endif
#endif
