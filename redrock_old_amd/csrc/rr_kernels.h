/* rr_kernels.h — the launch header of every kernel unit: the entry points the C host layer
 * (rr_api.c and the *_api.c files) calls, grouped by the .hip file that defines them. */
#ifndef RR_KERNELS_H
#define RR_KERNELS_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/rr_format.h"
#include "../../include/rr_serdes.h"

/* scratch layout (uint64 words): [0] tile counter, [1] done counter, [2] byte total,
 * [8 .. 8+64) 16 shards x {bad, payload, elems, -}, then one look-back word per tile
 * (decode: per byte window, followed by the u32 first-value table of the windows). */
#define RR_SCRATCH_HDR 72

#ifdef __cplusplus
extern "C" {
#endif

/* rr_kernels.hip, the decode (include/rr_serdes.h) */
/* sums: rr_decode_sums_words(data_cap) words, zero on entry (count_kernel adds the window and
 * group sums into them, decode_kernel reads them; a batch of one window generation runs
 * decode_kernel's one-launch form alone, which keeps its look-back and end words there and leaves
 * them zero); zero / nzero: words the call zeroes on the way (the other half of the context's
 * double buffer).  first_only (test hooks): 1 launch only count_kernel (the two-launch form);
 * 2 the one-launch form sums every earlier window itself (its look-back's help path).
 * flags: RR_CTX_ZL_RAW (rr_serdes.h), a kernel argument of every decode kernel. */
hipError_t rr_launch_decode(const uint8_t *blob, const uint64_t *offsets, uint64_t n, rr_value *values,
                            rr_elem *elems, uint64_t elem_cap, uint8_t *arena, uint64_t *scratch, uint64_t *sums,
                            uint64_t *zero, uint64_t nzero, uint64_t data_cap, rr_totals *totals, hipStream_t stream,
                            int first_only, unsigned flags);
uint64_t rr_decode_sums_words(uint64_t data_cap);
uint64_t rr_decode_scratch_words(uint64_t data_cap, uint64_t n);
/* small batches (one workgroup, one launch; the encode's likewise): whether a batch qualifies, and
 * the launch; a non-NULL done (host-mapped) receives seq once every result is visible to the host */
int rr_small_decode_fits(uint64_t n, uint64_t data_cap);
hipError_t rr_launch_decode_small(const uint8_t *blob, const uint64_t *offsets, uint64_t n, rr_value *values,
                                  rr_elem *elems, uint64_t elem_cap, uint8_t *arena, uint64_t data_cap, rr_totals *totals,
                                  uint32_t *done, uint32_t seq, unsigned flags, hipStream_t stream);
/* rr_kernels.hip, the encode (include/rr_serdes.h) */
hipError_t rr_launch_encode(const rr_value *values, const rr_elem *elems, uint64_t elem_cap, const uint8_t *arena,
                            uint64_t arena_cap, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *offsets,
                            uint64_t *scratch, uint64_t *sums, rr_totals *totals, hipStream_t stream, int first_only);
uint64_t rr_encode_sums_words(uint64_t n);
uint64_t rr_encode_scratch_words(uint64_t n, uint64_t data_cap);
int rr_small_encode_fits(uint64_t n, uint64_t data_cap);
hipError_t rr_launch_encode_small(const rr_value *values, const rr_elem *elems, uint64_t elem_cap, const uint8_t *arena,
                                  uint64_t arena_cap, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *offsets,
                                  rr_totals *totals, uint32_t *done, uint32_t seq, hipStream_t stream);
/* the pipelined host encode: the end of the arena bytes the valid values [0, n) read, as
 * RR_NEED_BLOCKS partial maxima into mapped host words */
#define RR_NEED_BLOCKS 32
hipError_t rr_launch_arena_need(const rr_value *values, uint64_t n, const rr_elem *elems, uint64_t elem_cap,
                                uint64_t arena_cap, uint64_t *need, hipStream_t stream);
/* rr_util.hip: zeroing, the look-back scan, the shard helpers of rr_shard.c, the copy kernel */
hipError_t rr_launch_zero_words(uint64_t *words, uint64_t n, hipStream_t stream);
uint64_t rr_scan_words(uint64_t n);
hipError_t rr_launch_scan_u64(uint64_t *x, uint64_t n, uint64_t *lb, uint64_t *err, hipStream_t stream);
hipError_t rr_launch_shard_plan(const uint64_t *offsets, uint64_t n, uint32_t g, uint64_t *plan, hipStream_t stream);
hipError_t rr_launch_offsets_rebase(uint64_t *offs, uint64_t count, uint64_t sub, hipStream_t stream);
hipError_t rr_launch_flat_rebase(rr_value *values, uint64_t n, rr_elem *elems, uint64_t ne, uint64_t elem_add,
                                 uint64_t byte_add, hipStream_t stream);
hipError_t rr_launch_copy(uint8_t *dst, const uint8_t *src, uint64_t bytes, hipStream_t stream);
hipError_t rr_launch_copy_shape(uint8_t *dst, const uint8_t *src, uint64_t bytes, int shape, hipStream_t stream);
/* rr_snappy.hip (include/rr_snappy.h) */
uint64_t rr_snappy_scratch_words(uint64_t n, uint64_t slot_bytes);
hipError_t rr_launch_snappy_decompress(const uint8_t *in, uint64_t in_cap, const uint64_t *in_offs, uint64_t n, uint8_t *out,
                                       uint64_t out_cap, uint64_t *out_offs, uint8_t *status, uint64_t *scratch,
                                       hipStream_t stream);
hipError_t rr_launch_snappy_compress(const uint8_t *in, uint64_t in_cap, const uint64_t *in_offs, uint64_t n, uint8_t *out,
                                     uint64_t *out_offs, uint64_t *scratch, uint64_t slot_bytes, hipStream_t stream);
/* shared by the snappy and LZ4 codecs (rr_snappy.hip): the varint32 length preambles of n blocks
 * (out_offs[i] the announced length, out_offs[n] = 0, status[i] 0 or 1 = E_HEADER, lb[0, lbw)
 * zeroed for the scan that follows), and the per-block slots -> packed output copy */
hipError_t rr_launch_varint_lengths(const uint8_t *in, const uint64_t *in_offs, uint64_t n, uint64_t *out_offs,
                                    uint8_t *status, uint64_t *lb, uint64_t lbw, hipStream_t stream);
hipError_t rr_launch_slot_pack(const uint8_t *slots, const uint64_t *slot_offs, uint64_t n, uint8_t *out,
                               const uint64_t *out_offs, hipStream_t stream);
/* rr_lz4.hip (include/rr_lz4.h) */
uint64_t rr_lz4_scratch_words(uint64_t n, uint64_t slot_bytes);
hipError_t rr_launch_lz4_decompress(const uint8_t *in, uint64_t in_cap, const uint64_t *in_offs, uint64_t n, uint8_t *out,
                                    uint64_t out_cap, uint64_t *out_offs, uint8_t *status, uint64_t *scratch,
                                    hipStream_t stream);
hipError_t rr_launch_lz4_compress(const uint8_t *in, uint64_t in_cap, const uint64_t *in_offs, uint64_t n, uint8_t *out,
                                  uint64_t *out_offs, uint64_t *scratch, uint64_t slot_bytes, hipStream_t stream);
/* The launches below are stages of one shape, rr_stage_device.h's: sizes, scan, emit ("the stage"),
 * some with an attempted list in front (flags, scan, compaction).
 * rr_rdbsave.hip (include/rr_rdbsave.h): the stage, then the Lists' two launches; scratch of
 * rr_rdbsave_scratch_words(n, lzf ? elem_cap : 0).  lzf: RR_RDBSAVE_LZF, the LZF instantiations of
 * the size and emit kernels */
uint64_t rr_rdbsave_scratch_words(uint64_t n, uint64_t lzf_elems);
hipError_t rr_launch_rdbsave(const rr_value *values, const rr_elem *elems, uint64_t elem_cap, const uint8_t *arena,
                             uint64_t arena_cap, uint64_t n, int list_fill, int lzf, uint8_t *out, uint64_t cap, uint64_t *offsets,
                             uint8_t *types, uint8_t *status, uint64_t *scratch, rr_totals *totals, hipStream_t stream);
/* rr_rdbload.hip (include/rr_rdbload.h): the stage; scratch of rr_rdbload_scratch_words(n).
 * opt6: lru & RR_LRU_MASK, then the five thresholds in rr_rdbload_opts' order */
uint64_t rr_rdbload_scratch_words(uint64_t n);
hipError_t rr_launch_rdbload(const uint8_t *data, uint64_t in_cap, const uint64_t *in_offs, const uint8_t *types, uint64_t n,
                             const uint32_t *opt6, uint8_t *out, uint64_t out_cap, uint64_t *out_offs, uint8_t *status,
                             uint64_t *scratch, rr_totals *totals, hipStream_t stream);
/* rr_rdbconvert.hip (include/rr_rdbconvert.h): the attempted list, then the stage over it; scratch of
 * rr_rdbconvert_scratch_words(n).  opt6 as for rr_launch_rdbload */
uint64_t rr_rdbconvert_scratch_words(uint64_t n);
hipError_t rr_launch_rdbconvert(const uint8_t *data, uint64_t in_cap, const uint64_t *in_offs, const uint8_t *types,
                                const uint8_t *load_status, uint64_t n, const uint32_t *opt6, uint8_t *out, uint64_t out_cap,
                                uint64_t *out_offs, uint8_t *out_types, uint8_t *status, uint64_t *scratch, rr_totals *totals,
                                hipStream_t stream);
/* rr_rdbzset.hip (include/rr_d2string.h, include/rr_rdbzset.h).  The printer: one launch, none for n ==
 * 0.  The stage: as rr_rdbconvert.hip's, the same scratch formula (rr_rdbzset_scratch_words(n));
 * opt6 as for rr_launch_rdbload */
hipError_t rr_launch_d2string(const uint64_t *bits, uint64_t n, uint8_t *text, uint8_t *len, hipStream_t stream);
uint64_t rr_rdbzset_scratch_words(uint64_t n);
hipError_t rr_launch_rdbzset(const uint8_t *data, uint64_t in_cap, const uint64_t *in_offs, const uint8_t *types,
                             const uint8_t *convert_status, uint64_t n, const uint32_t *opt6, uint8_t *out, uint64_t out_cap,
                             uint64_t *out_offs, uint8_t *status, uint64_t *scratch, rr_totals *totals, hipStream_t stream);
/* rr_rdbmerge.hip (include/rr_rdbloadall.h): the stage over the three load stages' batches (host
 * structs of device pointers, read at the launch), a thread a value for the sizes and a wave a span
 * of the output for the gather; scratch of rr_rdbmerge_scratch_words(n).  The second launch copies
 * the three batches' offsets[n] to dst[0..3) */
uint64_t rr_rdbmerge_scratch_words(uint64_t n);
hipError_t rr_launch_rdbmerge(const rr_blob_batch *in1, const uint8_t *s1, const rr_blob_batch *in2, const uint8_t *s2,
                              const uint8_t *conv_types, const rr_blob_batch *in3, const uint8_t *s3, const uint8_t *types,
                              uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_offs, uint8_t *out_types, uint8_t *status,
                              uint64_t *scratch, rr_totals *totals, hipStream_t stream);
hipError_t rr_launch_rdbmerge_stage_bytes(const uint64_t *o1, const uint64_t *o2, const uint64_t *o3, uint64_t n, uint64_t *dst,
                                          hipStream_t stream);
/* rr_aof.hip (include/rr_aof.h): the stage; scratch of rr_aof_scratch_words(n).  expires may
 * be NULL; every other pointer on the device */
uint64_t rr_aof_scratch_words(uint64_t n);
hipError_t rr_launch_aof(const rr_value *values, const rr_elem *elems, uint64_t elem_cap, const uint8_t *arena,
                         uint64_t arena_cap, uint64_t n, const uint8_t *keys, const uint64_t *key_offs, uint64_t key_cap,
                         const int64_t *expires, uint8_t *out, uint64_t cap, uint64_t *offsets, uint8_t *status,
                         uint64_t *scratch, rr_totals *totals, hipStream_t stream);
/* rr_rdbfile.hip (include/rr_rdbfile.h).  The CRC kernels' shape is RR_CRC64_RUN bytes a lane,
 * RR_CRC64_PIECE bytes a wave and step, at most RR_CRC64_MAX_WAVES waves (rr_rdbfile.h, mirrored in
 * the Python binding).  The section: sizes, scan, emit, CRC, combine; every pointer of *in on the
 * device, scratch of rr_rdbfile_scratch_words(n).  rr_launch_crc64: state[0] = crc64(state[0],
 * data[0, bytes)), scratch of rr_crc64_scratch_words().  The DUMP calls: sizes / check, scan, emit /
 * copy; scratch of rr_rdbdump_scratch_words(n). */
struct rr_rdbfile_in;
struct rr_rdbfile_result;
uint64_t rr_rdbfile_scratch_words(uint64_t n);
uint64_t rr_crc64_scratch_words(void);
uint64_t rr_rdbdump_scratch_words(uint64_t n);
hipError_t rr_launch_rdbfile(const struct rr_rdbfile_in *in, uint32_t flags, uint8_t *out, uint64_t out_cap, uint64_t *rec_offsets,
                             uint8_t *rec_status, uint64_t *state, struct rr_rdbfile_result *result, uint64_t *scratch,
                             hipStream_t stream);
hipError_t rr_launch_crc64(const uint8_t *data, uint64_t bytes, uint64_t *state, uint64_t *scratch, hipStream_t stream);
hipError_t rr_launch_rdbdump(const uint8_t *data, uint64_t in_cap, const uint64_t *in_offs, const uint8_t *types,
                             const uint8_t *status, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_offs,
                             uint8_t *out_status, uint64_t *scratch, struct rr_rdbfile_result *result, hipStream_t stream);
hipError_t rr_launch_rdbdump_verify(const uint8_t *data, uint64_t in_cap, const uint64_t *in_offs, uint64_t n, uint8_t *out,
                                    uint64_t out_cap, uint64_t *out_offs, uint8_t *types, uint8_t *status, uint64_t *scratch,
                                    struct rr_rdbfile_result *result, hipStream_t stream);
/* rr_rdbread.hip (include/rr_rdbread.h).  The split: sizes, one scan over key sizes | payload sizes,
 * emit; a wave a record, at most RR_RDBREAD_MAX_WAVES waves; every pointer of *out on the device,
 * scratch of rr_rdbread_scratch_words(n).  The verdict: state[0] against the 8 bytes at ck, into
 * *result (bytes as given). */
struct rr_rdbread_out;
uint64_t rr_rdbread_scratch_words(uint64_t n);
hipError_t rr_launch_rdbread_split(const uint8_t *data, uint64_t data_cap, const uint64_t *rec_start, const uint64_t *rec_end,
                                   uint64_t n, const struct rr_rdbread_out *out, uint64_t *scratch,
                                   struct rr_rdbfile_result *result, hipStream_t stream);
hipError_t rr_launch_rdbread_verdict(const uint8_t *ck, uint64_t bytes, const uint64_t *state, struct rr_rdbfile_result *result,
                                     hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
