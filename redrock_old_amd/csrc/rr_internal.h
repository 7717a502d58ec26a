/* rr_internal.h — what the C host files of the engine share; the function bodies are in rr_api.c. */
#ifndef RR_INTERNAL_H
#define RR_INTERNAL_H

#include "rr_kernels.h"

#define RR_HOST_CHUNK (16ull << 20)   /* pipelined host decode: bytes per chunk (at least) */
#define RR_HOST_MAXCHUNK 64

struct rr_ctx {
    int device;
    unsigned options;            /* RR_CTX_* */
    hipStream_t stream;          /* used by the host entry points */
    uint64_t *scratch;           /* look-back words + counters */
    uint64_t scratch_words;
    int scratch_used;            /* a call has used the scratch (growing it then waits for the device) */
    /* The zero-between-calls sums: [encode group sums, enc words][decode half 0, dec words]
     * [decode half 1][decode half for graph-captured calls].  A decode call adds its window and
     * group sums into one half while its count_kernel zeroes what the previous call left in the
     * other; the calls alternate (dphase), so no kernel has to find out that it finishes last. */
    uint64_t *dsums;
    uint64_t dsums_enc, dsums_dec;   /* words of the encode region / of each decode half */
    uint64_t dext[2];                /* words each decode half holds non-zero (its last call's sums) */
    int dphase;                      /* the half the next decode call uses */
    int dsums_dirty;                 /* a call failed midway: re-zero the whole buffer first */
    int fail_second;             /* test hooks: 1 (rr_debug_fail_second) the next pipeline call stops after its first
                                    kernel; 2 (rr_debug_one_help) the next one-launch decode helps every window */
    /* device staging for host entry points */
    void *d_in, *d_off, *d_vals, *d_elems, *d_arena, *d_out, *d_ooff;
    size_t c_in, c_off, c_vals, c_elems, c_arena, c_out, c_ooff;
    rr_totals *d_totals;
    /* pipelined host decode (rr_api.c): transfer streams, per-chunk events and totals */
    int pipe_ready;
    hipStream_t up, down, aux;
    hipEvent_t ev_up[RR_HOST_MAXCHUNK], ev_dec[RR_HOST_MAXCHUNK];
    rr_totals *d_ktot, *h_ktot;   /* device / pinned host, RR_HOST_MAXCHUNK each */
    uint64_t *h_need;             /* pinned, mapped: per chunk, the arena bytes its encode reads */
    hipEvent_t ev_arena[RR_HOST_MAXCHUNK], ev_enc[RR_HOST_MAXCHUNK], ev_need[RR_HOST_MAXCHUNK];
    /* small batches through the host entry points: one pinned buffer mapped into the device,
     * which the one-launch kernels read their input from and write their output to */
    uint8_t *h_small, *d_small;
    uint32_t small_seq;   /* the one-launch kernels' completion words (small_wait) */
    hipStream_t sstream;  /* the one-launch host calls' stream: the device's highest priority, so a
                           * per-key call is dispatched ahead of batch work queued elsewhere */
    size_t c_small;
};

/* the context's scratch: grow to `words` (waits on the previous call through an event; fails
 * under graph capture), and mark the end of a call's use of it */
int rr_ensure_scratch(rr_ctx *c, uint64_t words, hipStream_t stream);
int rr_mark_scratch(rr_ctx *c, hipStream_t stream);
/* grow a device staging buffer of the host entry points */
int rr_dgrow(void **p, size_t *cap, size_t need);

/* sets rr_last_error() and returns code */
int rr_fail(int code, const char *fmt, ...);
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
    return rr_fail(RR_API_EHIP, "%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); } while (0)

/* ---- what the host-pointer (*_host) entry points share; all of it returns from the caller on
 * failure and stages on the context `c` in scope ---- */
#define GROW(P, C, N) do { int r_ = rr_dgrow((void **)&(P), &(C), (N)); if (r_) return r_; } while (0)
#define UP(D, S, B) do { if ((B) != 0) HIPCHK(hipMemcpyAsync((D), (S), (B), hipMemcpyHostToDevice, c->stream)); } while (0)
#define DOWN(D, S, B) do { if ((B) != 0) HIPCHK(hipMemcpyAsync((D), (S), (B), hipMemcpyDeviceToHost, c->stream)); } while (0)

#define RR_HIDDEN __attribute__((visibility("hidden")))   /* shared between the host files, not exported */

/* the bytes the slices offs[0 .. n] reach within cap; a slice past them does not exist on the device */
RR_HIDDEN uint64_t rr_reach(const uint64_t *offs, uint64_t n, uint64_t cap);
/* The argument block of a device call from one blob batch to another (d_result: its rr_totals or
 * rr_rdbfile_result; have_arrays: the call's per-value arrays are all there).  Sets the error. */
RR_HIDDEN int rr_check_blob_io(const rr_ctx *c, const rr_blob_batch *in, const rr_blob_batch *out, const void *d_result,
                               int have_arrays);
/* The end of a *_host call whose result record (an rr_totals or an rr_rdbfile_result; *bytes its
 * bytes field) and per-value arrays are already queued for download: waits for them, fails on the
 * look-back's error mark, then brings down the first min(*bytes, cap) bytes of the output. */
RR_HIDDEN int rr_host_finish(rr_ctx *c, const char *name, const uint64_t *bytes, void *out, const void *d_out, uint64_t cap);

/* rr_rdbload_opts checked and resolved (NULL: the defaults) into what the RDB load kernels take: lru &
 * RR_LRU_MASK, then the five thresholds.  Sets the error.  (rr_rdbload_api.c) */
struct rr_rdbload_opts;
RR_HIDDEN int rr_rdbload_resolve_opts(const struct rr_rdbload_opts *o, uint32_t k[6]);

/* read / write exactly len bytes on a blocking fd: 1 done, 0 closed, -1 error
 * (the reference's _read_pipe_by_length / _write_pipe_by_length, rock_rdb.c:64-103) */
RR_HIDDEN int rr_read_full(int fd, void *buf, size_t len);
RR_HIDDEN int rr_write_full(int fd, const void *buf, size_t len);

#endif
