/*
 * rr_rdbsave_api.c — host layer of include/rr_rdbsave.h (flat batch -> RDB value payloads, SURVEY.md
 * §8f row f4): argument checks, the context's scratch, the host-pointer form that stages through
 * the context's device buffers, and the child side of the pipe mode (RR_RDB_SAVE_TAG, rr_rdb.h).
 */
#include <stdlib.h>
#include <string.h>

#include "rr_internal.h"
#include "../../include/rr_rdb.h"
#include "../../include/rr_rdbsave.h"

#define fail rr_fail

uint64_t rr_rdbsave_bound(uint64_t n, uint64_t n_elems, uint64_t payload_bytes) {
    return (17 * n + 26 * n_elems + payload_bytes + 15) & ~15ull;
}

/* quicklistSetFill (quicklist.c:117-124) into the 16-bit field of quicklist.h:78 */
static int clamp_fill(const rr_rdbsave_opts *o) {
    const int f = o ? o->list_fill : RR_RDBSAVE_DEFAULT_FILL;
    return f > 32767 ? 32767 : f < -5 ? -5 : f;
}

int rr_rdbsave_batch(rr_ctx *c, const rr_flat_batch *in, rr_blob_batch *out, uint8_t *types, uint8_t *status,
                     rr_totals *d_totals, const rr_rdbsave_opts *opts, void *stream) {
    if (!c || !in || !out || !d_totals) return fail(RR_API_EINVAL, "NULL argument");
    if (out->n != in->n) return fail(RR_API_EINVAL, "out->n != in->n");
    if (in->n >= RR_MAX_VALUES) return fail(RR_API_EINVAL, "batch too large (value indices are 32-bit)");
    if (!out->offsets) return fail(RR_API_EINVAL, "NULL offsets");
    if (in->n && (!in->values || !out->data || !types || !status)) return fail(RR_API_EINVAL, "NULL buffer");
    if ((uintptr_t)out->data & 15) return fail(RR_API_EINVAL, "out->data must be 16-byte aligned");
    if (opts && (opts->flags & ~RR_RDBSAVE_LZF)) return fail(RR_API_EINVAL, "rr_rdbsave_opts.flags: unknown bit");
    const int lzf = opts && (opts->flags & RR_RDBSAVE_LZF);
    HIPCHK(hipSetDevice(c->device));
    /* the LZF form keeps a u32 per descriptor between the size and the emit pass */
    int rc = rr_ensure_scratch(c, rr_rdbsave_scratch_words(in->n, lzf ? in->elem_cap : 0), (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(rr_launch_rdbsave(in->values, in->elems, in->elem_cap, in->arena, in->arena_cap, in->n, clamp_fill(opts), lzf,
                             out->data, out->data_cap, out->offsets, types, status, c->scratch, d_totals,
                             (hipStream_t)stream));
    return rr_mark_scratch(c, (hipStream_t)stream);
}

int rr_rdbsave_batch_host(rr_ctx *c, const rr_value *values, const rr_elem *elems, uint64_t n_elems,
                          const uint8_t *arena, uint64_t arena_bytes, uint64_t n, const rr_rdbsave_opts *opts,
                          uint8_t *data, uint64_t data_cap, uint64_t *offsets, uint8_t *types, uint8_t *status,
                          rr_totals *totals) {
    if (!c || !offsets || (n && (!values || !data || !types || !status))) return fail(RR_API_EINVAL, "NULL argument");
    if ((n_elems && !elems) || (arena_bytes && !arena)) return fail(RR_API_EINVAL, "NULL argument");
    if (opts && (opts->flags & ~RR_RDBSAVE_LZF)) return fail(RR_API_EINVAL, "rr_rdbsave_opts.flags: unknown bit");
    HIPCHK(hipSetDevice(c->device));
    GROW(c->d_vals, c->c_vals, (n ? n : 1) * sizeof(rr_value));
    GROW(c->d_elems, c->c_elems, (n_elems ? n_elems : 1) * sizeof(rr_elem));
    GROW(c->d_arena, c->c_arena, arena_bytes + 16);
    GROW(c->d_out, c->c_out, data_cap + 16);
    GROW(c->d_ooff, c->c_ooff, (n + 1) * sizeof(uint64_t));
    GROW(c->d_in, c->c_in, 2 * n + 16);   /* types, status */
    UP(c->d_vals, values, n * sizeof(rr_value));
    UP(c->d_elems, elems, n_elems * sizeof(rr_elem));
    UP(c->d_arena, arena, arena_bytes);
    rr_flat_batch in = {(rr_value *)c->d_vals, (rr_elem *)c->d_elems, (uint8_t *)c->d_arena, n, n_elems, arena_bytes};
    rr_blob_batch out = {(uint8_t *)c->d_out, (uint64_t *)c->d_ooff, n, data_cap};
    uint8_t *d_types = (uint8_t *)c->d_in, *d_status = d_types + n;
    int rc = rr_rdbsave_batch(c, &in, &out, d_types, d_status, c->d_totals, opts, c->stream);
    if (rc) return rc;
    rr_totals t;
    DOWN(&t, c->d_totals, sizeof t);
    DOWN(offsets, c->d_ooff, (n + 1) * sizeof(uint64_t));
    DOWN(types, d_types, n);
    DOWN(status, d_status, n);
    rc = rr_host_finish(c, "rdbsave", &t.bytes, data, c->d_out, data_cap);
    if (rc) return rc;
    if (totals) *totals = t;
    return RR_API_OK;
}

/* ---- pipe mode, child side ------------------------------------------------------------------ */
void rr_rdbsave_result_free(rr_rdbsave_result *r) {
    if (!r) return;
    free(r->types);
    free(r->status);
    free(r->offsets);
    free(r->data);
    memset(r, 0, sizeof *r);
}

int rr_rdbsave_request(int fd_req, int fd_resp, const int *dbis, const char *const *keys, const size_t *key_lens,
                       size_t k, rr_rdbsave_result *out) {
    if (!out || (k && (!dbis || !keys || !key_lens))) return fail(RR_API_EINVAL, "rr_rdbsave_request: NULL argument");
    memset(out, 0, sizeof *out);
    size_t len = sizeof(int) + sizeof(size_t);
    for (size_t i = 0; i < k; i++) len += sizeof(int) + sizeof(size_t) + key_lens[i];
    uint8_t *req = (uint8_t *)malloc(len), *p = req;
    if (!req) return fail(RR_API_ENOMEM, "malloc");
    const int tag = RR_RDB_SAVE_TAG;
    memcpy(p, &tag, sizeof tag); p += sizeof tag;
    memcpy(p, &k, sizeof k); p += sizeof k;
    for (size_t i = 0; i < k; i++) {
        memcpy(p, &dbis[i], sizeof(int)); p += sizeof(int);
        memcpy(p, &key_lens[i], sizeof(size_t)); p += sizeof(size_t);
        memcpy(p, keys[i], key_lens[i]); p += key_lens[i];
    }
    const int w = rr_write_full(fd_req, req, len);   /* the service reads a whole request before it answers */
    free(req);
    if (w != 1) return fail(RR_API_EINVAL, "request pipe write failed");
    uint64_t h[2];
    if (rr_read_full(fd_resp, h, sizeof h) != 1) return fail(RR_API_EINVAL, "pipe closed (save header)");
    out->n = h[0];
    out->bytes = h[1];
    out->types = (uint8_t *)malloc(h[0] ? h[0] : 1);
    out->status = (uint8_t *)malloc(h[0] ? h[0] : 1);
    out->offsets = (uint64_t *)malloc((h[0] + 1) * sizeof(uint64_t));
    out->data = (uint8_t *)malloc(h[1] + 16);
    if (!out->types || !out->status || !out->offsets || !out->data) {
        rr_rdbsave_result_free(out);
        return fail(RR_API_ENOMEM, "malloc");
    }
    if ((h[0] && (rr_read_full(fd_resp, out->types, h[0]) != 1 || rr_read_full(fd_resp, out->status, h[0]) != 1)) ||
        rr_read_full(fd_resp, out->offsets, (h[0] + 1) * sizeof(uint64_t)) != 1 ||
        (h[1] && rr_read_full(fd_resp, out->data, h[1]) != 1)) {
        rr_rdbsave_result_free(out);
        return fail(RR_API_EINVAL, "pipe closed (save body)");
    }
    return RR_API_OK;
}
