/*
 * rr_rdbzset_api.c — host layer of include/rr_rdbzset.h (the small ZSets rr_rdbconvert_batch left
 * because a score needs %.17g) and of include/rr_d2string.h's batch calls: argument checks, the
 * options of rr_rdbload.h, the context's scratch, and the host-pointer forms that stage through the
 * context's device buffers.
 */
#include <string.h>

#include "rr_internal.h"
#include "../../include/rr_d2string.h"
#include "../../include/rr_rdbzset.h"

#define fail rr_fail

uint64_t rr_rdbzset_bound(uint64_t n, uint64_t payload_bytes) {
    return (24 * n + 4 * payload_bytes + 15) & ~15ull;
}

int rr_rdbzset_batch(rr_ctx *c, const rr_blob_batch *in, const uint8_t *types, const uint8_t *convert_status,
                     rr_blob_batch *out, uint8_t *status, rr_totals *d_totals, const rr_rdbload_opts *opts, void *stream) {
    uint32_t k[6];
    int rc = rr_rdbload_resolve_opts(opts, k);   /* first, as rr_rdbload_batch does */
    if (rc) return rc;
    rc = rr_check_blob_io(c, in, out, d_totals, types && convert_status && status);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    rc = rr_ensure_scratch(c, rr_rdbzset_scratch_words(in->n), (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(rr_launch_rdbzset(in->data, in->data_cap, in->offsets, types, convert_status, in->n, k, out->data, out->data_cap,
                             out->offsets, status, c->scratch, d_totals, (hipStream_t)stream));
    return rr_mark_scratch(c, (hipStream_t)stream);
}

int rr_rdbzset_batch_host(rr_ctx *c, const uint8_t *data, const uint64_t *offsets, const uint8_t *types,
                          const uint8_t *convert_status, uint64_t n, const rr_rdbload_opts *opts, uint8_t *out,
                          uint64_t out_cap, uint64_t *out_offsets, uint8_t *status, rr_totals *totals) {
    uint32_t k[6];
    int rc = rr_rdbload_resolve_opts(opts, k);
    if (rc) return rc;
    if (!c || !offsets || !out_offsets || (n && (!types || !convert_status || !status)) || (out_cap && !out))
        return fail(RR_API_EINVAL, "NULL argument");
    const uint64_t nbytes = rr_reach(offsets, n, ~0ull);
    if (nbytes && !data) return fail(RR_API_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    GROW(c->d_in, c->c_in, nbytes + 16);
    GROW(c->d_off, c->c_off, (n + 1) * sizeof(uint64_t));
    GROW(c->d_vals, c->c_vals, 3 * n + 16);   /* types, convert_status, status */
    GROW(c->d_out, c->c_out, out_cap + 16);
    GROW(c->d_ooff, c->c_ooff, (n + 1) * sizeof(uint64_t));
    uint8_t *d_types = (uint8_t *)c->d_vals, *d_conv = d_types + n, *d_status = d_conv + n;
    UP(c->d_in, data, nbytes);
    UP(c->d_off, offsets, (n + 1) * sizeof(uint64_t));
    UP(d_types, types, n);
    UP(d_conv, convert_status, n);
    rr_blob_batch in = {(uint8_t *)c->d_in, (uint64_t *)c->d_off, n, nbytes};
    rr_blob_batch ob = {(uint8_t *)c->d_out, (uint64_t *)c->d_ooff, n, out_cap};
    rc = rr_rdbzset_batch(c, &in, d_types, d_conv, &ob, d_status, c->d_totals, opts, c->stream);
    if (rc) return rc;
    rr_totals t;
    DOWN(&t, c->d_totals, sizeof t);
    DOWN(out_offsets, c->d_ooff, (n + 1) * sizeof(uint64_t));
    DOWN(status, d_status, n);
    rc = rr_host_finish(c, "rdbzset", &t.bytes, out, c->d_out, out_cap);
    if (rc) return rc;
    if (totals) *totals = t;
    return RR_API_OK;
}

int rr_d2string_batch(rr_ctx *c, const uint64_t *bits, uint64_t n, uint8_t *text, uint8_t *len, void *stream) {
    if (!c || (n && (!bits || !text || !len))) return fail(RR_API_EINVAL, "NULL argument");
    if (n > (~0ull >> 6)) return fail(RR_API_EINVAL, "n too large");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(rr_launch_d2string(bits, n, text, len, (hipStream_t)stream));
    return RR_API_OK;
}

int rr_d2string_batch_host(rr_ctx *c, const uint64_t *bits, uint64_t n, uint8_t *text, uint8_t *len) {
    if (!c || (n && (!bits || !text || !len))) return fail(RR_API_EINVAL, "NULL argument");
    if (n > (~0ull >> 6)) return fail(RR_API_EINVAL, "n too large");
    if (n == 0) return RR_API_OK;
    HIPCHK(hipSetDevice(c->device));
    GROW(c->d_in, c->c_in, 8 * n);
    GROW(c->d_out, c->c_out, RR_D2STRING_SLOT * n);
    GROW(c->d_vals, c->c_vals, n);
    UP(c->d_in, bits, 8 * n);
    UP(c->d_out, text, RR_D2STRING_SLOT * n);   /* the bytes the kernel leaves come back as they were */
    int rc = rr_d2string_batch(c, (const uint64_t *)c->d_in, n, (uint8_t *)c->d_out, (uint8_t *)c->d_vals, c->stream);
    if (rc) return rc;
    DOWN(text, c->d_out, RR_D2STRING_SLOT * n);
    DOWN(len, c->d_vals, n);
    HIPCHK(hipStreamSynchronize(c->stream));
    return RR_API_OK;
}
