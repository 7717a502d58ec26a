/*
 * rr_rdbload_api.c — host layer of include/rr_rdbload.h (RDB value payloads -> rock blobs): argument
 * checks, the options' defaults, the context's scratch, and the host-pointer form that stages
 * through the context's device buffers.
 */
#include <string.h>

#include "rr_internal.h"
#include "../../include/rr_rdbload.h"

#define fail rr_fail

uint64_t rr_rdbload_bound(uint64_t n, uint64_t payload_bytes) {
    return (5 * n + 8 * payload_bytes + 15) & ~15ull;
}

/* lru, then the five thresholds: what the kernels take.  The defaults are config.c:2261-2267.
 * (rr_rdbconvert_api.c takes the same options through it.) */
int rr_rdbload_resolve_opts(const rr_rdbload_opts *o, uint32_t k[6]) {
    static const rr_rdbload_opts def = {0, 512, 512, 64, 128, 64, 0};
    if (!o) o = &def;
    if (o->flags) return fail(RR_API_EINVAL, "rr_rdbload_opts.flags: unknown bit");
    if (o->set_max_intset_entries > 32767 || o->hash_max_ziplist_entries > 32767 || o->zset_max_ziplist_entries > 32767)
        return fail(RR_API_EINVAL, "rr_rdbload_opts: an *_entries threshold above 32767");
    k[0] = o->lru & RR_LRU_MASK;
    k[1] = o->set_max_intset_entries;
    k[2] = o->hash_max_ziplist_entries;
    k[3] = o->hash_max_ziplist_value;
    k[4] = o->zset_max_ziplist_entries;
    k[5] = o->zset_max_ziplist_value;
    return RR_API_OK;
}

int rr_rdbload_batch(rr_ctx *c, const rr_blob_batch *in, const uint8_t *types, rr_blob_batch *out, uint8_t *status,
                     rr_totals *d_totals, const rr_rdbload_opts *opts, void *stream) {
    uint32_t k[6];
    int rc = rr_rdbload_resolve_opts(opts, k);   /* first: the options are checked whatever else is wrong */
    if (rc) return rc;
    rc = rr_check_blob_io(c, in, out, d_totals, types && status);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    rc = rr_ensure_scratch(c, rr_rdbload_scratch_words(in->n), (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(rr_launch_rdbload(in->data, in->data_cap, in->offsets, types, in->n, k, out->data, out->data_cap, out->offsets,
                             status, c->scratch, d_totals, (hipStream_t)stream));
    return rr_mark_scratch(c, (hipStream_t)stream);
}

int rr_rdbload_batch_host(rr_ctx *c, const uint8_t *data, const uint64_t *offsets, const uint8_t *types, uint64_t n,
                          const rr_rdbload_opts *opts, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                          uint8_t *status, rr_totals *totals) {
    uint32_t k[6];
    int rc = rr_rdbload_resolve_opts(opts, k);
    if (rc) return rc;
    if (!c || !offsets || !out_offsets || (n && (!types || !status)) || (out_cap && !out))
        return fail(RR_API_EINVAL, "NULL argument");
    const uint64_t nbytes = rr_reach(offsets, n, ~0ull);
    if (nbytes && !data) return fail(RR_API_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    GROW(c->d_in, c->c_in, nbytes + 16);
    GROW(c->d_off, c->c_off, (n + 1) * sizeof(uint64_t));
    GROW(c->d_vals, c->c_vals, 2 * n + 16);   /* types, status */
    GROW(c->d_out, c->c_out, out_cap + 16);
    GROW(c->d_ooff, c->c_ooff, (n + 1) * sizeof(uint64_t));
    uint8_t *d_types = (uint8_t *)c->d_vals, *d_status = d_types + n;
    UP(c->d_in, data, nbytes);
    UP(c->d_off, offsets, (n + 1) * sizeof(uint64_t));
    UP(d_types, types, n);
    rr_blob_batch in = {(uint8_t *)c->d_in, (uint64_t *)c->d_off, n, nbytes};
    rr_blob_batch ob = {(uint8_t *)c->d_out, (uint64_t *)c->d_ooff, n, out_cap};
    rc = rr_rdbload_batch(c, &in, d_types, &ob, d_status, c->d_totals, opts, c->stream);
    if (rc) return rc;
    rr_totals t;
    DOWN(&t, c->d_totals, sizeof t);
    DOWN(out_offsets, c->d_ooff, (n + 1) * sizeof(uint64_t));
    DOWN(status, d_status, n);
    rc = rr_host_finish(c, "rdbload", &t.bytes, out, c->d_out, out_cap);
    if (rc) return rc;
    if (totals) *totals = t;
    return RR_API_OK;
}
