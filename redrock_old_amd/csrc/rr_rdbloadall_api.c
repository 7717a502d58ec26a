/*
 * rr_rdbloadall_api.c — host layer of include/rr_rdbloadall.h (the three load stages merged into one
 * blob batch): argument checks, the workspace's layout, the three stage calls and the merge on one
 * stream over the context's single scratch, and the host-pointer form that stages through the
 * context's device buffers.
 */
#include <string.h>

#include "rr_internal.h"
#include "../../include/rr_rdbloadall.h"

#define fail rr_fail
#define A16(x) (((x) + 15) & ~15ull)

static int merge_in_ok(const rr_blob_batch *b, uint64_t n) {
    return b->n == n && b->offsets && (!b->data_cap || b->data) && b->data_cap < (1ull << 62);
}

int rr_rdbmerge_batch(rr_ctx *c, const rr_blob_batch *in1, const uint8_t *s1, const rr_blob_batch *in2, const uint8_t *s2,
                      const uint8_t *conv_types, const rr_blob_batch *in3, const uint8_t *s3, const uint8_t *types,
                      rr_blob_batch *out, uint8_t *out_types, uint8_t *status, rr_totals *d_totals, void *stream) {
    if (!in2 || !in3) return fail(RR_API_EINVAL, "NULL argument");
    int rc = rr_check_blob_io(c, in1, out, d_totals, s1 && s2 && s3 && conv_types && types && status);
    if (rc) return rc;
    if (!merge_in_ok(in1, out->n) || !merge_in_ok(in2, out->n) || !merge_in_ok(in3, out->n))
        return fail(RR_API_EINVAL, "rr_rdbmerge_batch: a stage batch with another n, NULL offsets or data, or a data_cap of 2^62 or more");
    if ((uintptr_t)out->data & 15) return fail(RR_API_EINVAL, "out->data must be 16-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    rc = rr_ensure_scratch(c, rr_rdbmerge_scratch_words(out->n), (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(rr_launch_rdbmerge(in1, s1, in2, s2, conv_types, in3, s3, types, out->n, out->data, out->data_cap, out->offsets,
                              out_types, status, c->scratch, d_totals, (hipStream_t)stream));
    return rr_mark_scratch(c, (hipStream_t)stream);
}

void rr_rdbloadall_caps(uint64_t n, uint64_t payload_bytes, uint64_t stage_cap[3]) {
    stage_cap[0] = rr_rdbload_bound(n, payload_bytes);
    stage_cap[1] = rr_rdbconvert_bound(n, payload_bytes);
    stage_cap[2] = rr_rdbzset_bound(n, payload_bytes);
}

/* the workspace (rr_rdbloadall.h): offsets | totals | s1, s2, s3, conv_types | the three data areas */
typedef struct ws_parts {
    uint64_t *offs[3];
    rr_totals *totals;
    uint8_t *st[3], *conv_types, *data[3];
    uint64_t bytes;
} ws_parts;

static ws_parts ws_carve(void *ws, uint64_t n, const uint64_t cap[3]) {
    ws_parts p;
    const uintptr_t base = (uintptr_t)ws;
    uint64_t at = 0;
    for (int k = 0; k < 3; k++) p.offs[k] = (uint64_t *)(base + at + (uint64_t)k * (n + 1) * sizeof(uint64_t));
    at += A16(3 * (n + 1) * sizeof(uint64_t));
    p.totals = (rr_totals *)(base + at);
    at += 3 * sizeof(rr_totals);
    for (int k = 0; k < 3; k++) p.st[k] = (uint8_t *)(base + at + (uint64_t)k * n);
    p.conv_types = (uint8_t *)(base + at + 3 * n);
    at += A16(4 * n);
    for (int k = 0; k < 3; k++) {
        p.data[k] = (uint8_t *)(base + at);
        at += A16(cap[k]);
    }
    p.bytes = at;
    return p;
}

uint64_t rr_rdbloadall_ws_bytes(uint64_t n, const uint64_t stage_cap[3]) {
    return ws_carve(NULL, n, stage_cap).bytes;
}

int rr_rdbloadall_batch(rr_ctx *c, const rr_blob_batch *in, const uint8_t *types, void *ws, uint64_t ws_bytes,
                        const uint64_t stage_cap[3], rr_blob_batch *out, uint8_t *out_types, uint8_t *status,
                        uint64_t *d_stage_bytes, rr_totals *d_totals, const rr_rdbload_opts *opts, void *stream) {
    uint32_t k6[6];
    int rc = rr_rdbload_resolve_opts(opts, k6);   /* first, as rr_rdbload_batch does */
    if (rc) return rc;
    rc = rr_check_blob_io(c, in, out, d_totals, types && status);
    if (rc) return rc;
    if (!ws || !stage_cap || !d_stage_bytes) return fail(RR_API_EINVAL, "NULL argument");
    if ((uintptr_t)ws & 15) return fail(RR_API_EINVAL, "rr_rdbloadall_batch: ws must be 16-byte aligned");
    if (stage_cap[0] >> 62 || stage_cap[1] >> 62 || stage_cap[2] >> 62) return fail(RR_API_EINVAL, "rr_rdbloadall_batch: stage_cap");
    const uint64_t n = in->n;
    const ws_parts p = ws_carve(ws, n, stage_cap);
    if (ws_bytes < p.bytes)
        return fail(RR_API_EINVAL, "rr_rdbloadall_batch: ws_bytes %llu below rr_rdbloadall_ws_bytes() = %llu",
                    (unsigned long long)ws_bytes, (unsigned long long)p.bytes);
    if ((uintptr_t)out->data & 15) return fail(RR_API_EINVAL, "out->data must be 16-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    /* The four steps share the context's one scratch.  rr_ensure_scratch grows it by freeing it, behind
     * a device-wide wait once it has been used, and refuses to under graph capture: sized here for the
     * largest step, no step of this call grows it, and a capture after one warm call finds it large enough. */
    uint64_t words = rr_rdbload_scratch_words(n), w;
    if ((w = rr_rdbconvert_scratch_words(n)) > words) words = w;
    if ((w = rr_rdbzset_scratch_words(n)) > words) words = w;
    if ((w = rr_rdbmerge_scratch_words(n)) > words) words = w;
    rc = rr_ensure_scratch(c, words, (hipStream_t)stream);
    if (rc) return rc;
    rr_blob_batch b[3];
    for (int k = 0; k < 3; k++) b[k] = (rr_blob_batch){stage_cap[k] ? p.data[k] : NULL, p.offs[k], n, stage_cap[k]};
    rc = rr_rdbload_batch(c, in, types, &b[0], p.st[0], &p.totals[0], opts, stream);
    if (rc) return rc;
    rc = rr_rdbconvert_batch(c, in, types, p.st[0], &b[1], p.conv_types, p.st[1], &p.totals[1], opts, stream);
    if (rc) return rc;
    rc = rr_rdbzset_batch(c, in, types, p.st[1], &b[2], p.st[2], &p.totals[2], opts, stream);
    if (rc) return rc;
    HIPCHK(rr_launch_rdbmerge_stage_bytes(p.offs[0], p.offs[1], p.offs[2], n, d_stage_bytes, (hipStream_t)stream));
    return rr_rdbmerge_batch(c, &b[0], p.st[0], &b[1], p.st[1], p.conv_types, &b[2], p.st[2], types, out, out_types, status,
                             d_totals, stream);
}

int rr_rdbloadall_batch_host(rr_ctx *c, const uint8_t *data, const uint64_t *offsets, const uint8_t *types, uint64_t n,
                             const rr_rdbload_opts *opts, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                             uint8_t *out_types, uint8_t *status, uint64_t *stage_bytes, rr_totals *totals) {
    uint32_t k6[6];
    int rc = rr_rdbload_resolve_opts(opts, k6);
    if (rc) return rc;
    if (!c || !offsets || !out_offsets || (n && (!types || !status)) || (out_cap && !out))
        return fail(RR_API_EINVAL, "NULL argument");
    const uint64_t nbytes = rr_reach(offsets, n, ~0ull);
    if (nbytes && !data) return fail(RR_API_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    GROW(c->d_in, c->c_in, nbytes + 16);
    GROW(c->d_off, c->c_off, (n + 1) * sizeof(uint64_t));
    GROW(c->d_vals, c->c_vals, 3 * n + 16);   /* types, out_types, status */
    GROW(c->d_elems, c->c_elems, 64);         /* the stages' bytes */
    GROW(c->d_out, c->c_out, out_cap + 16);
    GROW(c->d_ooff, c->c_ooff, (n + 1) * sizeof(uint64_t));
    uint8_t *d_types = (uint8_t *)c->d_vals, *d_otypes = d_types + n, *d_status = d_otypes + n;
    uint64_t *d_sb = (uint64_t *)c->d_elems;
    UP(c->d_in, data, nbytes);
    UP(c->d_off, offsets, (n + 1) * sizeof(uint64_t));
    UP(d_types, types, n);
    rr_blob_batch in = {(uint8_t *)c->d_in, (uint64_t *)c->d_off, n, nbytes};
    /* the sizing run, then the workspace it asks for (the arena buffer of the decode's host form) */
    uint64_t cap[3] = {0, 0, 0}, sb[3];
    uint64_t need = rr_rdbloadall_ws_bytes(n, cap);
    GROW(c->d_arena, c->c_arena, need);
    rr_blob_batch ob = {NULL, (uint64_t *)c->d_ooff, n, 0};
    rc = rr_rdbloadall_batch(c, &in, d_types, c->d_arena, need, cap, &ob, d_otypes, d_status, d_sb, c->d_totals, opts, c->stream);
    if (rc) return rc;
    DOWN(sb, d_sb, sizeof sb);
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; k++) {
        if (sb[k] >> 62) return fail(RR_API_EDEVICE, "rdbloadall: device-side failure (look-back timeout)");
        cap[k] = A16(sb[k]);
    }
    need = rr_rdbloadall_ws_bytes(n, cap);
    GROW(c->d_arena, c->c_arena, need);
    ob = (rr_blob_batch){(uint8_t *)c->d_out, (uint64_t *)c->d_ooff, n, out_cap};
    rc = rr_rdbloadall_batch(c, &in, d_types, c->d_arena, need, cap, &ob, d_otypes, d_status, d_sb, c->d_totals, opts, c->stream);
    if (rc) return rc;
    rr_totals t;
    DOWN(&t, c->d_totals, sizeof t);
    DOWN(out_offsets, c->d_ooff, (n + 1) * sizeof(uint64_t));
    DOWN(status, d_status, n);
    if (out_types) DOWN(out_types, d_otypes, n);
    if (stage_bytes) DOWN(stage_bytes, d_sb, sizeof sb);
    rc = rr_host_finish(c, "rdbloadall", &t.bytes, out, c->d_out, out_cap);
    if (rc) return rc;
    if (totals) *totals = t;
    return RR_API_OK;
}
