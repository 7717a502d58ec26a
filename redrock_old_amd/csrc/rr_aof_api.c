/*
 * rr_aof_api.c — host layer of include/rr_aof.h (flat batch -> AOF rewrite commands, SURVEY.md §8f row
 * f4): argument checks, the context's scratch, the host-pointer form that stages through the context's
 * device buffers, and the host twins of what the kernels print (the SELECT line, a score text).
 */
#include <string.h>

#include "rr_internal.h"
#include "../../include/rr_aof.h"
#include "rr_strtod_impl.h"

#define fail rr_fail

uint64_t rr_aof_bound(uint64_t n, uint64_t n_elems, uint64_t payload_bytes, uint64_t key_bytes) {
    return (128 * n + 32 * n_elems + payload_bytes + key_bytes * (2 + n_elems / 64) + 15) & ~15ull;
}

int rr_aof_select(uint8_t *buf, uint64_t cap, int dbi) {
    static const char head[] = "*2\r\n$6\r\nSELECT\r\n";
    char num[16], out[48];
    if (!buf || dbi < 0) return 0;
    const int nl = rr_d2s_ll(num, 0, (uint64_t)dbi);
    char cnt[4];
    const int cl = rr_d2s_ll(cnt, 0, (uint64_t)nl);
    int p = (int)sizeof head - 1;
    memcpy(out, head, (size_t)p);
    out[p++] = '$';
    memcpy(out + p, cnt, (size_t)cl); p += cl;
    out[p++] = '\r'; out[p++] = '\n';
    memcpy(out + p, num, (size_t)nl); p += nl;
    out[p++] = '\r'; out[p++] = '\n';
    if ((uint64_t)p > cap) return 0;
    memcpy(buf, out, (size_t)p);
    return p;
}

int rr_aof_score_text(char *buf, const char *text, uint64_t len) {
    uint32_t w[RR_D2S_WORDS];
    uint64_t bits;
    if (!buf || (len && !text) || len > RR_AOF_SCORE_TEXT_MAX) return -1;
    if (!rr_s2d_parse((const uint8_t *)text, (uint32_t)len, &bits, w)) return -1;
    return rr_d2s_print(buf, bits, w);
}

int rr_aof_batch(rr_ctx *c, const rr_flat_batch *in, const rr_blob_batch *keys, const int64_t *expires, rr_blob_batch *out,
                 uint8_t *status, rr_totals *d_totals, void *stream) {
    if (!c || !in || !keys || !out || !d_totals) return fail(RR_API_EINVAL, "NULL argument");
    if (out->n != in->n || keys->n != in->n) return fail(RR_API_EINVAL, "out->n, keys->n and in->n differ");
    if (in->n >= RR_MAX_VALUES) return fail(RR_API_EINVAL, "batch too large (value indices are 32-bit)");
    if (!out->offsets || !keys->offsets) return fail(RR_API_EINVAL, "NULL offsets");
    if (in->n && (!in->values || !status)) return fail(RR_API_EINVAL, "NULL buffer");
    if (out->data_cap && !out->data) return fail(RR_API_EINVAL, "NULL out->data");
    if ((uintptr_t)out->data & 15) return fail(RR_API_EINVAL, "out->data must be 16-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    int rc = rr_ensure_scratch(c, rr_aof_scratch_words(in->n), (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(rr_launch_aof(in->values, in->elems, in->elem_cap, in->arena, in->arena_cap, in->n, keys->data, keys->offsets,
                         keys->data_cap, expires, out->data, out->data_cap, out->offsets, status, c->scratch, d_totals,
                         (hipStream_t)stream));
    return rr_mark_scratch(c, (hipStream_t)stream);
}

int rr_aof_batch_host(rr_ctx *c, const rr_value *values, const rr_elem *elems, uint64_t n_elems, const uint8_t *arena,
                      uint64_t arena_bytes, uint64_t n, const uint8_t *key_data, const uint64_t *key_offsets,
                      uint64_t key_bytes, const int64_t *expires, uint8_t *data, uint64_t data_cap, uint64_t *offsets, uint8_t *status,
                      rr_totals *totals) {
    if (!c || !offsets || !key_offsets || (n && (!values || !status)) || (data_cap && !data))
        return fail(RR_API_EINVAL, "NULL argument");
    if ((n_elems && !elems) || (arena_bytes && !arena)) return fail(RR_API_EINVAL, "NULL argument");
    const uint64_t kbytes = rr_reach(key_offsets, n, key_bytes);   /* a slice past key_bytes is RR_RDBFILE_E_KEY */
    if (kbytes && !key_data) return fail(RR_API_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    GROW(c->d_vals, c->c_vals, (n ? n : 1) * sizeof(rr_value));
    GROW(c->d_elems, c->c_elems, (n_elems ? n_elems : 1) * sizeof(rr_elem));
    GROW(c->d_arena, c->c_arena, arena_bytes + 16);
    GROW(c->d_out, c->c_out, data_cap + 16);
    GROW(c->d_ooff, c->c_ooff, (n + 1) * sizeof(uint64_t));
    GROW(c->d_in, c->c_in, kbytes + 16);
    /* key offsets | expires | status */
    GROW(c->d_off, c->c_off, (2 * n + 1) * sizeof(uint64_t) + n + 16);
    uint64_t *d_koff = (uint64_t *)c->d_off;
    int64_t *d_exp = (int64_t *)(d_koff + n + 1);
    uint8_t *d_status = (uint8_t *)(d_exp + n);
    UP(c->d_vals, values, n * sizeof(rr_value));
    UP(c->d_elems, elems, n_elems * sizeof(rr_elem));
    UP(c->d_arena, arena, arena_bytes);
    UP(c->d_in, key_data, kbytes);
    UP(d_koff, key_offsets, (n + 1) * sizeof(uint64_t));
    if (expires) UP(d_exp, expires, n * sizeof(int64_t));
    rr_flat_batch in = {(rr_value *)c->d_vals, (rr_elem *)c->d_elems, (uint8_t *)c->d_arena, n, n_elems, arena_bytes};
    rr_blob_batch kb = {(uint8_t *)c->d_in, d_koff, n, kbytes};   /* every slice inside key_bytes ends at or before kbytes */
    rr_blob_batch out = {(uint8_t *)c->d_out, (uint64_t *)c->d_ooff, n, data_cap};
    int rc = rr_aof_batch(c, &in, &kb, expires ? d_exp : NULL, &out, d_status, c->d_totals, c->stream);
    if (rc) return rc;
    rr_totals t;
    DOWN(&t, c->d_totals, sizeof t);
    DOWN(offsets, c->d_ooff, (n + 1) * sizeof(uint64_t));
    DOWN(status, d_status, n);
    rc = rr_host_finish(c, "aof", &t.bytes, data, c->d_out, data_cap);
    if (rc) return rc;
    if (totals) *totals = t;
    return RR_API_OK;
}
