/*
 * rr_rdbread_api.c — host layer of include/rr_rdbread.h: the record index (rdbLoadRio's framing walked
 * by lengths alone, rdb.c:2044-2312) and the host string reader, which need no GPU, then argument
 * checks, the context's scratch and the host-pointer forms of the device calls.
 * RR_RDBREAD_HOST_ONLY compiles the index and the string reader alone (a stand-alone check needs no HIP).
 */
#include <string.h>

#include "../../include/rr_rdbread.h"

/* ---- a bounded cursor: every test is made against the bytes that remain --------------------------- */
typedef struct cur { const uint8_t *b; uint64_t n, p; } cur;   /* p <= n always */

#define W_OK 0   /* the walkers' result: W_OK, RR_RDBREAD_MORE, RR_RDBREAD_E_LEN or RR_RDBREAD_E_UNSUPPORTED */

static int c_skip(cur *c, uint64_t k) {
    if (k > c->n - c->p) return RR_RDBREAD_MORE;
    c->p += k;
    return W_OK;
}

/* rdbLoadLen, rdb.c:190-234 */
static int c_len(cur *c, int *isenc, uint64_t *val) {
    *isenc = 0;
    *val = 0;
    if (c->n - c->p < 1) return RR_RDBREAD_MORE;
    const uint8_t *q = c->b + c->p;
    const uint32_t b0 = q[0], t = b0 >> 6;
    if (t == 3) { *isenc = 1; *val = b0 & 0x3F; c->p += 1; return W_OK; }   /* :197-200 */
    if (t == 0) { *val = b0 & 0x3F; c->p += 1; return W_OK; }               /* :201-203 */
    if (t == 1) {                                                           /* :204-207 */
        if (c->n - c->p < 2) return RR_RDBREAD_MORE;
        *val = ((uint64_t)(b0 & 0x3F) << 8) | q[1];
        c->p += 2;
        return W_OK;
    }
    const uint32_t nb = b0 == 0x80 ? 4 : b0 == 0x81 ? 8 : 0;               /* :208-217 */
    if (!nb) return RR_RDBREAD_E_LEN;                                       /* :219 */
    if (c->n - c->p < 1 + nb) return RR_RDBREAD_MORE;
    uint64_t v = 0;
    for (uint32_t k = 0; k < nb; k++) v = (v << 8) | q[1 + k];
    *val = v;
    c->p += 1 + nb;
    return W_OK;
}

static int c_count(cur *c, uint64_t *val) {   /* rdbLoadLen(rdb, NULL): the encoded form is its six bits */
    int ie;
    return c_len(c, &ie, val);
}

/* rdbGenericLoadStringObject (rdb.c:487-540) skipped, not loaded */
static int c_skip_string(cur *c) {
    int ie, rc;
    uint64_t v, clen, ulen;
    if ((rc = c_len(c, &ie, &v))) return rc;
    if (!ie) return c_skip(c, v);
    if (v <= 2) return c_skip(c, 1ull << v);               /* RDB_ENC_INT8 / 16 / 32 */
    if (v != 3) return RR_RDBREAD_E_LEN;                   /* :512 unknown string encoding */
    if ((rc = c_count(c, &clen))) return rc;               /* :376 */
    if ((rc = c_count(c, &ulen))) return rc;               /* :377 */
    return c_skip(c, clen);
}

/* the value of RDB type `type` skipped (rdbLoadObject's reads, rdb.c:1450-1700, by lengths only) */
static int c_skip_value(cur *c, uint32_t type) {
    int rc;
    uint64_t cnt;
    switch (type) {
        case 0: case 9: case 10: case 11: case 12: case 13:
            return c_skip_string(c);
        case 1: case 2: case 14: case 4: case 5: case 3:
            if ((rc = c_count(c, &cnt))) return rc;
            /* every round takes at least one byte, so a count near 2^64 ends at the buffer's end */
            for (uint64_t k = 0; k < cnt; k++) {
                if ((rc = c_skip_string(c))) return rc;
                if (type == 4 && (rc = c_skip_string(c))) return rc;
                if (type == 5 && (rc = c_skip(c, 8))) return rc;
                if (type == 3) {                           /* rdbLoadDoubleValue, :583-598 */
                    if (c->n - c->p < 1) return RR_RDBREAD_MORE;
                    const uint32_t l = c->b[c->p];
                    if ((rc = c_skip(c, 1 + (l >= 253 ? 0u : l)))) return rc;
                }
            }
            return W_OK;
        default:
            return RR_RDBREAD_E_UNSUPPORTED;               /* modules, streams, 0xF7, unknown */
    }
}

static int is_prefix_op(uint32_t op) { return op == 0xFD || op == 0xFC || op == 0xF8 || op == 0xF9; }
static int type_indexed(uint32_t t) { return t <= 5 || (t >= 9 && t <= 14); }

int rr_rdbread_index(rr_rdbread_state *st, const uint8_t *buf, uint64_t bytes, uint64_t *rec_start, uint64_t *rec_end,
                     uint64_t *rec_db, uint64_t max_recs, rr_rdbread_item *items, uint64_t max_items,
                     rr_rdbread_index_result *res) {
    if (!st || !res || (bytes && !buf) || st->pos > bytes) return RR_API_EINVAL;
    if ((max_recs && (!rec_start || !rec_end || !rec_db)) || (max_items && !items)) return RR_API_EINVAL;
    memset(res, 0, sizeof *res);
    cur c = {buf, bytes, st->pos};
    if (st->version == 0) {                                /* rdb.c:2052-2064 */
        if (c.n - c.p < 9) return RR_RDBREAD_MORE;
        const uint8_t *h = buf + c.p;
        res->err_at = c.p;
        if (memcmp(h, "REDIS", 5) != 0) return RR_RDBREAD_E_MAGIC;
        uint32_t v = 0;
        for (int k = 5; k < 9; k++) {
            if (h[k] < '0' || h[k] > '9') return RR_RDBREAD_E_VERSION;
            v = v * 10 + (uint32_t)(h[k] - '0');
        }
        if (v < 1 || v > RR_RDB_VERSION) return RR_RDBREAD_E_VERSION;
        res->err_at = 0;
        st->version = v;
        st->db = 0;
        c.p += 9;
        st->pos = c.p;
    }
    for (;;) {                                             /* :2072-2242 */
        const uint64_t at = c.p;                           /* the start of this item or record */
        st->pos = at;
        if (c.n - c.p < 1) return RR_RDBREAD_MORE;
        uint32_t op = buf[c.p];
        int rc = W_OK;
        if (op == 0xFF) {                                  /* :2105-2107, :2298-2311 */
            const int has = st->version >= 5;
            if (c.n - c.p < (has ? 9u : 1u)) return RR_RDBREAD_MORE;
            res->eof_at = at;
            res->has_cksum = (uint32_t)has;
            if (has)
                for (int k = 0; k < 8; k++) res->cksum |= (uint64_t)buf[at + 1 + k] << (8 * k);
            st->pos = at + (has ? 9 : 1);
            return RR_RDBREAD_DONE;
        }
        if (op == 0xFA || op == 0xFE || op == 0xFB) {
            if (res->n_items == max_items) return RR_RDBREAD_FULL;
            uint64_t v = 0, db = st->db;
            c.p += 1;
            if (op == 0xFA) {                              /* :2131-2139 */
                if (!(rc = c_skip_string(&c))) rc = c_skip_string(&c);
            } else if (op == 0xFE) {                       /* :2108-2119 */
                rc = c_count(&c, &db);
            } else {                                       /* :2120-2130 */
                if (!(rc = c_count(&c, &v))) rc = c_count(&c, &v);
            }
            if (rc == RR_RDBREAD_MORE) return rc;
            if (rc) { res->err_at = at; return rc; }
            st->db = db;
            rr_rdbread_item *it = &items[res->n_items++];
            it->opcode = op;
            it->rsv = 0;
            it->at = at;
            it->end = c.p;
            continue;
        }
        if (res->n_recs == max_recs) return RR_RDBREAD_FULL;
        while (is_prefix_op(op)) {                         /* :2079-2104 */
            uint64_t v;
            c.p += 1;
            rc = op == 0xFD ? c_skip(&c, 4) : op == 0xFC ? c_skip(&c, 8) : op == 0xF9 ? c_skip(&c, 1) : c_count(&c, &v);
            if (rc) break;
            if (c.n - c.p < 1) { rc = RR_RDBREAD_MORE; break; }
            op = buf[c.p];
        }
        if (!rc) {
            if (!type_indexed(op)) rc = RR_RDBREAD_E_UNSUPPORTED;       /* (an opcode behind a prefix too) */
            else {
                c.p += 1;
                if (!(rc = c_skip_string(&c))) rc = c_skip_value(&c, op);   /* :2231-2242 */
            }
        }
        if (rc == RR_RDBREAD_MORE) return rc;
        if (rc) { res->err_at = at; return rc; }
        rec_start[res->n_recs] = at;
        rec_end[res->n_recs] = c.p;
        rec_db[res->n_recs] = st->db;
        res->n_recs++;
    }
}

int rr_rdbread_len(const uint8_t *buf, uint64_t bytes, uint64_t at, uint64_t *val, uint64_t *end) {
    if (!val || !end || (bytes && !buf) || at > bytes) return RR_API_EINVAL;
    cur c = {buf, bytes, at};
    const int rc = c_count(&c, val);
    if (rc) return rc;
    *end = c.p;
    return RR_RDBREAD_DONE;
}

/* lzf_decompress (lzf_d.c:59-188) with CHECK_INPUT: 1 when in[0, clen) gives exactly ulen bytes.
 * out == NULL: the check alone. */
static int lzf_expand(const uint8_t *in, uint64_t clen, uint8_t *out, uint64_t ulen) {
    uint64_t ip = 0, op = 0;
    if (clen == 0) return 0;
    do {
        uint32_t ctrl = in[ip++];
        if (ctrl < 32) {                                   /* :72 a literal run */
            const uint64_t run = ctrl + 1;
            if (run > ulen - op) return 0;                 /* :76 */
            if (run > clen - ip) return 0;                 /* :83 */
            if (out) memcpy(out + op, in + ip, run);
            ip += run;
            op += run;
        } else {                                           /* :106 a back reference */
            uint64_t l = ctrl >> 5;
            if (ip >= clen) return 0;                      /* :113 */
            if (l == 7) {
                l += in[ip++];                             /* :121 */
                if (ip >= clen) return 0;                  /* :123 */
            }
            const uint64_t off = ((uint64_t)(ctrl & 0x1F) << 8) + 1 + in[ip++];   /* :110, :131 */
            if (l + 2 > ulen - op) return 0;               /* :133 */
            if (off > op) return 0;                        /* :139 */
            if (out)
                for (uint64_t k = 0; k < l + 2; k++) out[op + k] = out[op + k - off];   /* octet by octet: overlap allowed */
            op += l + 2;
        }
    } while (ip < clen);                                   /* :185 */
    return op == ulen;
}

int rr_rdbread_string(const uint8_t *buf, uint64_t bytes, uint64_t at, uint8_t *out, uint64_t out_cap, uint64_t *len,
                      uint64_t *end) {
    if (!len || !end || (bytes && !buf) || at > bytes || (out_cap && !out)) return RR_API_EINVAL;
    cur c = {buf, bytes, at};
    int ie, rc;
    uint64_t v;
    if ((rc = c_len(&c, &ie, &v))) return rc;
    if (!ie) {                                             /* rdb.c:519-539 */
        const uint64_t from = c.p;
        if ((rc = c_skip(&c, v))) return rc;
        *len = v;
        *end = c.p;
        if (v > out_cap) return RR_E_CAPACITY;
        if (v) memcpy(out, buf + from, v);
        return RR_RDBREAD_DONE;
    }
    if (v <= 2) {                                          /* rdbLoadIntegerObject, :266-302 */
        const uint32_t w = 1u << v;
        const uint64_t from = c.p;
        if ((rc = c_skip(&c, w))) return rc;
        uint64_t x = 0;
        for (uint32_t k = 0; k < w; k++) x |= (uint64_t)buf[from + k] << (8 * k);
        const int64_t iv = w == 1 ? (int64_t)(int8_t)x : w == 2 ? (int64_t)(int16_t)x : (int64_t)(int32_t)x;
        char tmp[24];                                      /* ll2string */
        uint64_t a = iv < 0 ? 0ull - (uint64_t)iv : (uint64_t)iv;
        uint32_t q = sizeof tmp;
        do { tmp[--q] = (char)('0' + a % 10); a /= 10; } while (a);
        if (iv < 0) tmp[--q] = '-';
        *len = sizeof tmp - q;
        *end = c.p;
        if (*len > out_cap) return RR_E_CAPACITY;
        memcpy(out, tmp + q, *len);
        return RR_RDBREAD_DONE;
    }
    if (v != 3) return RR_RDBREAD_E_LEN;                   /* :512 */
    uint64_t clen, ulen;
    if ((rc = c_count(&c, &clen))) return rc;              /* rdbLoadLzfStringObject, :369-407 */
    if ((rc = c_count(&c, &ulen))) return rc;
    const uint64_t from = c.p;
    if ((rc = c_skip(&c, clen))) return rc;
    *len = ulen;
    *end = c.p;
    if (ulen >= 0x7FFFFFF0ull || !lzf_expand(buf + from, clen, NULL, ulen)) return RR_RDBREAD_E_KEY;
    if (ulen > out_cap) return RR_E_CAPACITY;
    lzf_expand(buf + from, clen, out, ulen);
    return RR_RDBREAD_DONE;
}

#ifndef RR_RDBREAD_HOST_ONLY
/* ---- the device calls ---------------------------------------------------------------------------- */
#include "rr_internal.h"

#define fail rr_fail

int rr_rdbread_split(rr_ctx *c, const uint8_t *data, uint64_t data_cap, const uint64_t *rec_start, const uint64_t *rec_end,
                     uint64_t n, uint32_t version, rr_rdbread_out *out, rr_rdbfile_result *d_result, void *stream) {
    if (!c || !out || !d_result) return fail(RR_API_EINVAL, "NULL argument");
    if (version < 1 || version > RR_RDB_VERSION) return fail(RR_API_EINVAL, "rr_rdbread_split: version %u", version);
    if (n >= RR_MAX_VALUES / 2) return fail(RR_API_EINVAL, "batch too large");
    if (out->keys.n != n || out->payloads.n != n) return fail(RR_API_EINVAL, "keys.n, payloads.n != n");
    if (!out->keys.offsets || !out->payloads.offsets) return fail(RR_API_EINVAL, "NULL offsets");
    if (n && (!rec_start || !rec_end || !out->types || !out->expires || !out->idle || !out->freq || !out->status))
        return fail(RR_API_EINVAL, "NULL buffer");
    if ((data_cap && !data) || (out->keys.data_cap && !out->keys.data) || (out->payloads.data_cap && !out->payloads.data))
        return fail(RR_API_EINVAL, "NULL buffer");
    HIPCHK(hipSetDevice(c->device));
    int rc = rr_ensure_scratch(c, rr_rdbread_scratch_words(n), (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(rr_launch_rdbread_split(data, data_cap, rec_start, rec_end, n, out, c->scratch, d_result, (hipStream_t)stream));
    return rr_mark_scratch(c, (hipStream_t)stream);
}

int rr_rdbread_verify(rr_ctx *c, const uint8_t *data, uint64_t data_cap, uint64_t eof_at, uint64_t *d_state,
                      rr_rdbfile_result *d_result, void *stream) {
    if (!c || !data || !d_state || !d_result) return fail(RR_API_EINVAL, "NULL argument");
    if (data_cap < 9 || eof_at > data_cap - 9) return fail(RR_API_EINVAL, "rr_rdbread_verify: no 9 bytes at eof_at");
    HIPCHK(hipSetDevice(c->device));
    int rc = rr_ensure_scratch(c, rr_crc64_scratch_words(), (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(rr_launch_crc64(data, eof_at + 1, d_state, c->scratch, (hipStream_t)stream));
    HIPCHK(rr_launch_rdbread_verdict(data + eof_at + 1, eof_at + 9, d_state, d_result, (hipStream_t)stream));
    return rr_mark_scratch(c, (hipStream_t)stream);
}

/* ---- host-pointer forms ---------------------------------------------------------------------------- */
static uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

int rr_rdbread_split_host(rr_ctx *c, const uint8_t *data, uint64_t data_cap, const uint64_t *rec_start,
                          const uint64_t *rec_end, uint64_t n, uint32_t version, rr_rdbread_out *out,
                          rr_rdbfile_result *result) {
    if (!c || !out || !out->keys.offsets || !out->payloads.offsets) return fail(RR_API_EINVAL, "NULL argument");
    if (n && (!rec_start || !rec_end || !out->types || !out->expires || !out->idle || !out->freq || !out->status))
        return fail(RR_API_EINVAL, "NULL buffer");
    if ((data_cap && !data) || (out->keys.data_cap && !out->keys.data) || (out->payloads.data_cap && !out->payloads.data))
        return fail(RR_API_EINVAL, "NULL buffer");
    HIPCHK(hipSetDevice(c->device));
    /* d_vals: result | expires | idle | rec_start | rec_end | freq | types | status */
    const uint64_t o_exp = 32, o_idle = o_exp + 8 * n, o_rs = o_idle + 8 * n, o_re = o_rs + 8 * n, o_freq = o_re + 8 * n,
                   o_types = o_freq + 2 * n, o_status = o_types + n;
    const uint64_t kcap = out->keys.data_cap, pcap = out->payloads.data_cap;
    GROW(c->d_in, c->c_in, data_cap + 16);
    GROW(c->d_vals, c->c_vals, up16(o_status + n) + 16);
    GROW(c->d_arena, c->c_arena, kcap + 16);
    GROW(c->d_elems, c->c_elems, (n + 1) * sizeof(uint64_t));
    GROW(c->d_out, c->c_out, pcap + 16);
    GROW(c->d_ooff, c->c_ooff, (n + 1) * sizeof(uint64_t));
    uint8_t *v = (uint8_t *)c->d_vals;
    UP(c->d_in, data, data_cap);
    UP(v + o_rs, rec_start, 8 * n);
    UP(v + o_re, rec_end, 8 * n);
    rr_rdbread_out d = {{(uint8_t *)c->d_arena, (uint64_t *)c->d_elems, n, kcap}, {(uint8_t *)c->d_out, (uint64_t *)c->d_ooff, n, pcap},
                        v + o_types, (int64_t *)(v + o_exp), (uint64_t *)(v + o_idle), (int16_t *)(v + o_freq), v + o_status};
    int rc = rr_rdbread_split(c, (const uint8_t *)c->d_in, data_cap, (const uint64_t *)(v + o_rs), (const uint64_t *)(v + o_re), n,
                              version, &d, (rr_rdbfile_result *)v, c->stream);
    if (rc) return rc;
    rr_rdbfile_result r;
    DOWN(&r, v, sizeof r);
    DOWN(out->keys.offsets, c->d_elems, (n + 1) * sizeof(uint64_t));
    DOWN(out->payloads.offsets, c->d_ooff, (n + 1) * sizeof(uint64_t));
    DOWN(out->types, v + o_types, n);
    DOWN(out->expires, v + o_exp, 8 * n);
    DOWN(out->idle, v + o_idle, 8 * n);
    DOWN(out->freq, v + o_freq, 2 * n);
    DOWN(out->status, v + o_status, n);
    rc = rr_host_finish(c, "rdbread split", &r.bytes, out->payloads.data, c->d_out, pcap);
    if (rc) return rc;
    const uint64_t kb = out->keys.offsets[n];
    DOWN(out->keys.data, c->d_arena, kb < kcap ? kb : kcap);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (result) *result = r;
    return RR_API_OK;
}

int rr_rdbread_verify_host(rr_ctx *c, const uint8_t *data, uint64_t data_cap, uint64_t eof_at, uint64_t *state,
                           rr_rdbfile_result *result) {
    if (!c || !data || !state) return fail(RR_API_EINVAL, "NULL argument");
    if (data_cap < 9 || eof_at > data_cap - 9) return fail(RR_API_EINVAL, "rr_rdbread_verify: no 9 bytes at eof_at");
    HIPCHK(hipSetDevice(c->device));
    GROW(c->d_in, c->c_in, eof_at + 9 + 16);
    GROW(c->d_vals, c->c_vals, 64);   /* result | state[2] */
    uint8_t *v = (uint8_t *)c->d_vals;
    UP(c->d_in, data, eof_at + 9);
    UP(v + 32, state, 16);
    int rc = rr_rdbread_verify(c, (const uint8_t *)c->d_in, eof_at + 9, eof_at, (uint64_t *)(v + 32), (rr_rdbfile_result *)v, c->stream);
    if (rc) return rc;
    rr_rdbfile_result r;
    DOWN(&r, v, sizeof r);
    DOWN(state, v + 32, 16);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (result) *result = r;
    return RR_API_OK;
}
#endif /* RR_RDBREAD_HOST_ONLY */
