/*
 * rr_rdbfile_api.c — host layer of include/rr_rdbfile.h: the host helpers that need no GPU (the
 * CRC-64 over tables generated from the polynomial, the stream's head and the SELECTDB / RESIZEDB
 * opcodes), then argument checks, the context's scratch and the host-pointer forms of the device
 * calls.  RR_RDBFILE_HOST_ONLY compiles the helpers alone (a stand-alone check needs no HIP).
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rr_rdbfile.h"

/* ---- CRC-64 "Jones" (crc64.c:1-12): reflected, init 0, no final xor ---------------------------- */
#define CRC_POLY 0x95ac9329ac4bc9b5ull   /* 0xad93d23594c935a9 bit-reversed */
#define GF_ONE   (1ull << 63)            /* x^0: bit 63 - i is the coefficient of x^i */

static uint64_t crc_tab[8][256];         /* [k][b]: the state after byte b and k zero bytes */
static uint64_t crc_pow[64];             /* x^(8 * 2^k) mod P */
static pthread_once_t crc_once = PTHREAD_ONCE_INIT;

static inline uint64_t gf_mulx(uint64_t a) { return (a >> 1) ^ (CRC_POLY & (0ull - (a & 1))); }

uint64_t rr_crc64_mul(uint64_t a, uint64_t b) {
    uint64_t r = 0;
    for (int i = 0; i < 64; i++) {
        r ^= a & (0ull - (b >> 63));
        b <<= 1;
        a = gf_mulx(a);
    }
    return r;
}

static void crc_build(void) {
    for (unsigned b = 0; b < 256; b++) {
        uint64_t c = b;
        for (int i = 0; i < 8; i++) c = gf_mulx(c);
        crc_tab[0][b] = c;
    }
    for (int k = 1; k < 8; k++)
        for (unsigned b = 0; b < 256; b++) {
            const uint64_t c = crc_tab[k - 1][b];
            crc_tab[k][b] = crc_tab[0][c & 0xFF] ^ (c >> 8);
        }
    uint64_t p = GF_ONE;
    for (int i = 0; i < 8; i++) p = gf_mulx(p);
    for (int k = 0; k < 64; k++) {
        crc_pow[k] = p;
        p = rr_crc64_mul(p, p);
    }
}
static void crc_init(void) { pthread_once(&crc_once, crc_build); }

uint64_t rr_crc64(uint64_t crc, const void *ptr, uint64_t len) {
    crc_init();
    const uint8_t *p = (const uint8_t *)ptr;
    for (; len >= 8; len -= 8, p += 8) {
        uint64_t w;
        memcpy(&w, p, 8);
#if __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
        w = __builtin_bswap64(w);
#endif
        crc ^= w;
        crc = crc_tab[7][crc & 0xFF] ^ crc_tab[6][(crc >> 8) & 0xFF] ^ crc_tab[5][(crc >> 16) & 0xFF] ^
              crc_tab[4][(crc >> 24) & 0xFF] ^ crc_tab[3][(crc >> 32) & 0xFF] ^ crc_tab[2][(crc >> 40) & 0xFF] ^
              crc_tab[1][(crc >> 48) & 0xFF] ^ crc_tab[0][crc >> 56];
    }
    for (; len; len--) crc = crc_tab[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
    return crc;
}

uint64_t rr_crc64_shift(uint64_t crc, uint64_t n) {
    crc_init();
    for (int k = 0; n; n >>= 1, k++)
        if (n & 1) crc = rr_crc64_mul(crc, crc_pow[k]);
    return crc;
}

/* ---- the writers ----------------------------------------------------------------------------------- */
typedef struct wbuf { uint8_t *buf; uint64_t cap, n; } wbuf;   /* counts always, writes what fits */

static void w_bytes(wbuf *w, const void *p, uint64_t len) {
    if (w->buf && w->n + len <= w->cap) memcpy(w->buf + w->n, p, len);
    w->n += len;
}
static void w_byte(wbuf *w, uint8_t b) { w_bytes(w, &b, 1); }

static void w_len(wbuf *w, uint64_t len) {   /* rdbSaveLen, rdb.c:147-178 */
    uint8_t b[9];
    if (len < 64) { b[0] = (uint8_t)len; w_bytes(w, b, 1); }
    else if (len < 16384) { b[0] = (uint8_t)(0x40 | (len >> 8)); b[1] = (uint8_t)len; w_bytes(w, b, 2); }
    else if (len <= 0xFFFFFFFFull) {
        b[0] = 0x80;
        for (int k = 0; k < 4; k++) b[1 + k] = (uint8_t)(len >> (8 * (3 - k)));
        w_bytes(w, b, 5);
    } else {
        b[0] = 0x81;
        for (int k = 0; k < 8; k++) b[1 + k] = (uint8_t)(len >> (8 * (7 - k)));
        w_bytes(w, b, 9);
    }
}

/* rdbTryIntegerEncoding (rdb.c:307-321): the canonical decimal of an int32, up to 11 bytes */
static int try_int(const char *s, uint64_t len, int64_t *out) {
    if (len == 0 || len > 11) return 0;
    char buf[24];
    memcpy(buf, s, len);
    buf[len] = 0;
    char *end;
    const long long v = strtoll(buf, &end, 10);
    if (end != buf + len) return 0;   /* (an embedded NUL ends it early too) */
    char back[24];
    const int bl = snprintf(back, sizeof back, "%lld", v);
    if ((uint64_t)bl != len || memcmp(back, s, len)) return 0;
    if (v < -2147483648ll || v > 2147483647ll) return 0;
    *out = v;
    return 1;
}

static void w_rawstring(wbuf *w, const char *s, uint64_t len) {   /* rdbSaveRawString, rdb.c:411-441 */
    int64_t v;
    if (try_int(s, len, &v)) {                                    /* rdbEncodeInteger :241-261 */
        uint8_t b[5];
        const int nb = v >= -128 && v <= 127 ? 1 : v >= -32768 && v <= 32767 ? 2 : 4;
        b[0] = (uint8_t)(0xC0 | (nb == 1 ? 0 : nb == 2 ? 1 : 2));
        for (int k = 0; k < nb; k++) b[1 + k] = (uint8_t)((uint64_t)v >> (8 * k));
        w_bytes(w, b, 1 + (uint64_t)nb);
        return;
    }
    w_len(w, len);
    w_bytes(w, s, len);
}

static void w_aux(wbuf *w, const char *key, const char *val) {    /* rdbSaveAuxField, rdb.c:1076-1085 */
    w_byte(w, 0xFA);
    w_rawstring(w, key, strlen(key));
    w_rawstring(w, val, strlen(val));
}
static void w_aux_int(wbuf *w, const char *key, long long v) {    /* rdbSaveAuxFieldStrInt :1094-1098 */
    char buf[24];
    snprintf(buf, sizeof buf, "%lld", v);
    w_aux(w, key, buf);
}

uint64_t rr_rdbfile_head(uint8_t *buf, uint64_t cap, const char *ver, int64_t ctime, uint64_t used_mem,
                         const rr_rdbfile_repl *repl, int aof_preamble) {
    wbuf c = {NULL, 0, 0};   /* first the size, then the bytes when they fit */
    for (int pass = 0; pass < 2; pass++) {
        char magic[10];
        snprintf(magic, sizeof magic, "REDIS%04d", RR_RDB_VERSION);   /* rdb.c:1180 */
        w_bytes(&c, magic, 9);
        w_aux(&c, "redis-ver", ver ? ver : "");                       /* :1106-1109 */
        w_aux_int(&c, "redis-bits", 64);
        w_aux_int(&c, "ctime", ctime);
        w_aux_int(&c, "used-mem", (long long)used_mem);
        if (repl) {                                                   /* :1112-1119 */
            w_aux_int(&c, "repl-stream-db", repl->stream_db);
            w_aux(&c, "repl-id", repl->replid ? repl->replid : "");
            w_aux_int(&c, "repl-offset", repl->offset);
        }
        w_aux_int(&c, "aof-preamble", aof_preamble != 0);             /* :1120 */
        if (pass || !buf || c.n > cap) break;
        c.buf = buf;
        c.cap = cap;
        c.n = 0;
    }
    return c.n;
}

uint64_t rr_rdbfile_selectdb(uint8_t *buf, uint64_t cap, uint64_t dbid, uint64_t db_size, uint64_t expires_size) {
    uint8_t tmp[32];
    wbuf c = {tmp, sizeof tmp, 0};
    w_byte(&c, 0xFE);                                                 /* rdb.c:1193-1194 */
    w_len(&c, dbid);
    w_byte(&c, 0xFB);                                                 /* :1203-1205 */
    w_len(&c, db_size > 0xFFFFFFFFull ? 0xFFFFFFFFull : db_size);
    w_len(&c, expires_size > 0xFFFFFFFFull ? 0xFFFFFFFFull : expires_size);
    if (buf && c.n <= cap) memcpy(buf, tmp, c.n);
    return c.n;
}

uint64_t rr_rdbfile_bound(uint64_t n, uint64_t key_bytes, uint64_t payload_bytes, uint64_t head_bytes) {
    return (head_bytes + 27 * n + key_bytes + payload_bytes + 9 + 15) & ~15ull;
}

#ifndef RR_RDBFILE_HOST_ONLY
/* ---- the device calls ---------------------------------------------------------------------------- */
#include "rr_internal.h"

#define fail rr_fail
#define RDBFILE_FLAGS (RR_RDBFILE_IDLE | RR_RDBFILE_FREQ | RR_RDBFILE_EOF | RR_RDBFILE_NO_CKSUM)

int rr_rdbfile_section(rr_ctx *c, const rr_rdbfile_in *in, uint32_t flags, uint8_t *out, uint64_t out_cap,
                       uint64_t *rec_offsets, uint8_t *rec_status, uint64_t *d_state, rr_rdbfile_result *d_result,
                       void *stream) {
    if (!c || !in || !rec_offsets || !d_state || !d_result) return fail(RR_API_EINVAL, "NULL argument");
    if (flags & ~RDBFILE_FLAGS) return fail(RR_API_EINVAL, "rr_rdbfile_section: unknown flag");
    const uint64_t n = in->payloads.n;
    if (in->keys.n != n) return fail(RR_API_EINVAL, "keys.n != payloads.n");
    if (n >= RR_MAX_VALUES) return fail(RR_API_EINVAL, "batch too large (value indices are 32-bit)");
    if (!in->payloads.offsets || !in->keys.offsets) return fail(RR_API_EINVAL, "NULL offsets");
    if (n && (!in->types || !in->status || !rec_status)) return fail(RR_API_EINVAL, "NULL buffer");
    if ((in->payloads.data_cap && !in->payloads.data) || (in->keys.data_cap && !in->keys.data) || (in->head_bytes && !in->head) ||
        (out_cap && !out))
        return fail(RR_API_EINVAL, "NULL buffer");
    if (n && (((flags & RR_RDBFILE_IDLE) && !in->idle) || ((flags & RR_RDBFILE_FREQ) && !in->freq)))
        return fail(RR_API_EINVAL, "RR_RDBFILE_IDLE / RR_RDBFILE_FREQ without the array");
    if ((uintptr_t)out & 15) return fail(RR_API_EINVAL, "out must be 16-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    int rc = rr_ensure_scratch(c, rr_rdbfile_scratch_words(n), (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(rr_launch_rdbfile(in, flags, out, out_cap, rec_offsets, rec_status, d_state, d_result, c->scratch, (hipStream_t)stream));
    return rr_mark_scratch(c, (hipStream_t)stream);
}

int rr_crc64_device(rr_ctx *c, const uint8_t *data, uint64_t bytes, uint64_t *d_state, void *stream) {
    if (!c || !d_state || (bytes && !data)) return fail(RR_API_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    int rc = rr_ensure_scratch(c, rr_crc64_scratch_words(), (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(rr_launch_crc64(data, bytes, d_state, c->scratch, (hipStream_t)stream));
    return rr_mark_scratch(c, (hipStream_t)stream);
}

int rr_rdbdump_batch(rr_ctx *c, const rr_blob_batch *in, const uint8_t *types, const uint8_t *status, rr_blob_batch *out,
                     uint8_t *out_status, rr_rdbfile_result *d_result, void *stream) {
    int rc = rr_check_blob_io(c, in, out, d_result, types && status && out_status);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    rc = rr_ensure_scratch(c, rr_rdbdump_scratch_words(in->n), (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(rr_launch_rdbdump(in->data, in->data_cap, in->offsets, types, status, in->n, out->data, out->data_cap, out->offsets,
                             out_status, c->scratch, d_result, (hipStream_t)stream));
    return rr_mark_scratch(c, (hipStream_t)stream);
}

int rr_rdbdump_verify_batch(rr_ctx *c, const rr_blob_batch *in, rr_blob_batch *out, uint8_t *types, uint8_t *status,
                            rr_rdbfile_result *d_result, void *stream) {
    int rc = rr_check_blob_io(c, in, out, d_result, types && status);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    rc = rr_ensure_scratch(c, rr_rdbdump_scratch_words(in->n), (hipStream_t)stream);
    if (rc) return rc;
    HIPCHK(rr_launch_rdbdump_verify(in->data, in->data_cap, in->offsets, in->n, out->data, out->data_cap, out->offsets, types,
                                    status, c->scratch, d_result, (hipStream_t)stream));
    return rr_mark_scratch(c, (hipStream_t)stream);
}

/* ---- host-pointer forms ---------------------------------------------------------------------------- */
static uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

int rr_rdbfile_section_host(rr_ctx *c, const rr_rdbfile_in *in, uint32_t flags, uint8_t *out, uint64_t out_cap,
                            uint64_t *rec_offsets, uint8_t *rec_status, uint64_t *state, rr_rdbfile_result *result) {
    if (!c || !in || !rec_offsets || !state) return fail(RR_API_EINVAL, "NULL argument");
    const uint64_t n = in->payloads.n;
    if (!in->payloads.offsets || !in->keys.offsets || in->keys.n != n) return fail(RR_API_EINVAL, "bad batch");
    if (n && (!in->types || !in->status || !rec_status)) return fail(RR_API_EINVAL, "NULL buffer");
    if (n && (((flags & RR_RDBFILE_IDLE) && !in->idle) || ((flags & RR_RDBFILE_FREQ) && !in->freq)))
        return fail(RR_API_EINVAL, "RR_RDBFILE_IDLE / RR_RDBFILE_FREQ without the array");
    if ((in->head_bytes && !in->head) || (out_cap && !out)) return fail(RR_API_EINVAL, "NULL buffer");
    const uint64_t pb = rr_reach(in->payloads.offsets, n, in->payloads.data_cap), kb = rr_reach(in->keys.offsets, n, in->keys.data_cap);
    if ((pb && !in->payloads.data) || (kb && !in->keys.data)) return fail(RR_API_EINVAL, "NULL buffer");
    HIPCHK(hipSetDevice(c->device));
    /* d_vals: expires | idle | state[2] | result | types | status | freq | rec_status | head */
    const uint64_t o_idle = 8 * n, o_state = 16 * n, o_res = o_state + 16, o_types = o_res + 32, o_status = o_types + n,
                   o_freq = o_status + n, o_rs = o_freq + n, o_head = up16(o_rs + n);
    GROW(c->d_in, c->c_in, pb + 16);
    GROW(c->d_off, c->c_off, (n + 1) * sizeof(uint64_t));
    GROW(c->d_arena, c->c_arena, kb + 16);
    GROW(c->d_elems, c->c_elems, (n + 1) * sizeof(uint64_t));
    GROW(c->d_vals, c->c_vals, o_head + in->head_bytes + 16);
    GROW(c->d_out, c->c_out, out_cap + 16);
    GROW(c->d_ooff, c->c_ooff, (n + 1) * sizeof(uint64_t));
    uint8_t *v = (uint8_t *)c->d_vals;
    UP(c->d_in, in->payloads.data, pb);
    UP(c->d_off, in->payloads.offsets, (n + 1) * sizeof(uint64_t));
    UP(c->d_arena, in->keys.data, kb);
    UP(c->d_elems, in->keys.offsets, (n + 1) * sizeof(uint64_t));
    if (in->expires) UP(v, in->expires, 8 * n);
    if (flags & RR_RDBFILE_IDLE) UP(v + o_idle, in->idle, 8 * n);
    UP(v + o_state, state, 16);
    UP(v + o_types, in->types, n);
    UP(v + o_status, in->status, n);
    if (flags & RR_RDBFILE_FREQ) UP(v + o_freq, in->freq, n);
    UP(v + o_head, in->head, in->head_bytes);
    const rr_rdbfile_in d = {{(uint8_t *)c->d_in, (uint64_t *)c->d_off, n, pb}, {(uint8_t *)c->d_arena, (uint64_t *)c->d_elems, n, kb},
                             v + o_types, v + o_status, in->expires ? (const int64_t *)v : NULL, (const uint64_t *)(v + o_idle),
                             v + o_freq, v + o_head, in->head_bytes};
    int rc = rr_rdbfile_section(c, &d, flags, (uint8_t *)c->d_out, out_cap, (uint64_t *)c->d_ooff, v + o_rs, (uint64_t *)(v + o_state),
                                (rr_rdbfile_result *)(v + o_res), c->stream);
    if (rc) return rc;
    rr_rdbfile_result r;
    DOWN(&r, v + o_res, sizeof r);
    DOWN(state, v + o_state, 16);
    DOWN(rec_offsets, c->d_ooff, (n + 1) * sizeof(uint64_t));
    DOWN(rec_status, v + o_rs, n);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (r.bytes == ~0ull) return fail(RR_API_EDEVICE, "rdbfile: device-side failure (look-back timeout)");
    if (r.status == RR_OK) DOWN(out, c->d_out, r.bytes);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (result) *result = r;
    return RR_API_OK;
}

int rr_rdbdump_batch_host(rr_ctx *c, const uint8_t *data, const uint64_t *offsets, const uint8_t *types, const uint8_t *status,
                          uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, uint8_t *out_status,
                          rr_rdbfile_result *result) {
    if (!c || !offsets || !out_offsets || (n && (!types || !status || !out_status)) || (out_cap && !out))
        return fail(RR_API_EINVAL, "NULL argument");
    const uint64_t nb = rr_reach(offsets, n, ~0ull);
    if (nb && !data) return fail(RR_API_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    GROW(c->d_in, c->c_in, nb + 16);
    GROW(c->d_off, c->c_off, (n + 1) * sizeof(uint64_t));
    GROW(c->d_vals, c->c_vals, 32 + 3 * n + 16);   /* result, types, status, out_status */
    GROW(c->d_out, c->c_out, out_cap + 16);
    GROW(c->d_ooff, c->c_ooff, (n + 1) * sizeof(uint64_t));
    uint8_t *v = (uint8_t *)c->d_vals;
    UP(c->d_in, data, nb);
    UP(c->d_off, offsets, (n + 1) * sizeof(uint64_t));
    UP(v + 32, types, n);
    UP(v + 32 + n, status, n);
    rr_blob_batch in = {(uint8_t *)c->d_in, (uint64_t *)c->d_off, n, nb};
    rr_blob_batch ob = {(uint8_t *)c->d_out, (uint64_t *)c->d_ooff, n, out_cap};
    int rc = rr_rdbdump_batch(c, &in, v + 32, v + 32 + n, &ob, v + 32 + 2 * n, (rr_rdbfile_result *)v, c->stream);
    if (rc) return rc;
    rr_rdbfile_result r;
    DOWN(&r, v, sizeof r);
    DOWN(out_offsets, c->d_ooff, (n + 1) * sizeof(uint64_t));
    DOWN(out_status, v + 32 + 2 * n, n);
    rc = rr_host_finish(c, "rdbdump", &r.bytes, out, c->d_out, out_cap);
    if (rc) return rc;
    if (result) *result = r;
    return RR_API_OK;
}

int rr_rdbdump_verify_batch_host(rr_ctx *c, const uint8_t *data, const uint64_t *offsets, uint64_t n, uint8_t *out,
                                 uint64_t out_cap, uint64_t *out_offsets, uint8_t *types, uint8_t *status,
                                 rr_rdbfile_result *result) {
    if (!c || !offsets || !out_offsets || (n && (!types || !status)) || (out_cap && !out))
        return fail(RR_API_EINVAL, "NULL argument");
    const uint64_t nb = rr_reach(offsets, n, ~0ull);
    if (nb && !data) return fail(RR_API_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    GROW(c->d_in, c->c_in, nb + 16);
    GROW(c->d_off, c->c_off, (n + 1) * sizeof(uint64_t));
    GROW(c->d_vals, c->c_vals, 32 + 2 * n + 16);   /* result, types, status */
    GROW(c->d_out, c->c_out, out_cap + 16);
    GROW(c->d_ooff, c->c_ooff, (n + 1) * sizeof(uint64_t));
    uint8_t *v = (uint8_t *)c->d_vals;
    UP(c->d_in, data, nb);
    UP(c->d_off, offsets, (n + 1) * sizeof(uint64_t));
    rr_blob_batch in = {(uint8_t *)c->d_in, (uint64_t *)c->d_off, n, nb};
    rr_blob_batch ob = {(uint8_t *)c->d_out, (uint64_t *)c->d_ooff, n, out_cap};
    int rc = rr_rdbdump_verify_batch(c, &in, &ob, v + 32, v + 32 + n, (rr_rdbfile_result *)v, c->stream);
    if (rc) return rc;
    rr_rdbfile_result r;
    DOWN(&r, v, sizeof r);
    DOWN(out_offsets, c->d_ooff, (n + 1) * sizeof(uint64_t));
    DOWN(types, v + 32, n);
    DOWN(status, v + 32 + n, n);
    rc = rr_host_finish(c, "rdbdump verify", &r.bytes, out, c->d_out, out_cap);
    if (rc) return rc;
    if (result) *result = r;
    return RR_API_OK;
}
#endif /* RR_RDBFILE_HOST_ONLY */
