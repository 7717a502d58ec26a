/*
 * test_rdbsave_pipe.c — the SAVE request of rr_rdb_serve (RR_RDB_SAVE_TAG, include/rr_rdb.h) and
 * its child side rr_rdbsave_request (include/rr_rdbsave.h) over real pipes and an in-memory
 * snapshot store of the golden fixtures' valid blobs (fixtures.h, written by the Python test).
 *
 *   1. a RAW request, a SAVE request for 5000 keys, a RAW request again on the same pipes;
 *      the payloads equal rr_rdbsave_batch_host of the same blobs decoded by rr_decode_batch_host;
 *   2. a SAVE request with a missing key ends the service.
 * Exit status 0 when every check passes.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "rr_rdb.h"
#include "rr_rdbsave.h"
#include "fixtures.h"

static int fails;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf("FAIL: "); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const fixture_t *valid[N_FIXTURES];
static int nvalid;

static const fixture_t *fixture_of(const char *key, size_t len) {
    char buf[32];
    if (len < 3 || len >= sizeof buf || key[0] != 'k') return NULL;
    memcpy(buf, key, len);
    buf[len] = 0;
    const long i = strtol(buf + 2, NULL, 10);
    return i < 0 ? NULL : valid[i % nvalid];
}
static int store_get(void *user, size_t k, const int *dbis, const char *const *keys, const size_t *lens, void **vals,
                     size_t *vlens) {
    (void)user;
    for (size_t i = 0; i < k; i++) {
        const fixture_t *f = dbis[i] == 3 ? fixture_of(keys[i], lens[i]) : NULL;
        vals[i] = NULL;
        if (!f) continue;
        vals[i] = malloc(f->len ? f->len : 1);
        memcpy(vals[i], f->blob, f->len);
        vlens[i] = f->len;
    }
    return 0;
}

typedef struct { int rfd, wfd; rr_ctx *ctx; int rc; } server_t;
static void *serve_thread(void *a) {
    server_t *s = (server_t *)a;
    s->rc = rr_rdb_serve(s->rfd, s->wfd, store_get, free, NULL, s->ctx, 4096);
    close(s->wfd);
    return NULL;
}
static void start(server_t *s, int *fq, int *fr, rr_ctx *ctx, pthread_t *th) {
    int a[2], b[2];
    if (pipe(a) || pipe(b)) { perror("pipe"); exit(2); }
    s->rfd = a[0]; s->wfd = b[1]; s->ctx = ctx; s->rc = 0;
    *fq = a[1];
    *fr = b[0];
    pthread_create(th, NULL, serve_thread, s);
}
static void stop(server_t *s, int fq, int fr, pthread_t th) {
    close(fq);
    pthread_join(th, NULL);
    close(fr);
    close(s->rfd);
}

static void check_raw(int fq, int fr, char **keys, size_t *lens, int *dbis, size_t k, const char *what) {
    rr_rdb_blobs b;
    const int rc = rr_rdb_request_batch(fq, fr, dbis, (const char *const *)keys, lens, k, &b);
    CHECK(rc == RR_API_OK && b.n == k, "%s: rc %d", what, rc);
    for (size_t i = 0; rc == RR_API_OK && i < k; i++) {
        const fixture_t *f = fixture_of(keys[i], lens[i]);
        if (b.offsets[i + 1] - b.offsets[i] != f->len || memcmp(b.data + b.offsets[i], f->blob, f->len)) {
            CHECK(0, "%s: value %zu differs", what, i);
            break;
        }
    }
    rr_rdb_blobs_free(&b);
}

int main(void) {
    for (int i = 0; i < N_FIXTURES; i++)
        if (FIXTURES[i].status == 0) valid[nvalid++] = &FIXTURES[i];
    rr_ctx *serve_ctx = NULL, *ctx = NULL;
    if (rr_ctx_create(0, &serve_ctx) || rr_ctx_create(0, &ctx)) { printf("no GPU: %s\n", rr_last_error()); return 2; }
    const size_t k = 5000;
    char **keys = malloc(k * sizeof *keys);
    size_t *lens = malloc(k * sizeof *lens);
    int *dbis = malloc(k * sizeof *dbis);
    for (size_t i = 0; i < k; i++) {
        keys[i] = malloc(24);
        lens[i] = (size_t)snprintf(keys[i], 24, "k:%zu", i);
        dbis[i] = 3;
    }

    /* 1. RAW, SAVE, RAW on one pair of pipes */
    server_t s;
    pthread_t th;
    int fq, fr;
    start(&s, &fq, &fr, serve_ctx, &th);
    check_raw(fq, fr, keys, lens, dbis, 300, "RAW before SAVE");
    rr_rdbsave_result res;
    int rc = rr_rdbsave_request(fq, fr, dbis, (const char *const *)keys, lens, k, &res);
    CHECK(rc == RR_API_OK && res.n == k, "SAVE request: rc %d (%s)", rc, rr_last_error());
    check_raw(fq, fr, keys, lens, dbis, 300, "RAW after SAVE");
    stop(&s, fq, fr, th);
    CHECK(s.rc == 0, "service exit %d", s.rc);

    if (rc == RR_API_OK && res.n == k) {
        /* the same blobs through the host calls */
        uint64_t *offs = malloc((k + 1) * sizeof *offs), bytes = 0;
        offs[0] = 0;
        for (size_t i = 0; i < k; i++) offs[i + 1] = bytes += fixture_of(keys[i], lens[i])->len;
        uint8_t *data = calloc(bytes + 32, 1), *arena = malloc(bytes + 32);
        for (size_t i = 0; i < k; i++) memcpy(data + offs[i], fixture_of(keys[i], lens[i])->blob, offs[i + 1] - offs[i]);
        const uint64_t ecap = rr_decode_elem_bound(k, bytes);
        rr_value *vals = malloc(k * sizeof *vals);
        rr_elem *els = malloc((ecap ? ecap : 1) * sizeof *els);
        rr_totals t, st;
        rc = rr_decode_batch_host(ctx, data, offs, k, vals, els, ecap, arena, &t);
        CHECK(rc == RR_API_OK, "decode: %s", rr_last_error());
        const uint64_t cap = rr_rdbsave_bound(k, t.n_elems, bytes);
        uint8_t *out = malloc(cap + 16), *ty = malloc(k), *sts = malloc(k);
        uint64_t *oo = malloc((k + 1) * sizeof *oo);
        rc = rr_rdbsave_batch_host(ctx, vals, els, t.n_elems, arena, bytes, k, NULL, out, cap, oo, ty, sts, &st);
        CHECK(rc == RR_API_OK, "rdbsave host: %s", rr_last_error());
        CHECK(st.n_bad == 0 && st.bytes == oo[k] && st.bytes > k, "host totals: bad %llu bytes %llu",
              (unsigned long long)st.n_bad, (unsigned long long)st.bytes);
        CHECK(res.bytes == oo[k], "bytes %llu vs %llu", (unsigned long long)res.bytes, (unsigned long long)oo[k]);
        CHECK(!memcmp(res.offsets, oo, (k + 1) * sizeof *oo), "offsets differ");
        CHECK(!memcmp(res.types, ty, k) && !memcmp(res.status, sts, k), "types / status differ");
        CHECK(res.bytes == oo[k] && !memcmp(res.data, out, oo[k]), "payloads differ");
        for (size_t i = 0; i < k; i++)
            if (res.types[i] != fixture_of(keys[i], lens[i])->blob[0] || res.status[i] != 0) { CHECK(0, "value %zu: type / status", i); break; }
        free(offs); free(data); free(arena); free(vals); free(els); free(out); free(ty); free(sts); free(oo);
    }
    rr_rdbsave_result_free(&res);

    /* 2. a missing key ends the service */
    start(&s, &fq, &fr, serve_ctx, &th);
    dbis[7] = 4;   /* no such database in the store */
    rc = rr_rdbsave_request(fq, fr, dbis, (const char *const *)keys, lens, 20, &res);
    CHECK(rc != RR_API_OK, "missing key: request succeeded");
    stop(&s, fq, fr, th);
    CHECK(s.rc != 0, "missing key: service exit %d", s.rc);

    rr_ctx_destroy(ctx);
    rr_ctx_destroy(serve_ctx);
    printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
