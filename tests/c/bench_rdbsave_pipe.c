/*
 * bench_rdbsave_pipe.c — keys/s of the snapshot pipes' three batch modes over the same pipes and
 * the same in-memory store (a generated batch, include/rr_serdes.h rr_gen_batch): the pipelined RAW
 * batch (rr_rdb_request_batch), FLAT (rr_rdb_request_flat) and SAVE (rr_rdbsave_request).  Each leg
 * ends when the child holds the answer in memory: blobs, the flat batch, or the RDB payloads.  Only
 * SAVE's answer is final — the child writes it to the rio as it is; after RAW or FLAT it still has
 * to build (and for RAW, parse) every robj before rdbSaveObject (DESIGN.md §11 times those legs with
 * the object built, `tests/test_compat.py bench`).
 * Usage: bench_rdbsave_pipe [config, default 4] [keys, default 100000] [keys per request, default 4096]
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "rr_rdb.h"
#include "rr_rdbsave.h"

static rr_host_batch gen;

static int store_get(void *user, size_t k, const int *dbis, const char *const *keys, const size_t *lens, void **vals,
                     size_t *vlens) {
    (void)user; (void)dbis;
    for (size_t i = 0; i < k; i++) {
        char buf[32];
        const size_t l = lens[i] < sizeof buf - 1 ? lens[i] : sizeof buf - 1;
        memcpy(buf, keys[i], l);
        buf[l] = 0;
        const uint64_t j = strtoull(buf + 2, NULL, 10) % gen.n;
        vlens[i] = gen.offsets[j + 1] - gen.offsets[j];
        vals[i] = malloc(vlens[i] ? vlens[i] : 1);
        memcpy(vals[i], gen.data + gen.offsets[j], vlens[i]);
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
static double now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + t.tv_nsec * 1e-9; }

int main(int argc, char **argv) {
    const int config = argc > 1 ? atoi(argv[1]) : 4;
    const size_t k = argc > 2 ? strtoull(argv[2], NULL, 10) : 100000;
    const size_t per = argc > 3 ? strtoull(argv[3], NULL, 10) : 4096;
    rr_ctx *ctx = NULL;
    if (rr_ctx_create(0, &ctx)) { printf("no GPU: %s\n", rr_last_error()); return 2; }
    if (rr_gen_batch(config, k, rr_gen_default_seed(config), &gen)) { printf("gen: %s\n", rr_last_error()); return 2; }
    char **keys = malloc(k * sizeof *keys);
    size_t *lens = malloc(k * sizeof *lens);
    int *dbis = malloc(k * sizeof *dbis);
    for (size_t i = 0; i < k; i++) {
        keys[i] = malloc(24);
        lens[i] = (size_t)snprintf(keys[i], 24, "k:%zu", i);
        dbis[i] = 3;
    }
    int a[2], b[2];
    if (pipe(a) || pipe(b)) { perror("pipe"); return 2; }
    server_t s = {a[0], b[1], ctx, 0};
    pthread_t th;
    pthread_create(&th, NULL, serve_thread, &s);
    const int fq = a[1], fr = b[0];
    int fails = 0;
    uint64_t save_bytes = 0, bad = 0;
    const char *names[3] = {"RAW batch (blobs in the child)", "FLAT (flat batch in the child)", "SAVE (RDB payloads in the child)"};
    printf("config %d, %zu keys, %llu blob bytes, %zu keys per request\n", config, k, (unsigned long long)gen.bytes, per);
    for (int round = 0; round < 2; round++) {          /* round 0 warms the context's buffers */
        for (int mode = 0; mode < 3; mode++) {
            const double t0 = now();
            for (size_t at = 0; at < k; at += per) {
                const size_t c = k - at < per ? k - at : per;
                int rc;
                if (mode == 0) {
                    rr_rdb_blobs r;
                    rc = rr_rdb_request_batch(fq, fr, dbis + at, (const char *const *)keys + at, lens + at, c, &r);
                    rr_rdb_blobs_free(&r);
                } else if (mode == 1) {
                    rr_rdb_flat r;
                    rc = rr_rdb_request_flat(fq, fr, dbis + at, (const char *const *)keys + at, lens + at, c, &r);
                    rr_rdb_flat_free(&r);
                } else {
                    rr_rdbsave_result r;
                    rc = rr_rdbsave_request(fq, fr, dbis + at, (const char *const *)keys + at, lens + at, c, &r);
                    if (rc == RR_API_OK && round) {
                        save_bytes += r.bytes;
                        for (uint64_t i = 0; i < r.n; i++) bad += r.status[i] != 0;
                    }
                    rr_rdbsave_result_free(&r);
                }
                if (rc != RR_API_OK) { printf("FAIL: %s: %s\n", names[mode], rr_last_error()); fails++; break; }
            }
            const double dt = now() - t0;
            if (round) printf("  %-36s %8.0f K keys/s  (%.1f ms)\n", names[mode], k / dt / 1e3, dt * 1e3);
        }
    }
    printf("  SAVE payload bytes %llu, values not saved %llu\n", (unsigned long long)save_bytes, (unsigned long long)bad);
    close(fq);
    pthread_join(th, NULL);
    printf("%d failures\n", fails + (s.rc != 0));
    return fails || s.rc ? 1 : 0;
}
