/*
 * test_compat_zlraw.c — the compat shim's ziplist check (rr_compat_set_ziplist_check, the
 * environment's RR_COMPAT_ZL_CHECK) over the golden fixtures (fixtures.h, written by
 * tests/test_compat.py), linked with the minimal Redis model and the engine library.
 *
 *   default    no call: the environment unset or "1" -> the strict walk, today's behaviour: every
 *              fixture with a nonzero status panics, the others round-trip.
 *   env-off    no call, RR_COMPAT_ZL_CHECK=0 in the environment -> reference acceptance.
 *   call-off   rr_compat_set_ziplist_check(0) -> reference acceptance; then back on -> strict.
 *   gpu-off    call-off's checks on the GPU route too (GPU suite): objects equal the host route's.
 *   rdb        rr_compat_rdb_load_batch against a scripted parent (the FLAT response of rr_rdb.c
 *              written into the pipe by hand, decoded with the host codec in either mode): the
 *              ziplist check applied is this process's, whatever mode the parent decoded in.
 * Reference acceptance (rock_serdes.c:356-366, :455-466): a ziplist fixture the strict walk rejects
 * as RR_E_ZL_CORRUPT (status 10) yields an object whose ziplist is the blob's bytes 13.., and
 * serObject writes the blob back; a wrong byte count (status 9) still panics; every other fixture
 * behaves as before; rr_compat_des_batch matches the per-key results.
 * Exit status 0 when every check passes.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "server.h"
#include "rock_serdes_compat.h"
#include "fixtures.h"

static int fails;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf("FAIL %s: ", fx ? fx->name : "-"); printf(__VA_ARGS__); printf("\n"); } } while (0)

#define ST_ZL_LEN 9
#define ST_ZL_CORRUPT 10

static int is_ziplist(const fixture_t *fx) { return fx->len >= 13 && (fx->blob[0] == 12 || fx->blob[0] == 13); }
/* does the mode accept the fixture? */
static int accepted(const fixture_t *fx, int strict) {
    return fx->status == 0 || (!strict && fx->status == ST_ZL_CORRUPT && is_ziplist(fx));
}

static void *bufs[N_FIXTURES];
static size_t lens[N_FIXTURES], nok;
static const fixture_t *okfx[N_FIXTURES];
static robj *objs[N_FIXTURES];

/* every fixture through desObject / serObject; keeps the accepted ones' objects in objs.  Returns
 * the corrupt-ziplist fixtures accepted. */
static int per_key(const char *what, int strict, int *len_panics) {
    const fixture_t *fx = NULL;
    int raw_accepted = 0;
    nok = 0;
    *len_panics = 0;
    for (int i = 0; i < N_FIXTURES; i++) {
        fx = &FIXTURES[i];
        jmp_buf jb;
        mr_panic_jmp = &jb;
        robj *volatile o = NULL;
        if (setjmp(jb) == 0) {
            o = desObject((void *)fx->blob, fx->len);
        } else {
            CHECK(!accepted(fx, strict), "%s: desObject panicked on a blob this mode accepts: %s", what, mr_panic_msg);
            if (fx->status == ST_ZL_LEN) ++*len_panics;
            continue;
        }
        mr_panic_jmp = NULL;
        CHECK(accepted(fx, strict), "%s: desObject accepted a blob this mode rejects (status %d)", what, fx->status);
        if (!accepted(fx, strict)) continue;
        if (is_ziplist(fx)) {   /* the object's ziplist is the blob's bytes 13.. */
            CHECK(o->encoding == OBJ_ENCODING_ZIPLIST && o->type == (fx->blob[0] == 13 ? OBJ_HASH : OBJ_ZSET),
                  "%s: not a ziplist object", what);
            CHECK(!memcmp(o->ptr, fx->blob + 13, fx->len - 13), "%s: the ziplist bytes differ from the blob's", what);
        }
        sds s = serObject(o);
        CHECK(sdslen(s) == fx->out_len && !memcmp(s, fx->out, fx->out_len),
              "%s: serObject(desObject(b)) differs (%zu vs %zu bytes)", what, sdslen(s), fx->out_len);
        sdsfree(s);
        raw_accepted += fx->status == ST_ZL_CORRUPT;
        objs[nok] = o;
        bufs[nok] = (void *)fx->blob;
        lens[nok] = fx->len;
        okfx[nok++] = fx;
    }
    mr_panic_jmp = NULL;
    return raw_accepted;
}

/* rr_compat_des_batch over the accepted fixtures: blob for blob what the per-key calls built */
static void batch_matches(const char *what) {
    const fixture_t *fx = NULL;
    robj *b[N_FIXTURES];
    sds outs[N_FIXTURES];
    rr_compat_des_batch(bufs, lens, nok, b);
    rr_compat_ser_batch(b, nok, outs);
    for (size_t i = 0; i < nok; i++) {
        fx = okfx[i];
        CHECK(b[i]->type == objs[i]->type && b[i]->encoding == objs[i]->encoding && b[i]->lru == objs[i]->lru,
              "%s: batch object differs from the per-key one", what);
        if (is_ziplist(fx)) CHECK(!memcmp(b[i]->ptr, objs[i]->ptr, fx->len - 13), "%s: batch ziplist bytes differ", what);
        CHECK(sdslen(outs[i]) == fx->out_len && !memcmp(outs[i], fx->out, fx->out_len), "%s: batch round trip differs", what);
        sdsfree(outs[i]);
        decrRefCount(b[i]);
    }
}

static void drop(void) {
    for (size_t i = 0; i < nok; i++) decrRefCount(objs[i]);
    nok = 0;
}

static int count_status(int st) {
    int n = 0;
    for (int i = 0; i < N_FIXTURES; i++) n += FIXTURES[i].status == st && (st != ST_ZL_CORRUPT || is_ziplist(&FIXTURES[i]));
    return n;
}

/* One key restored through rr_compat_rdb_load_batch from a parent that decoded the blob with
 * `parent_flags` (the FLAT response: {n, n_elems, bytes}, records, descriptors, arena).  Returns 1
 * for an object whose ziplist is the blob's, 0 for a panic (its message in mr_panic_msg). */
static int rdb_restore(const fixture_t *fx, unsigned parent_flags) {
    int req[2], resp[2];
    if (pipe(req) || pipe(resp)) return -1;
    const uint64_t offs[2] = {0, fx->len};
    rr_value v;
    rr_elem el[64];
    uint8_t *arena = malloc(fx->len + 16);
    rr_totals t;
    if (rr_host_decode_batch_ex(fx->blob, offs, 1, &v, el, 64, arena, &t, parent_flags) != RR_API_OK) return -1;
    const uint64_t h[3] = {1, t.n_elems < 64 ? t.n_elems : 64, fx->len};
    if (write(resp[1], h, sizeof h) != (ssize_t)sizeof h || write(resp[1], &v, sizeof v) != (ssize_t)sizeof v ||
        write(resp[1], el, h[1] * sizeof(rr_elem)) != (ssize_t)(h[1] * sizeof(rr_elem)) ||
        write(resp[1], arena, fx->len) != (ssize_t)fx->len)
        return -1;
    free(arena);
    sds key = sdsnewlen("k", 1);
    robj *volatile o = NULL;
    jmp_buf jb;
    mr_panic_jmp = &jb;
    volatile int ok = 0;
    if (setjmp(jb) == 0) {
        robj *out = NULL;
        rr_compat_rdb_load_batch(req[1], resp[0], 0, &key, 1, &out);
        o = out;
        ok = o->encoding == OBJ_ENCODING_ZIPLIST && !memcmp(o->ptr, fx->blob + 13, fx->len - 13);
        decrRefCount(o);
    }
    mr_panic_jmp = NULL;
    sdsfree(key);
    close(req[0]); close(req[1]); close(resp[0]); close(resp[1]);
    return ok;
}

static int rdb_mode(void) {
    const fixture_t *fx = NULL;
    int n_corrupt = 0, n_good = 0;
    for (int i = 0; i < N_FIXTURES; i++) {
        fx = &FIXTURES[i];
        if (!is_ziplist(fx) || fx->len > 4000 || (fx->status != 0 && fx->status != ST_ZL_CORRUPT)) continue;
        const int corrupt = fx->status == ST_ZL_CORRUPT;
        n_corrupt += corrupt;
        n_good += !corrupt;
        for (unsigned parent = 0; parent <= RR_CTX_ZL_RAW; parent += RR_CTX_ZL_RAW) {
            rr_compat_set_ziplist_check(1);   /* strict here: a corrupt ziplist panics whatever the parent did */
            int got = rdb_restore(fx, parent);
            CHECK(got == !corrupt, "strict child, parent flags %u: %d", parent, got);
            if (corrupt && !got) CHECK(strstr(mr_panic_msg, "bad blob") != NULL, "strict child's panic: %s", mr_panic_msg);
            rr_compat_set_ziplist_check(0);   /* off here: accepted from a raw parent; a strict parent's
                                               * rejection cannot be undone and is named */
            got = rdb_restore(fx, parent);
            CHECK(got == (!corrupt || parent != 0), "check off, parent flags %u: %d", parent, got);
            if (corrupt && !parent) CHECK(strstr(mr_panic_msg, "RR_CTX_ZL_RAW") != NULL, "the pairing's panic: %s", mr_panic_msg);
        }
    }
    fx = NULL;
    CHECK(n_corrupt >= 1 && n_good >= 1, "%d corrupt and %d good ziplist fixtures", n_corrupt, n_good);
    printf("rdb restore: the child's ziplist check over %d corrupt and %d good ziplists, both parent modes; %d failures\n",
           n_corrupt, n_good, fails);
    return fails ? 1 : 0;
}

int main(int argc, char **argv) {
    setvbuf(stdout, NULL, _IONBF, 0);
    const char *mode = argc > 1 ? argv[1] : "default";
    if (!strcmp(mode, "rdb")) return rdb_mode();
    const fixture_t *fx = NULL;
    const int n_corrupt = count_status(ST_ZL_CORRUPT), n_len = count_status(ST_ZL_LEN);
    int lp = 0;
    CHECK(n_corrupt >= 1 && n_len >= 1, "the fixtures hold %d corrupt ziplists and %d wrong byte counts", n_corrupt, n_len);
    rr_compat_set_route(RR_COMPAT_ROUTE_HOST);
    if (!strcmp(mode, "default")) {   /* nothing set (or the environment says 1): the strict walk */
        const int got = per_key("default", 1, &lp);
        CHECK(got == 0 && lp == n_len, "strict: %d corrupt ziplists accepted, %d length panics", got, lp);
        batch_matches("default batch");
        drop();
        printf("ziplist check: strict (default), %d corrupt ziplists rejected; %d failures\n", n_corrupt, fails);
        return fails ? 1 : 0;
    }
    if (!strcmp(mode, "call-off") || !strcmp(mode, "gpu-off")) rr_compat_set_ziplist_check(0);
    int got = per_key(mode, 0, &lp);
    CHECK(got == n_corrupt && lp == n_len, "off: %d of %d corrupt ziplists accepted, %d of %d length panics", got, n_corrupt,
          lp, n_len);
    batch_matches("host batch");
    if (!strcmp(mode, "gpu-off")) {   /* the GPU route: the same objects (RR_CTX_ZL_RAW on the shim's context) */
        rr_compat_set_route(RR_COMPAT_ROUTE_GPU);
        batch_matches("gpu batch");
        jmp_buf jb;
        mr_panic_jmp = &jb;
        volatile int panicked = 0;
        for (int i = 0; i < N_FIXTURES; i++)
            if (FIXTURES[i].status == ST_ZL_LEN) {
                fx = &FIXTURES[i];
                robj *o = NULL;
                if (setjmp(jb) == 0) rr_compat_des_batch((void *const *)&fx->blob, &fx->len, 1, &o);
                else panicked++;
            }
        mr_panic_jmp = NULL;
        fx = NULL;
        CHECK(panicked == n_len, "gpu route: %d of %d wrong byte counts panicked", (int)panicked, n_len);
        rr_compat_set_route(RR_COMPAT_ROUTE_HOST);
    }
    drop();
    if (strcmp(mode, "env-off")) {   /* back on: strict again on the same process */
        rr_compat_set_ziplist_check(1);
        got = per_key("back on", 1, &lp);
        CHECK(got == 0 && lp == n_len, "back on: %d corrupt ziplists accepted", got);
        drop();
    }
    printf("ziplist check off: reference acceptance, %d corrupt ziplists accepted, %d wrong byte counts rejected; %d failures\n",
           n_corrupt, n_len, fails);
    return fails ? 1 : 0;
}
