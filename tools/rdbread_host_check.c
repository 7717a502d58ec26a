/* Stand-alone check of the host half of include/rr_rdbread.h (no GPU, no HIP): rr_rdbread_index,
 * rr_rdbread_string and rr_rdbread_len over a small hand-built stream: whole; cut at every byte, in a
 * buffer allocated to exactly the cut length, and resumed from where the index stopped; and with
 * every single byte set to 0xFF and to 0x81 in turn.  Built with redrock_old_amd/csrc/rr_rdbread_api.c
 * under -DRR_RDBREAD_HOST_ONLY, for a sanitizer run:
 *   gcc -O1 -g -fsanitize=address,undefined -DRR_RDBREAD_HOST_ONLY -Iinclude \
 *       tools/rdbread_host_check.c redrock_old_amd/csrc/rr_rdbread_api.c -o rdbread_host_check
 * Exit status 0 and "rdbread host check ok" when everything holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rr_rdbread.h"

static int failures;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

#define MAXR 16
static uint8_t S[512];
static uint64_t slen, want_start[MAXR], want_end[MAXR], want_db[MAXR], want_item[MAXR][2], n_want, n_want_items, want_eof;

static void put(const void *p, size_t n) { memcpy(S + slen, p, n); slen += n; }
#define LIT(s) put(s, sizeof(s) - 1)
static void fill(size_t n) { for (size_t i = 0; i < n; i++) S[slen++] = (uint8_t)(i * 7 + 1); }
static void rec_begin(uint64_t db) { want_start[n_want] = slen; want_db[n_want] = db; }
static void rec_end(void) { want_end[n_want++] = slen; }
static void item_begin(void) { want_item[n_want_items][0] = slen; }
static void item_end(void) { want_item[n_want_items++][1] = slen; }

static void build(void) {
    LIT("REDIS0009");
    item_begin(); LIT("\xFA\x09redis-ver\x06" "6.0.20"); item_end();
    item_begin(); LIT("\xFA\x0Aredis-bits\xC0\x40"); item_end();
    item_begin(); LIT("\xFE\x00"); item_end();
    item_begin(); LIT("\xFB\x05\x01"); item_end();
    rec_begin(0); LIT("\xFC\x01\x02\x03\x04\x05\x06\x07\x08\x00\x02k1\x05hello"); rec_end();               /* String, expire */
    rec_begin(0); LIT("\xF8\x40\x40\xF9\x07\x04\xC1\x39\x30\x01\xC3\x04\x06\x00" "a\x60\x00\xC0\x7F"); rec_end();   /* Hash: LZF field, int value; int16 key */
    rec_begin(0); LIT("\xFD\x10\x00\x00\x00\x03\x01z\x02\x01" "a\xFD\x01" "b\x03" "1.5"); rec_end();          /* legacy ZSet: NaN and a text score */
    rec_begin(0); LIT("\x0E\x03ql1\x01\x0B\x0B\x00\x00\x00\x0A\x00\x00\x00\x00\x00\xFF"); rec_end();          /* Quicklist, one node */
    rec_begin(0); LIT("\x05\xC3\x04\x03\x02key\x01\x01m\x00\x00\x00\x00\x00\x00\xF0\x3F"); rec_end();         /* ZSet 2, LZF key */
    item_begin(); LIT("\xFE\x01"); item_end();
    rec_begin(1); LIT("\x02\x01s\x02\x80\x00\x00\x00\x03" "abc\x41\x00"); fill(256); rec_end();              /* Set: 5-byte and 2-byte lengths */
    rec_begin(1); LIT("\x01\x01l\x00"); rec_end();                                                             /* legacy List, empty */
    want_eof = slen;
    LIT("\xFF\x11\x22\x33\x44\x55\x66\x77\x88");
}

typedef struct idx {
    uint64_t rs[MAXR], re[MAXR], rd[MAXR];
    rr_rdbread_item items[MAXR];
    rr_rdbread_index_result res;
    rr_rdbread_state st;
} idx;

/* what any outcome must respect: the extents lie in order inside the bytes given */
static void sane(const idx *x, int rc, uint64_t bytes) {
    CHECK(rc >= 0 && x->st.pos <= bytes && x->res.n_recs <= MAXR && x->res.n_items <= MAXR);
    uint64_t prev = 0;
    for (uint64_t i = 0; i < x->res.n_recs; i++) {
        CHECK(x->rs[i] >= prev && x->rs[i] < x->re[i] && x->re[i] <= bytes);
        prev = x->re[i];
    }
    for (uint64_t i = 0; i < x->res.n_items; i++) CHECK(x->items[i].at < x->items[i].end && x->items[i].end <= bytes);
    if (rc == RR_RDBREAD_DONE) CHECK(x->res.eof_at < bytes && x->st.pos <= bytes);
}

int main(void) {
    build();
    idx *w = (idx *)calloc(1, sizeof *w);
    int rc = rr_rdbread_index(&w->st, S, slen, w->rs, w->re, w->rd, MAXR, w->items, MAXR, &w->res);
    CHECK(rc == RR_RDBREAD_DONE && w->res.n_recs == n_want && w->res.n_items == n_want_items && w->st.version == 9);
    CHECK(w->res.eof_at == want_eof && w->res.has_cksum == 1 && w->res.cksum == 0x8877665544332211ull && w->st.pos == slen);
    for (uint64_t i = 0; i < n_want; i++) CHECK(w->rs[i] == want_start[i] && w->re[i] == want_end[i] && w->rd[i] == want_db[i]);
    for (uint64_t i = 0; i < n_want_items; i++) CHECK(w->items[i].at == want_item[i][0] && w->items[i].end == want_item[i][1]);
    sane(w, rc, slen);

    /* the strings of the head and a few keys */
    uint8_t out[16];
    uint64_t len, end;
    CHECK(rr_rdbread_string(S, slen, want_item[0][0] + 1, out, sizeof out, &len, &end) == RR_RDBREAD_DONE && len == 9 && !memcmp(out, "redis-ver", 9));
    CHECK(rr_rdbread_string(S, slen, end, out, sizeof out, &len, &end) == RR_RDBREAD_DONE && len == 6 && !memcmp(out, "6.0.20", 6) && end == want_item[0][1]);
    CHECK(rr_rdbread_string(S, slen, want_item[1][1] - 2, out, sizeof out, &len, &end) == RR_RDBREAD_DONE && len == 2 && !memcmp(out, "64", 2));
    CHECK(rr_rdbread_string(S, slen, want_start[1] + 6, out, sizeof out, &len, &end) == RR_RDBREAD_DONE && len == 5 && !memcmp(out, "12345", 5));
    CHECK(rr_rdbread_string(S, slen, want_start[1] + 10, out, sizeof out, &len, &end) == RR_RDBREAD_DONE && len == 6 && !memcmp(out, "aaaaaa", 6));
    CHECK(rr_rdbread_string(S, slen, want_start[1] + 10, out, 5, &len, &end) == RR_E_CAPACITY && len == 6);
    CHECK(rr_rdbread_string(S, slen, want_start[4] + 1, out, sizeof out, &len, &end) == RR_RDBREAD_DONE && len == 3 && !memcmp(out, "key", 3));
    uint64_t val;
    CHECK(rr_rdbread_len(S, slen, want_item[3][0] + 1, &val, &end) == RR_RDBREAD_DONE && val == 5 && end == want_item[3][0] + 2);

    /* cut at every byte: the buffer holds exactly the cut, so a read past it is a sanitizer report */
    for (uint64_t cut = 0; cut < slen; cut++) {
        uint8_t *b = (uint8_t *)malloc(cut ? cut : 1);
        memcpy(b, S, cut);
        idx *x = (idx *)calloc(1, sizeof *x);
        rc = rr_rdbread_index(&x->st, b, cut, x->rs, x->re, x->rd, MAXR, x->items, MAXR, &x->res);
        CHECK(rc == RR_RDBREAD_MORE);
        sane(x, rc, cut);
        for (uint64_t i = 0; i < x->res.n_recs; i++) CHECK(x->rs[i] == want_start[i] && x->re[i] == want_end[i]);
        /* resumed over the whole stream from where it stopped: the rest of the records */
        const uint64_t got = x->res.n_recs, got_items = x->res.n_items;
        rc = rr_rdbread_index(&x->st, S, slen, x->rs, x->re, x->rd, MAXR, x->items, MAXR, &x->res);
        CHECK(rc == RR_RDBREAD_DONE && got + x->res.n_recs == n_want && got_items + x->res.n_items == n_want_items);
        for (uint64_t i = 0; i < x->res.n_recs; i++) CHECK(x->rs[i] == want_start[got + i] && x->re[i] == want_end[got + i] && x->rd[i] == want_db[got + i]);
        for (uint64_t at = 0; at <= cut; at++) {
            const int r2 = rr_rdbread_string(b, cut, at, out, 8, &len, &end);
            CHECK(r2 >= 0 && (r2 != RR_RDBREAD_DONE || (end <= cut && len <= 8)));
        }
        free(x);
        free(b);
    }

    /* every single byte 0xFF, then 0x81: any outcome, inside the buffer */
    static const uint8_t subst[2] = {0xFF, 0x81};
    for (int k = 0; k < 2; k++)
        for (uint64_t i = 0; i < slen; i++) {
            uint8_t *b = (uint8_t *)malloc(slen);
            memcpy(b, S, slen);
            b[i] = subst[k];
            idx *x = (idx *)calloc(1, sizeof *x);
            rc = rr_rdbread_index(&x->st, b, slen, x->rs, x->re, x->rd, MAXR, x->items, MAXR, &x->res);
            sane(x, rc, slen);
            if (rc == RR_RDBREAD_E_UNSUPPORTED || rc == RR_RDBREAD_E_LEN) CHECK(x->res.err_at == x->st.pos);
            uint8_t *o8 = (uint8_t *)malloc(8);
            for (uint64_t at = 0; at <= slen; at++) {
                const int r2 = rr_rdbread_string(b, slen, at, o8, 8, &len, &end);
                CHECK(r2 >= 0 && (r2 != RR_RDBREAD_DONE || (end <= slen && len <= 8)));
                CHECK(rr_rdbread_len(b, slen, at, &val, &end) >= 0);
            }
            free(o8);
            free(x);
            free(b);
        }

    /* capacities: one record or item a call */
    {
        idx *x = (idx *)calloc(1, sizeof *x);
        uint64_t nr = 0, ni = 0;
        for (int guard = 0; guard < 64; guard++) {
            rc = rr_rdbread_index(&x->st, S, slen, x->rs, x->re, x->rd, 1, x->items, 1, &x->res);
            for (uint64_t i = 0; i < x->res.n_recs; i++, nr++) CHECK(x->rs[i] == want_start[nr] && x->re[i] == want_end[nr]);
            for (uint64_t i = 0; i < x->res.n_items; i++, ni++) CHECK(x->items[i].at == want_item[ni][0]);
            if (rc != RR_RDBREAD_FULL) break;
        }
        CHECK(rc == RR_RDBREAD_DONE && nr == n_want && ni == n_want_items);
        free(x);
    }
    free(w);
    if (failures) return 1;
    printf("rdbread host check ok\n");
    return 0;
}
