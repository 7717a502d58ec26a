/*
 * aof_host_check.c — a stand-alone check of the score-text parser and printer (csrc/rr_strtod_impl.h
 * and csrc/rr_d2string_impl.h) over a fixed list, with its own main: it links nothing of the engine, so
 * it can be built with a sanitizer and run on its own,
 *     gcc -std=c99 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *         -I redrock_old_amd/csrc tools/aof_host_check.c -o aof_host_check && ./aof_host_check
 * Every accepted text must print what %.17g of strtod prints (the C library's own, computed here), and
 * every refused one must be refused.  Exit status 0: all of them held.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rr_strtod_impl.h"

static const char *const taken[] = {
    "0", "-0", "0.0", "1", "-1", "17", "1.5", "1.50", ".5", "5.", "1E5", "1e5", "1e+5", "1e-5", "0.1", "-0.1",
    "inf", "-inf", "1e309", "-1e309", "1e-400", "-1e-400", "1e310", "9e-326", "1e-324", "3e-324",
    "9007199254740993", "9007199254740992", "9007199254740991", "92233720368547758", "4503599627370496",
    "4.9406564584124654e-324", "4.9406564584124653e-324", "4.9406564584124655e-324",
    "2.4703282292062328e-324", "2.4703282292062327e-324", "2.4703282292062329e-324",
    "2.2250738585072014e-308", "2.2250738585072011e-308", "2.2250738585072009e-308",
    "1.7976931348623157e+308", "1.7976931348623158e+308", "1.7976931348623159e+308", "1.797693134862316e308",
    "9.9999999999999992e+22", "1e23", "1.0000000000000001e-05", "0.10000000000000001", "10000000000000000",
    "1e+17", "123456789012345.67", "0.000001", "00012.5000", "100000000000000000000", "1e00000000000000000000000000000005",
    "0.00000000000000000000000000000000000001", "12345678901234567e-340", "99999999999999999e292", "99999999999999999e293",
    "5e-324", "7.4e-324", "7.5e-324", "1e99999", "1e-99999", "0e99999"};

static const char *const refused[] = {
    "", "-", ".", "-.", "e5", "1e", "1e+", "nan", "-nan", "NaN", "0x10", "+1", " 1", "1 ", "1.2.3", "1e5.0", "infinity", "INF",
    "Inf", "--1", "1-", "123456789012345678", "9223372036854775807", "1.2345678901234567891", "11111111111111111111111111111111111111111", "1,5"};

int main(void) {
    uint32_t w[RR_D2S_WORDS];
    char got[64], want[64];
    int bad = 0;
    size_t i;
    for (i = 0; i < sizeof taken / sizeof *taken; i++) {
        const char *t = taken[i];
        uint64_t bits = 0;
        /* a heap copy of exactly the text's bytes: a read past them is the sanitizer's to report */
        const size_t n = strlen(t);
        uint8_t *copy = (uint8_t *)malloc(n ? n : 1);
        int gl, wl;
        memcpy(copy, t, n);
        if (!rr_s2d_parse(copy, (uint32_t)n, &bits, w)) {
            printf("refused: \"%s\"\n", t);
            bad++;
            free(copy);
            continue;
        }
        free(copy);
        gl = rr_d2s_print(got, bits, w);
        wl = snprintf(want, sizeof want, "%.17g", strtod(t, NULL));
        if (gl != wl || memcmp(got, want, (size_t)gl) != 0) {
            printf("\"%s\": got %.*s, want %s\n", t, gl, got, want);
            bad++;
        }
    }
    for (i = 0; i < sizeof refused / sizeof *refused; i++) {
        const char *t = refused[i];
        uint64_t bits = 0;
        const size_t n = strlen(t);
        uint8_t *copy = (uint8_t *)malloc(n ? n : 1);
        memcpy(copy, t, n);
        if (rr_s2d_parse(copy, (uint32_t)n, &bits, w)) {
            printf("taken: \"%s\"\n", t);
            bad++;
        }
        free(copy);
    }
    printf("aof_host_check: %zu taken, %zu refused, %d wrong\n", sizeof taken / sizeof *taken, sizeof refused / sizeof *refused, bad);
    return bad != 0;
}
