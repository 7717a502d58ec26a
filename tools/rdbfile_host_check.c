/* Stand-alone check of the host helpers of include/rr_rdbfile.h (no GPU, no HIP): the CRC-64 known
 * answers, the combine identities, the head and SELECTDB writers and their capacity rule.  Built
 * with redrock_old_amd/csrc/rr_rdbfile_api.c under -DRR_RDBFILE_HOST_ONLY, for a sanitizer run:
 *   gcc -O1 -g -pthread -fsanitize=address,undefined -DRR_RDBFILE_HOST_ONLY -Iinclude \
 *       tools/rdbfile_host_check.c redrock_old_amd/csrc/rr_rdbfile_api.c -o rdbfile_host_check
 * Exit status 0 and "rdbfile host check ok" when everything holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rr_rdbfile.h"

static int failures;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static uint64_t bytewise(uint64_t crc, const uint8_t *p, size_t n) {   /* the definition, bit by bit */
    for (size_t i = 0; i < n; i++) {
        crc ^= p[i];
        for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ ((crc & 1) ? 0x95ac9329ac4bc9b5ull : 0);
    }
    return crc;
}

int main(void) {
    CHECK(rr_crc64(0, "123456789", 9) == 0xe9c6d914c4b8d9caull);
    const uint8_t one = 1, two = 2;
    CHECK(rr_crc64(0, &one, 1) == 0x7ad870c830358979ull);   /* table entries 1 and 2 */
    CHECK(rr_crc64(0, &two, 1) == 0xf5b0e190606b12f2ull);
    const uint8_t dump_a[5] = {0x00, 0x01, 0x61, 0x09, 0x00};
    CHECK(rr_crc64(0, dump_a, 5) == 0x051eb0db57be0c6full);  /* 6f 0c be 57 db b0 1e 05 little-endian */

    static const size_t lens[] = {0, 1, 7, 8, 9, 63, 64, 65, 4097};
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    for (size_t li = 0; li < sizeof lens / sizeof *lens; li++)
        for (size_t mis = 0; mis < 16; mis++) {
            const size_t n = lens[li];
            uint8_t *raw = (uint8_t *)malloc(n + 16 + 1);    /* exactly: a read past the end is an ASan report */
            uint8_t *p = raw + mis;
            for (size_t i = 0; i < n; i++) {
                seed = seed * 6364136223846793005ull + 1442695040888963407ull;
                p[i] = (uint8_t)(seed >> 56);
            }
            uint8_t *exact = (uint8_t *)malloc(n ? n : 1);
            memcpy(exact, p, n);
            CHECK(rr_crc64(0, exact, n) == bytewise(0, p, n));
            CHECK(rr_crc64(0x0123456789ABCDEFull, p, n) == bytewise(0x0123456789ABCDEFull, p, n));
            /* crc(0, A || B) = shift(crc(0, A), |B|) ^ crc(0, B);  crc(c, B) = crc(0, B) ^ shift(c, |B|) */
            const size_t a = n / 3;
            CHECK(rr_crc64(0, p, n) == (rr_crc64_shift(rr_crc64(0, p, a), n - a) ^ rr_crc64(0, p + a, n - a)));
            CHECK(rr_crc64(0xFEEDull, p, n) == (rr_crc64(0, p, n) ^ rr_crc64_shift(0xFEEDull, n)));
            free(exact);
            free(raw);
        }
    CHECK(rr_crc64_mul(0x1234, 1ull << 63) == 0x1234);      /* times x^0 */

    uint8_t buf[512];
    const rr_rdbfile_repl repl = {3, "0123456789abcdef0123456789abcdef01234567", 123456789012ll};
    const uint64_t need = rr_rdbfile_head(NULL, 0, "6.0.20", 1700000000, 5000000000ull, &repl, 0);
    CHECK(need > 9 && need < sizeof buf);
    uint8_t *tight = (uint8_t *)malloc(need);
    CHECK(rr_rdbfile_head(tight, need, "6.0.20", 1700000000, 5000000000ull, &repl, 0) == need);
    CHECK(memcmp(tight, "REDIS0009\xFA\x09redis-ver\x06" "6.0.20\xFA\x0Aredis-bits\xC0\x40", 9 + 11 + 7 + 12 + 2) == 0);
    memset(buf, 0xA5, sizeof buf);
    CHECK(rr_rdbfile_head(buf, need - 1, "6.0.20", 1700000000, 5000000000ull, &repl, 0) == need);
    for (size_t i = 0; i < sizeof buf; i++) CHECK(buf[i] == 0xA5);
    free(tight);
    uint8_t sel[6];
    CHECK(rr_rdbfile_selectdb(sel, sizeof sel, 64, 10, 2) == 6 && memcmp(sel, "\xFE\x40\x40\xFB\x0A\x02", 6) == 0);
    memset(sel, 0xA5, sizeof sel);
    CHECK(rr_rdbfile_selectdb(sel, 5, 64, 10, 2) == 6 && sel[0] == 0xA5);
    CHECK(rr_rdbfile_selectdb(NULL, 0, 16384, 1ull << 40, 0) == 1 + 5 + 1 + 5 + 1);
    CHECK(rr_rdbfile_bound(3, 10, 100, 7) == ((7 + 81 + 10 + 100 + 9 + 15) & ~15ull));
    if (failures) return 1;
    printf("rdbfile host check ok\n");
    return 0;
}
