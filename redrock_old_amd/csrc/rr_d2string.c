/*
 * rr_d2string.c — the host twin of the GPU's score printer (include/rr_d2string.h): the statements of
 * rr_d2string_impl.h over a local array.  No HIP, no libc beyond memcpy: the file compiles on its own.
 */
#include <string.h>

#include "rr_d2string_impl.h"

int rr_d2string(char *buf, double v);

int rr_d2string(char *buf, double v) {
    uint32_t w[RR_D2S_WORDS];
    uint64_t bits;
    memcpy(&bits, &v, sizeof bits);
    return rr_d2s_print(buf, bits, w);
}
