/*
 * rr_d2string.h — d2string (util.c:517-552), exact, on the host and on the GPU.
 *
 * The reference stores a ZSet score in a ziplist as the text d2string prints.  Its last branch is
 * snprintf("%.17g"); the GPU has no printf, so that branch is done here in multi-word integer
 * arithmetic (csrc/rr_d2string_impl.h, one text compiled for both sides).  The result is byte for
 * byte the reference's under glibc, for every double:
 *   NaN (either sign)   "nan"                                                        (:518-519)
 *   +-infinity          "inf", "-inf"                                                (:520-524)
 *   +-0                 "0", "-0"                                                    (:525-530)
 *   an integer-valued v with -(2^52 - 1) < v < 2^52: ll2string's decimal text        (:542-545)
 *   everything else     %.17g                                                        (:548)
 * %.17g: the 17 significant decimal digits of the exact binary value, rounded to nearest on that
 * value, ties to even.  With X the decimal exponent after rounding: -4 <= X < 17 gives fixed
 * notation with 16 - X fractional digits, everything else d.dddde+-XX with an exponent of at least
 * two digits; in both the fraction's trailing zeros go, and the point with them when nothing is left
 * behind it.  "-" for negatives, never "+".  The longest text is "-4.9406564584124654e-324".
 */
#ifndef RR_D2STRING_H
#define RR_D2STRING_H

#include "rr_serdes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RR_D2STRING_MAX  24     /* the longest text, bytes */
#define RR_D2STRING_SLOT 32     /* the batch calls' bytes per text */

/* Host.  Writes at most RR_D2STRING_MAX bytes, no NUL; returns the length. */
int rr_d2string(char *buf, double v);

/* Device-resident: every pointer on ctx's device.  text[32 * i .. 32 * i + len[i]) = d2string of the
 * double whose bits are bits[i]; the rest of the slot is not written.  One launch on `stream`, a
 * lane a score, no scratch, no host synchronisation.  n == 0 launches nothing. */
int rr_d2string_batch(rr_ctx *ctx, const uint64_t *bits, uint64_t n, uint8_t *text, uint8_t *len, void *stream);

/* The same over host pointers, staged through the context's device buffers; blocks.  text is read
 * first (32 * n bytes), so the bytes the call does not write come back as they were. */
int rr_d2string_batch_host(rr_ctx *ctx, const uint64_t *bits, uint64_t n, uint8_t *text, uint8_t *len);

#ifdef __cplusplus
}
#endif
#endif
