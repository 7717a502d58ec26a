/*
 * rr_strtod_impl.h — a correctly rounded decimal-to-double conversion in exact integer arithmetic,
 * the other direction of rr_d2string_impl.h: one text for the host (rr_aof_api.c, C99) and the device
 * (rr_aof.hip).  Plain C, no library call, no floating point.  It is included behind
 * rr_d2string_impl.h and takes that file's RR_D2S_FN / RR_D2S_WORD / RR_D2S_STRIDE: the multi-word
 * state is the printer's RR_D2S_WORDS words, so a lane parses a score text and prints the double in
 * the same LDS.
 *
 * The texts taken (include/rr_aof.h): "inf", "-inf", and
 *     -? ( digits+ [ . digits* ] | . digits+ ) ( [eE] [+-]? digits+ )?
 * of at most RR_S2D_MAX_TEXT bytes with at most 17 significant digits, counted from the first
 * non-zero digit through the last non-zero one.  So the value is M * 10^E with 0 <= M < 10^17 < 2^57.
 *   E >= 0  the integer M * 5^E, by short multiplication with 5^13 a step, is exact; the value is
 *           that integer times 2^E.  A first digit at 10^310 or above is infinity before any of this,
 *           so E <= 309 and the integer has at most 57 + 718 bits: 25 words.
 *   E <  0  with n = -E the value is M / (5^n 2^n).  X = M << S with S = floor(2379 n / 1024) + 65
 *           (2379 / 1024 > log2 5, so X / 5^n >= 2^64), divided by 5^13 a step in short division.
 *           floor(floor(x / a) / b) = floor(x / (a b)), and the whole division is exact only if
 *           every step's remainder is zero: the remainders are one sticky bit.  A first digit below
 *           10^-326 rounds to zero before any of this, so n <= 342, S <= 859 and X has at most
 *           57 + 859 bits: 29 words.  The value is (Q + sticky) * 2^-(S + n).
 * rr_s2d_round then keeps the leading 53 bits of Q (fewer for a subnormal: nothing below 2^-1074)
 * and rounds to nearest, ties to even, on the bit below them and the sticky rest.
 */
#ifndef RR_STRTOD_IMPL_H
#define RR_STRTOD_IMPL_H

#include "rr_d2string_impl.h"

#define RR_S2D_MAX_TEXT 40
#define RR_S2D_MAX_DIGITS 17
#define RR_S2D_P13 1220703125u   /* 5^13 < 2^32 */

/* 64 bits of the number in words [0, top) from bit `pos` up; bits past the top are zero */
RR_D2S_FN uint64_t rr_s2d_bits64(const RR_D2S_WORD *w, uint32_t top, uint32_t pos) {
    const uint32_t wi = pos >> 5, b = pos & 31u;
    const uint64_t lo = wi < top ? RR_D2S_W(wi) : 0u, mid = wi + 1 < top ? RR_D2S_W(wi + 1) : 0u;
    const uint64_t hi = wi + 2 < top ? RR_D2S_W(wi + 2) : 0u;
    const uint64_t v = (lo | (mid << 32)) >> b;
    return b ? v | (hi << (64 - b)) : v;
}

/* The bits of the double nearest to (Q + sticky's fraction) * 2^e2, ties to even; Q the number in
 * words [0, top), its top word not zero, and Q >= 2^55 wherever sticky is set.  Overflow gives
 * infinity, underflow a subnormal or zero. */
RR_D2S_FN uint64_t rr_s2d_round(const RR_D2S_WORD *w, uint32_t top, uint32_t sticky, int32_t e2, uint32_t neg) {
    const uint64_t sign = (uint64_t)neg << 63;
    uint32_t tw = RR_D2S_W(top - 1), L = 32u * (top - 1), k;
    int32_t shift, ee;
    uint64_t mant, bits;
    while (tw) {
        ++L;
        tw >>= 1;
    }
    shift = (int32_t)L - 53;                                /* a normal number keeps 53 bits */
    if (shift < -1074 - e2) shift = -1074 - e2;             /* nothing below 2^-1074 */
    if (shift <= 0) {
        mant = rr_s2d_bits64(w, top, 0) << (uint32_t)-shift;   /* Q < 2^53 and exact */
    } else {
        const uint32_t s = (uint32_t)shift, rb = s - 1;     /* the bit below the kept ones */
        uint32_t round = 0, rest = sticky;
        mant = rr_s2d_bits64(w, top, s);
        if ((rb >> 5) < top) {
            const uint32_t x = RR_D2S_W(rb >> 5);
            round = (x >> (rb & 31u)) & 1u;
            rest |= (uint32_t)((x & ((1u << (rb & 31u)) - 1u)) != 0);
        }
        for (k = 0; k < (rb >> 5) && k < top; ++k) rest |= (uint32_t)(RR_D2S_W(k) != 0);
        if (round && (rest || (mant & 1u))) ++mant;
    }
    /* mant * 2^(shift + e2) with mant <= 2^53; mant < 2^52 only for a subnormal (ee == 0).  The sum
     * carries a mantissa that rounded up to the next power of two into the exponent */
    ee = shift + e2 + 1074;
    if (ee >= 2046) return sign | 0x7FF0000000000000ull;
    bits = ((uint64_t)(uint32_t)ee << 52) + mant;
    if ((bits >> 52) >= 0x7FFu) return sign | 0x7FF0000000000000ull;
    return sign | bits;
}

/* The double nearest to (-1)^neg * a */
RR_D2S_FN uint64_t rr_s2d_from_u64(uint32_t neg, uint64_t a, RR_D2S_WORD *w) {
    if (a == 0) return (uint64_t)neg << 63;
    RR_D2S_W(0) = (uint32_t)a;
    RR_D2S_W(1) = (uint32_t)(a >> 32);
    return rr_s2d_round(w, (a >> 32) ? 2u : 1u, 0, 0, neg);
}

/* The double nearest to (-1)^neg * M * 10^E, 0 <= M < 10^17 with nd digits */
RR_D2S_FN uint64_t rr_s2d_scale(uint32_t neg, uint64_t M, uint32_t nd, int32_t E, RR_D2S_WORD *w) {
    const uint64_t sign = (uint64_t)neg << 63;
    const int32_t first = E + (int32_t)nd - 1;              /* the decimal exponent of M's first digit */
    uint32_t top, k, left, f, j, sticky = 0;
    if (M == 0) return sign;
    if (first >= 310) return sign | 0x7FF0000000000000ull;  /* >= 10^310 > DBL_MAX + half an ulp */
    if (first < -326) return sign;                          /* < 10^-325 < 2^-1075 */
    if (E >= 0) {
        RR_D2S_W(0) = (uint32_t)M;
        RR_D2S_W(1) = (uint32_t)(M >> 32);
        top = (M >> 32) ? 2u : 1u;
        for (left = (uint32_t)E; left;) {
            uint64_t carry = 0;
            const uint32_t c = left < 13u ? left : 13u;
            left -= c;
            for (f = 1, j = 0; j < c; ++j) f *= 5u;
            for (k = 0; k < top; ++k) {
                const uint64_t t = (uint64_t)RR_D2S_W(k) * f + carry;
                RR_D2S_W(k) = (uint32_t)t;
                carry = t >> 32;
            }
            if (carry) RR_D2S_W(top++) = (uint32_t)carry;
        }
        return rr_s2d_round(w, top, 0, E, neg);
    } else {
        const uint32_t n = (uint32_t)-E, S = ((n * 2379u) >> 10) + 65u, k0 = S >> 5, sh = S & 31u;
        const uint64_t lo64 = M << sh;                      /* M < 2^57: at most 88 bits with sh */
        top = k0 + 3;
        for (k = 0; k < top; ++k) RR_D2S_W(k) = 0;
        RR_D2S_W(k0) = (uint32_t)lo64;
        RR_D2S_W(k0 + 1) = (uint32_t)(lo64 >> 32);
        RR_D2S_W(k0 + 2) = sh ? (uint32_t)(M >> (64 - sh)) : 0u;
        while (RR_D2S_W(top - 1) == 0) --top;
        for (left = n; left;) {
            uint64_t rem = 0;
            const uint32_t c = left < 13u ? left : 13u;
            left -= c;
            if (c == 13u) {                                 /* a constant divisor: no division instruction */
                for (k = top; k-- > 0;) {
                    const uint64_t t = (rem << 32) | RR_D2S_W(k);
                    const uint32_t q = (uint32_t)(t / RR_S2D_P13);
                    rem = t - (uint64_t)q * RR_S2D_P13;
                    RR_D2S_W(k) = q;
                }
            } else {
                for (f = 1, j = 0; j < c; ++j) f *= 5u;
                for (k = top; k-- > 0;) {
                    const uint64_t t = (rem << 32) | RR_D2S_W(k);
                    const uint32_t q = (uint32_t)(t / f);   /* rem < f: the quotient fits */
                    rem = t - (uint64_t)q * f;
                    RR_D2S_W(k) = q;
                }
            }
            sticky |= (uint32_t)(rem != 0);
            while (RR_D2S_W(top - 1) == 0) --top;           /* Q >= 2^64 throughout */
        }
        return rr_s2d_round(w, top, sticky, -(int32_t)(S + n), neg);
    }
}

/* The text s[0, len) -> *bits; returns 1, or 0 for a text that is not taken (the head of this file) */
RR_D2S_FN int rr_s2d_parse(const uint8_t *s, uint32_t len, uint64_t *bits, RR_D2S_WORD *w) {
    uint32_t p = 0, neg = 0, nd = 0, pend = 0, pend_frac = 0, ndig = 0, frac = 0, j;
    uint64_t M = 0;
    int32_t E = 0;
    if (len == 0 || len > RR_S2D_MAX_TEXT) return 0;
    if (s[0] == '-') {
        neg = 1;
        p = 1;
    }
    if (len - p == 3 && s[p] == 'i' && s[p + 1] == 'n' && s[p + 2] == 'f') {
        *bits = ((uint64_t)neg << 63) | 0x7FF0000000000000ull;
        return 1;
    }
    for (; p < len; ++p) {
        const uint32_t c = s[p];
        uint32_t d;
        if (c == '.' && !frac) {
            frac = 1;
            continue;
        }
        if (c < '0' || c > '9') break;
        d = c - '0';
        ++ndig;
        if (M == 0 && d == 0) {                             /* a leading zero */
            E -= (int32_t)frac;
        } else if (d == 0) {                                /* significant only if a digit follows */
            ++pend;
            pend_frac += frac;
        } else {
            if (nd + pend + 1 > RR_S2D_MAX_DIGITS) return 0;
            for (j = 0; j <= pend; ++j) M *= 10u;
            M += d;
            nd += pend + 1;
            E -= (int32_t)(pend_frac + frac);
            pend = pend_frac = 0;
        }
    }
    if (ndig == 0) return 0;                                /* "", "-", ".", "e5" */
    E += (int32_t)(pend - pend_frac);                       /* the integer part's trailing zeros */
    if (p < len) {
        uint32_t eneg = 0, x = 0, xd = 0;
        if (s[p] != 'e' && s[p] != 'E') return 0;
        ++p;
        if (p < len && (s[p] == '+' || s[p] == '-')) eneg = s[p++] == '-';
        for (; p < len; ++p) {
            const uint32_t c = s[p];
            if (c < '0' || c > '9') return 0;
            if (x < 100000u) x = x * 10u + (c - '0');       /* anything this large is an overflow or underflow */
            ++xd;
        }
        if (xd == 0) return 0;
        E += eneg ? -(int32_t)x : (int32_t)x;
    }
    *bits = rr_s2d_scale(neg, M, nd, E, w);
    return 1;
}

#endif
