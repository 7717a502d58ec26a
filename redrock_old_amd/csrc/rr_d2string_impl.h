/*
 * rr_d2string_impl.h — d2string (util.c:517-552) with its snprintf("%.17g") branch done in exact
 * integer arithmetic: one text for the host (rr_d2string.c, C99) and the device (rr_rdbzset.hip).
 * Plain C, no library call, no floating point.  The including file may define, before the include,
 *   RR_D2S_FN      the functions' qualifier                        (static inline)
 *   RR_D2S_WORD    the type of a word of the multi-word state      (uint32_t)
 *   RR_D2S_STRIDE  word k of the caller's number is w[k * STRIDE]  (1)
 *   RR_D2S_CHAR    the type of a byte of the text                  (char)
 * The device gives every lane its own number in LDS, w = base + lane and a stride of the wave's 64
 * lanes: lane l's word k lies in bank l mod 32 whatever k is, so lanes at different k never collide.
 *
 * %.17g of m * 2^e, 0 < m < 2^53 (include/rr_d2string.h has the rule):
 *   e >= 0  the integer m << e, at most 1024 bits, in 32 words.  Short division by 10^9 peels limbs
 *           off, the lowest first; the last three are the leading 19..27 digits, everything peeled
 *           off before them is one sticky bit.
 *   e <  0  the integer part m >> -e is below 2^53 (two limbs); the fraction (m mod 2^-e) / 2^-e is
 *           a fixed-point number of ceil(-e / 32) <= 34 words.  Short multiplication by 10^9 peels
 *           limbs off the top, the highest first, until 18 digits are there; what is left of the
 *           fraction then is the sticky bit.  Only the words between the lowest and the highest
 *           non-zero one are touched: a subnormal's three words walk up through the 34.
 * 18 digits and the sticky bit decide round-to-nearest-even on the exact value.
 */
#ifndef RR_D2STRING_IMPL_H
#define RR_D2STRING_IMPL_H

#include <stdint.h>

#ifndef RR_D2S_FN
#define RR_D2S_FN static inline
#endif
#ifndef RR_D2S_WORD
#define RR_D2S_WORD uint32_t
#endif
#ifndef RR_D2S_STRIDE
#define RR_D2S_STRIDE 1
#endif
#ifndef RR_D2S_CHAR
#define RR_D2S_CHAR char
#endif

#define RR_D2S_WORDS 34   /* ceil(1074 / 32): the longest fraction, a subnormal's */
#define RR_D2S_W(k) w[(k) * RR_D2S_STRIDE]
#define RR_D2S_E9 1000000000u

/* decimal digits of 0 < v < 10^9 */
RR_D2S_FN uint32_t rr_d2s_ndig9(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u);
}

/* The leading digits, collected from base-10^9 limbs fed from the most significant down: acc holds
 * the first nd <= 18 significant digits, sticky whether anything non-zero lay below them.  The first
 * limb fed is not zero. */
RR_D2S_FN void rr_d2s_feed(uint64_t *acc, uint32_t *nd, uint32_t *sticky, uint32_t limb) {
    uint32_t t, k;
    if (*nd == 0) {
        *acc = limb;
        *nd = rr_d2s_ndig9(limb);
        return;
    }
    t = 18 - *nd;
    if (t > 9) t = 9;
    for (k = t; k < 9; ++k) {   /* the 9 - t low digits do not fit */
        *sticky |= (uint32_t)(limb % 10u != 0);
        limb /= 10u;
    }
    for (k = 0; k < t; ++k) *acc *= 10u;
    *acc += limb;
    *nd += t;
}

/* ll2string (util.c:312-350) of -2^63 < v < 2^63 given as sign and magnitude; returns the length */
RR_D2S_FN int rr_d2s_ll(RR_D2S_CHAR *buf, uint32_t neg, uint64_t a) {
    uint32_t len = neg, p;
    uint64_t t = a;
    do {
        ++len;
        t /= 10u;
    } while (t);
    p = len;
    do {
        buf[--p] = (RR_D2S_CHAR)('0' + (uint32_t)(a % 10u));
        a /= 10u;
    } while (a);
    if (neg) buf[0] = '-';
    return (int)len;
}

/* d2string of the double with these bits into buf (at most RR_D2STRING_MAX = 24 bytes, no NUL);
 * w: RR_D2S_WORDS words of state, values on entry and exit of no meaning.  Returns the length. */
RR_D2S_FN int rr_d2s_print(RR_D2S_CHAR *buf, uint64_t bits, RR_D2S_WORD *w) {
    const uint32_t neg = (uint32_t)(bits >> 63);
    const uint64_t mag = bits & 0x7FFFFFFFFFFFFFFFull;
    const uint32_t bexp = (uint32_t)(mag >> 52);
    const uint64_t m = bexp ? (mag & 0xFFFFFFFFFFFFFull) | (1ull << 52) : mag;
    const int32_t e = (int32_t)(bexp ? bexp : 1u) - 1075;   /* the value is m * 2^e */
    uint64_t acc = 0, q;
    uint32_t nd = 0, sticky = 0, k, n, hi8, lo9, tz, p = 0, len, last, stop, base, after;
    int32_t X;   /* the decimal exponent of the first significant digit */

    if (bexp == 0x7FF) {                                   /* util.c:518-524 */
        if (mag & 0xFFFFFFFFFFFFFull) {
            buf[0] = 'n'; buf[1] = 'a'; buf[2] = 'n';
            return 3;
        }
        if (neg) buf[p++] = '-';
        buf[p] = 'i'; buf[p + 1] = 'n'; buf[p + 2] = 'f';
        return (int)p + 3;
    }
    if (mag == 0) {                                        /* :525-530 */
        if (neg) buf[p++] = '-';
        buf[p] = '0';
        return (int)p + 1;
    }
    /* :542-545: min < value < max and value == (double)(long long)value.  e >= 0 means |value| >=
     * 2^52; e <= -53 means 0 < |value| < 1 */
    if (e < 0 && e > -53 && (m & ((1ull << -e) - 1)) == 0) {
        const uint64_t iv = m >> -e;
        if (neg ? iv < 4503599627370495ull : iv < 4503599627370496ull) return rr_d2s_ll(buf, neg, iv);
    }

    if (e >= 0) {
        const uint32_t sh = (uint32_t)e & 31u, k0 = (uint32_t)e >> 5;
        const uint64_t lo64 = m << sh;
        uint32_t top, l0 = 0, l1 = 0, l2 = 0, dropped = 0, L = 0;
        n = ((uint32_t)e + 53u + 31u) >> 5;                /* <= 32 */
        for (k = 0; k < n; ++k) RR_D2S_W(k) = 0;
        RR_D2S_W(k0) = (uint32_t)lo64;
        RR_D2S_W(k0 + 1) = (uint32_t)(lo64 >> 32);
        if (k0 + 2 < n) RR_D2S_W(k0 + 2) = sh ? (uint32_t)(m >> (64 - sh)) : 0u;
        top = n;                                           /* the number is words [0, top) */
        while (top > 0 && RR_D2S_W(top - 1) == 0) --top;
        while (top > 0) {
            uint64_t rem = 0;
            for (k = top; k-- > 0;) {
                const uint64_t t = (rem << 32) | RR_D2S_W(k);
                const uint32_t d = (uint32_t)(t / RR_D2S_E9);   /* rem < 10^9: the quotient fits */
                rem = t - (uint64_t)d * RR_D2S_E9;
                RR_D2S_W(k) = d;
            }
            while (top > 0 && RR_D2S_W(top - 1) == 0) --top;
            dropped |= (uint32_t)(l2 != 0);
            l2 = l1;
            l1 = l0;
            l0 = (uint32_t)rem;
            ++L;
        }
        X = (int32_t)(rr_d2s_ndig9(l0) + 9u * (L - 1u)) - 1;   /* the last limb is the leading one, not zero */
        rr_d2s_feed(&acc, &nd, &sticky, l0);
        if (L >= 2) rr_d2s_feed(&acc, &nd, &sticky, l1);
        if (L >= 3) rr_d2s_feed(&acc, &nd, &sticky, l2);
        sticky |= dropped;
    } else {
        const uint32_t s = (uint32_t)-e;                   /* 1 .. 1074 */
        const uint64_t ip = s < 64 ? m >> s : 0;
        const uint64_t fm = s < 64 ? m & ((1ull << s) - 1) : m;
        uint32_t sh, lo = 0, top, z = 0;
        uint64_t lo64;
        n = (s + 31u) >> 5;                                /* 1 .. 34 */
        sh = 32u * n - s;
        lo64 = fm << sh;                                   /* fm < 2^min(s, 53): at most 84 bits with sh */
        for (k = 0; k < n; ++k) RR_D2S_W(k) = 0;
        RR_D2S_W(0) = (uint32_t)lo64;
        if (n > 1) RR_D2S_W(1) = (uint32_t)(lo64 >> 32);
        if (n > 2) RR_D2S_W(2) = sh ? (uint32_t)(fm >> (64 - sh)) : 0u;
        top = n < 3 ? n : 3;                               /* the fraction's non-zero words are [lo, top) */
        while (top > 0 && RR_D2S_W(top - 1) == 0) --top;
        while (lo < top && RR_D2S_W(lo) == 0) ++lo;
        X = 0;
        if (ip) {
            const uint32_t h = (uint32_t)(ip / RR_D2S_E9), l = (uint32_t)(ip % RR_D2S_E9);
            if (h) {
                X = (int32_t)rr_d2s_ndig9(h) + 8;
                rr_d2s_feed(&acc, &nd, &sticky, h);
            } else {
                X = (int32_t)rr_d2s_ndig9(l) - 1;
            }
            rr_d2s_feed(&acc, &nd, &sticky, l);
        }
        while (nd < 18 && lo < top) {
            uint64_t carry = 0;
            uint32_t limb = 0;
            for (k = lo; k < top; ++k) {
                const uint64_t t = (uint64_t)RR_D2S_W(k) * RR_D2S_E9 + carry;
                RR_D2S_W(k) = (uint32_t)t;
                carry = t >> 32;
            }
            if (top < n) {                                 /* below 2^-32: this limb is zero */
                RR_D2S_W(top) = (uint32_t)carry;
                if (carry) ++top;
            } else {
                limb = (uint32_t)carry;
            }
            while (lo < top && RR_D2S_W(lo) == 0) ++lo;
            if (nd == 0) {
                if (limb == 0) {
                    ++z;
                    continue;
                }
                X = -(int32_t)(9u * z + 10u - rr_d2s_ndig9(limb));
            }
            rr_d2s_feed(&acc, &nd, &sticky, limb);
        }
        sticky |= (uint32_t)(lo < top);
    }
    for (; nd < 18; ++nd) acc *= 10u;                      /* a short number: exact zeros */

    q = acc / 10u;                                         /* 17 digits, to nearest, ties to even */
    k = (uint32_t)(acc % 10u);
    if (k > 5 || (k == 5 && (sticky || (q & 1)))) {
        if (++q == 100000000000000000ull) {
            q = 10000000000000000ull;
            ++X;
        }
    }
    hi8 = (uint32_t)(q / RR_D2S_E9);                       /* digits 0..7 | 8..16 */
    lo9 = (uint32_t)(q % RR_D2S_E9);
    tz = 0;                                                /* %g drops the fraction's trailing zeros */
    k = lo9;
    if (k == 0) {
        tz = 9;
        k = hi8;
    }
    while (k % 10u == 0) {
        k /= 10u;
        ++tz;
    }
    last = 16 - tz;                                        /* the last non-zero digit */

    /* digit i goes to base + i, one further behind the point, which follows digit `after`; digits
     * above `stop` are not printed */
    if (neg) buf[p++] = '-';
    if (X >= -4 && X < 17) {
        if (X >= 0) {
            base = p;
            after = (uint32_t)X;
            stop = last > after ? last : after;
            len = base + stop + 1;
            if (last > after) {
                buf[base + after + 1] = '.';
                ++len;
            }
        } else {
            buf[p] = '0';
            buf[p + 1] = '.';
            for (k = 0; k < (uint32_t)(-X - 1); ++k) buf[p + 2 + k] = '0';
            base = p + 2 + (uint32_t)(-X - 1);
            after = 17;
            stop = last;
            len = base + stop + 1;
        }
    } else {
        uint32_t ax = (uint32_t)(X < 0 ? -X : X), x;
        base = p;
        after = 0;
        stop = last;
        x = base + stop + 1;
        if (last > 0) {
            buf[base + 1] = '.';
            ++x;
        }
        buf[x] = 'e';
        buf[x + 1] = X < 0 ? '-' : '+';
        x += 2;
        if (ax >= 100) {
            buf[x++] = (RR_D2S_CHAR)('0' + ax / 100u);
            ax %= 100u;
        }
        buf[x] = (RR_D2S_CHAR)('0' + ax / 10u);
        buf[x + 1] = (RR_D2S_CHAR)('0' + ax % 10u);
        len = x + 2;
    }
    for (k = 17; k-- > 0;) {
        uint32_t d;
        if (k >= 8) {
            d = lo9 % 10u;
            lo9 /= 10u;
        } else {
            d = hi8 % 10u;
            hi8 /= 10u;
        }
        if (k <= stop) buf[base + k + (k > after ? 1u : 0u)] = (RR_D2S_CHAR)('0' + d);
    }
    return (int)len;
}

#endif
