// rr_rdbconvert_device.h — what the kernels that build rdbLoadObject's small encodings share
// (rr_rdbconvert.hip, rr_rdbzset.hip): a wave's sort arrays in LDS, the ziplist under construction,
// d2string's classes without %.17g, the order of scores and members, and the two halves of the ZSet
// conversion that do not depend on how a score is printed: reading the members and scores into the
// sort arrays, and the rank sort.  Line references are to the reference's ziplist.c, t_zset.c, util.c
// and sds.c (include/rr_rdbconvert.h restates the rule).  Wave-uniform unless it says per lane.
#pragma once
#include "rr_rdbload_device.h"
#include "../../include/rr_rdbconvert.h"

namespace rr {

constexpr uint32_t MAXN = RR_RDBCONVERT_MAX_N;
constexpr uint32_t PEEK = 64;                          // the wave's window: a string's first bytes only
constexpr uint32_t INTF = 0x80000000u;                 // mlen[]: the member is in the integer form, moff[] its value
// a wave's sort arrays: key[MAXN] u64 | moff[MAXN] u32, mlen[MAXN] u32 (a Set: sorted[MAXN] i64) | ord[MAXN] u16;
// the window follows them
constexpr uint32_t SORT_LDS = 8 * MAXN + 8 * MAXN + 2 * MAXN;
static_assert(SORT_LDS % 8 == 0 && MAXN <= 65535 && PEEK >= RR_WAVE, "static LDS");

struct Lds {
    lds_u64 *key;      // a Set's values; a ZSet's score bits
    lds_u64 *sorted;   // a Set's values in order (over moff / mlen)
    lds_u32 *moff, *mlen;
    lds_u16 *ord;      // a ZSet's permutation: ord[rank] = index
    lds_u8 *win;
};
__device__ __forceinline__ Lds sort_lds(lds_u8 *b) {   // b: SORT_LDS + PEEK bytes, 8-aligned
    return {(lds_u64 *)b, (lds_u64 *)(b + 8 * MAXN), (lds_u32 *)(b + 8 * MAXN), (lds_u32 *)(b + 12 * MAXN),
            (lds_u16 *)(b + 16 * MAXN), b + 18 * MAXN};
}

// what other lanes of the wave wrote to LDS is read after this (a wave's LDS operations complete in
// order; this keeps the compiler from moving them)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- the ziplist under construction (ziplist.c:743-839 at the tail) -------------------------------
struct Zl {
    uint64_t pos;    // where the next entry starts
    uint64_t prev;   // the last entry's whole size
    uint64_t last;   // the last entry's offset (zltail)
};
// zipStorePrevEntryLength (ziplist.c:408-419); returns where the encoding starts
template <bool EMIT>
__device__ __forceinline__ uint64_t zl_prevlen(const Zl &z, uint8_t *zb) {
    const uint32_t pls = z.prev < 254 ? 1 : 5;
    if (EMIT && lane_id() == 0) {
        if (pls == 1) zb[z.pos] = (uint8_t)z.prev;
        else {
            zb[z.pos] = 0xFE;
            put_le(zb + z.pos + 1, z.prev, 4);
        }
    }
    return z.pos + pls;
}
__device__ __forceinline__ void zl_advance(Zl &z, uint64_t end) {
    z.prev = end - z.pos;
    z.last = z.pos;
    z.pos = end;
}
// an integer entry (zipTryEncoding's choice :487-498, zipSaveInteger :507-534)
template <bool EMIT>
__device__ __forceinline__ void zl_push_int(Zl &z, uint8_t *zb, int64_t v) {
    const uint64_t q = zl_prevlen<EMIT>(z, zb);
    const uint32_t nb = zint_bytes(v);
    if (EMIT && lane_id() == 0) {
        zb[q] = (uint8_t)zint_enc(v);
        put_le(zb + q + 1, (uint64_t)v, nb);
    }
    zl_advance(z, q + 1 + nb);
}
// a string entry's prevlen and header (zipStoreEntryEncoding :332-364); returns where its bytes go.
// The caller places them and then calls zl_advance(z, that + len).
template <bool EMIT>
__device__ __forceinline__ uint64_t zl_str_hdr(const Zl &z, uint8_t *zb, uint32_t len) {
    const uint64_t q = zl_prevlen<EMIT>(z, zb);
    const uint32_t h = zstr_hdr(len);
    if (EMIT && lane_id() == 0) {
        if (h == 1) zb[q] = (uint8_t)len;
        else if (h == 2) {
            zb[q] = (uint8_t)(0x40 | (len >> 8));
            zb[q + 1] = (uint8_t)len;
        } else {
            zb[q] = 0x80;
            put_be(zb + q + 1, len, 4);
        }
    }
    return q + h;
}
// ziplistPush of a loaded string: zipTryEncoding (:480-504) first.  The integer form is ll2string's
// text, which string2ll takes back; a string of more than 20 bytes cannot pass string2ll.
template <bool EMIT>
__device__ __forceinline__ void zl_push(const Rd &r, const Str &s, Zl &z, uint8_t *zb, lds_u8 *win) {
    int64_t iv = s.iv;
    bool isint = s.kind == S_INT;
    if (!isint && s.len >= 1 && s.len <= 20) isint = str_is_ll(r, materialize(r, s, 20, win), s.len, win, iv);
    if (isint) {
        zl_push_int<EMIT>(z, zb, iv);
        return;
    }
    const uint64_t d = zl_str_hdr<EMIT>(z, zb, s.len);
    if (EMIT) emit_string(r, s, zb + d);
    zl_advance(z, d + s.len);
}

// ---- scores ----------------------------------------------------------------------------------------
// d2string (util.c:517-552) without its %.17g branch: 0 not taken (NaN, or a score for :548), 1 the
// integer iv (ll2string :545; +0 is "0" :530), 2 "inf", 3 "-inf" (:521-524), 4 "-0" (:528)
enum : uint32_t { SC_NO = 0, SC_INT = 1, SC_INF = 2, SC_NINF = 3, SC_NZERO = 4 };
__device__ __forceinline__ uint32_t score_class(uint64_t bits, int64_t &iv) {
    const uint64_t mag = bits & 0x7FFFFFFFFFFFFFFFull;
    iv = 0;
    if (mag > 0x7FF0000000000000ull) return SC_NO;
    if (mag == 0x7FF0000000000000ull) return bits >> 63 ? SC_NINF : SC_INF;
    if (mag == 0) return bits >> 63 ? SC_NZERO : SC_INT;
    const double d = __longlong_as_double((long long)bits);
    if (!(d > -4503599627370495.0 && d < 4503599627370496.0)) return SC_NO;   // :542-544
    const long long t = (long long)d;
    if ((double)t != d) return SC_NO;
    iv = t;
    return SC_INT;
}
// the order of doubles (no NaN) as the order of unsigned integers, -0 with 0
__device__ __forceinline__ uint64_t score_key(uint64_t bits) {
    if ((bits << 1) == 0) bits = 0;
    return bits >> 63 ? ~bits : bits | (1ull << 63);
}

// ---- members, for the tie compare (per lane, each lane its own pair) --------------------------------
// an integer-form member's text (ll2string of an int32: at most 11 bytes), byte k at bits 8k
struct Txt {
    uint64_t lo, hi;
};
__device__ __forceinline__ Txt int_text(int32_t v, uint32_t len) {
    Txt t = {0, 0};
    uint64_t a = v < 0 ? 0ull - (uint64_t)(int64_t)v : (uint64_t)v;
    uint32_t q = len;
    do {
        --q;
        const uint64_t c = '0' + a % 10;
        if (q < 8) t.lo |= c << (8 * q);
        else t.hi |= c << (8 * (q - 8));
        a /= 10;
    } while (a && q);
    if (v < 0) t.lo = (t.lo & ~0xFFull) | '-';
    return t;
}
__device__ __forceinline__ uint32_t member_byte(rsrc_t R, uint32_t off, bool isint, const Txt &t, uint32_t k) {
    if (isint) return (uint32_t)((k < 8 ? t.lo >> (8 * k) : t.hi >> (8 * (k & 7))) & 0xFF);
    return ld8(R, off + k);
}
// sdscmp (sds.c:792-802) of members a and b: < 0, 0, > 0
__device__ __forceinline__ int member_cmp(rsrc_t R, uint32_t ao, uint32_t al, uint32_t bo, uint32_t bl) {
    const bool ai = al & INTF, bi = bl & INTF;
    al &= ~INTF;
    bl &= ~INTF;
    const Txt ta = ai ? int_text((int32_t)ao, al) : Txt{0, 0}, tb = bi ? int_text((int32_t)bo, bl) : Txt{0, 0};
    const uint32_t m = al < bl ? al : bl;
    for (uint32_t k = 0; k < m; ++k) {
        const uint32_t ca = member_byte(R, ao, ai, ta, k), cb = member_byte(R, bo, bi, tb, k);
        if (ca != cb) return ca < cb ? -1 : 1;
    }
    return al < bl ? -1 : al > bl ? 1 : 0;
}

// ---- a ZSet_2 payload's members and scores (rdb.c:1517-1551) ------------------------------------------
// The cnt_in <= MAXN pairs at r.p into key / moff / mlen; false when the value stays the CPU path's.
// CHECK: the size pass's rejections.  FRAC: take every score but NaN; without it only the scores
// score_class prints.
template <bool CHECK, bool FRAC>
__device__ __forceinline__ bool zset_read(Rd &r, uint32_t cnt_in, const Opt &O, const Lds &W) {
    const uint32_t lane = lane_id();
    Str s;
    for (uint32_t k = 0; k < cnt_in; ++k) {
        if (rd_string<CHECK>(r, s)) return false;
        if (s.kind == S_LZF || s.len > O.zset_v) return false;
        if (r.n - r.p < 8) return false;
        const uint64_t bits = le_lanes(ld8(r.R, r.p + lane), 0, 8);   // rdbLoadBinaryDoubleValue
        r.p += 8;
        int64_t iv;
        if (FRAC ? (bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull : score_class(bits, iv) == SC_NO) return false;
        if (lane == 0) {
            W.key[k] = bits;
            W.moff[k] = s.kind == S_INT ? (uint32_t)(int32_t)s.iv : s.off;
            W.mlen[k] = s.len | (s.kind == S_INT ? INTF : 0u);
        }
    }
    return r.p == r.n;
}
// zslInsert's order (t_zset.c:142-145) of what zset_read left: ord[rank] = index, a lane an element
__device__ __forceinline__ void zset_rank_sort(rsrc_t R, const Lds &W, uint32_t cnt_in) {
    wave_sync();
    for (uint32_t i = lane_id(); i < cnt_in; i += RR_WAVE) {
        const uint64_t ki = score_key(W.key[i]);
        const uint32_t io = W.moff[i], il = W.mlen[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < cnt_in; ++j) {
            const uint64_t kj = score_key(W.key[j]);
            bool before = kj < ki;
            if (kj == ki && j != i) {
                const int c = member_cmp(R, W.moff[j], W.mlen[j], io, il);
                before = c < 0 || (c == 0 && j < i);
            }
            rank += before ? 1u : 0u;
        }
        W.ord[rank] = (uint16_t)i;
    }
    wave_sync();
}
// the member at rank k, as zl_push takes it
__device__ __forceinline__ Str zset_member(const Lds &W, uint32_t i) {
    const uint32_t mo = rfl(W.moff[i]), ml = rfl(W.mlen[i]);
    Str s;
    s.kind = ml & INTF ? S_INT : S_RAW;
    s.off = mo;
    s.len = ml & ~INTF;
    s.clen = 0;
    s.iv = (int64_t)(int32_t)mo;
    return s;
}

}  // namespace rr
