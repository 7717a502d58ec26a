// rr_rdbload_device.h — the reader of an RDB value payload, shared by the kernels that walk one
// (rr_rdbload.hip, rr_rdbconvert.hip): the value's slice behind a buffer resource, rdbLoadLen, the
// three string forms of rdbGenericLoadStringObject, the LZF routines and the wave's LDS window.
// Line references are to the reference's rdb.c, lzf_d.c and util.c (include/rr_rdbload.h restates
// the rule).  Everything here is wave-uniform: every lane takes the same path.
//
// The window: a kernel gives each wave WIN bytes of LDS, or fewer when it only ever looks at a
// string's head: src_peek at k == 0 and materialize with need <= 64 touch the first 64 bytes only.
#pragma once
#include "rr_rdb_device.h"
#include "rr_stage_device.h"
#include "../../include/rr_rdbload.h"

namespace rr {

constexpr uint32_t WIN = RR_RDBLOAD_LZF_NODE_MAX;   // a wave's LDS window, bytes

// rr_rdbload_opts as the kernels take it: lru & RR_LRU_MASK, then the five thresholds
struct Opt {
    uint32_t lru, set_ie, hash_e, hash_v, zset_e, zset_v;
};
inline Opt opt_of(const uint32_t *opt6) { return {opt6[0], opt6[1], opt6[2], opt6[3], opt6[4], opt6[5]}; }

// little- and big-endian numbers out of a peeked register: byte i of the number is lane at + i
__device__ __forceinline__ uint64_t le_lanes(uint32_t v, uint32_t at, uint32_t nb) {
    uint64_t x = 0;
    for (uint32_t k = 0; k < nb; ++k) x |= (uint64_t)rl32(v, at + k) << (8 * k);
    return x;
}
__device__ __forceinline__ uint64_t be_lanes(uint32_t v, uint32_t at, uint32_t nb) {
    uint64_t x = 0;
    for (uint32_t k = 0; k < nb; ++k) x = (x << 8) | rl32(v, at + k);
    return x;
}
// ---- the value's slice -------------------------------------------------------------------------
struct Rd {
    rsrc_t R;               // exactly the slice
    const uint8_t *base;    // its first byte (raw pointer: used for ranges the size pass has checked)
    uint32_t n, p;          // its length, the read position
};
// the reader at the start of the slice [o0, o1) of data (slice_ok)
__device__ __forceinline__ Rd rd_of(const uint8_t *data, uint64_t o0, uint64_t o1) {
    return {mk_rsrc(data + o0, (uint32_t)(o1 - o0)), data + o0, (uint32_t)(o1 - o0), 0};
}
// a string as rdbGenericLoadStringObject meets it (rdb.c:487-540)
enum : uint32_t { S_RAW = 0, S_INT = 1, S_LZF = 2 };
struct Str {
    uint32_t kind;
    uint32_t off;     // RAW: the bytes; LZF: the stream (offsets into the slice)
    uint32_t len;     // the loaded string's length (INT: its decimal digits)
    uint32_t clen;    // LZF: the stream's length
    int64_t iv;       // INT
};
// where a string's bytes can be looked at: the slice (a RAW string), or the wave's window
struct Src {
    bool lds;
    uint32_t off;
};

__device__ __forceinline__ uint32_t src_peek(const Rd &r, const Src &s, uint32_t k, const lds_u8 *win) {   // byte k + lane
    const uint32_t lane = lane_id();
    if (s.lds) return k + lane < WIN ? (uint32_t)win[k + lane] : 0u;
    return ld8(r.R, s.off + k + lane);
}

// rdbLoadLen (rdb.c:190-234) out of a peeked register, the length's first byte in lane i, avail
// bytes left in the slice from there.  isenc: the 0xC0 form (val its low 6 bits).
__device__ __forceinline__ uint32_t parse_len(uint32_t v, uint32_t i, uint32_t avail, bool &isenc, uint64_t &val, uint32_t &used) {
    isenc = false;
    val = 0;
    used = 1;
    if (avail < 1) return RR_RDBLOAD_E_TRUNC;
    const uint32_t c = rl32(v, i), t = c >> 6;
    if (t == 3) { isenc = true; val = c & 0x3F; return RR_OK; }           // :197-200
    if (t == 0) { val = c & 0x3F; return RR_OK; }                         // :201-203
    if (t == 1) {                                                         // :204-207
        used = 2;
        if (avail < 2) return RR_RDBLOAD_E_TRUNC;
        val = ((c & 0x3F) << 8) | rl32(v, i + 1);
        return RR_OK;
    }
    if (c == 0x80) {                                                      // :208-212
        used = 5;
        if (avail < 5) return RR_RDBLOAD_E_TRUNC;
        val = be_lanes(v, i + 1, 4);
        return RR_OK;
    }
    if (c == 0x81) {                                                      // :213-217
        used = 9;
        if (avail < 9) return RR_RDBLOAD_E_TRUNC;
        val = be_lanes(v, i + 1, 8);
        return RR_OK;
    }
    return RR_RDBLOAD_E_LEN;                                              // :219
}

// ---- LZF (lzf_d.c:68-184) ------------------------------------------------------------------------
// Does the stream of clen bytes at slice offset `at` decompress to exactly len bytes?  Only control
// bytes are looked at; 64 stream bytes a load.  Every round advances ip.
__device__ __forceinline__ bool lzf_check(rsrc_t R, uint32_t at, uint32_t clen, uint64_t len) {
    const uint32_t lane = lane_id();
    if (clen == 0) return false;
    uint32_t ip = 0, base = 0;
    uint64_t op = 0;
    uint32_t v = ld8(R, at + lane);
    for (;;) {
        if (ip - base + 3 > RR_WAVE) {
            base = ip;
            v = ld8(R, at + base + lane);
        }
        const uint32_t c = rl32(v, ip - base);
        ++ip;
        if (c < 32) {                                      // :72 a literal run of c + 1
            const uint32_t run = c + 1;
            if (op + run > len) return false;              // :76
            if (run > clen - ip) return false;             // :83
            ip += run;
            op += run;
        } else {                                           // :106 a back reference
            uint32_t l = c >> 5;
            if (ip >= clen) return false;                  // :113
            if (l == 7) {
                l += rl32(v, ip - base);                   // :121
                ++ip;
                if (ip >= clen) return false;              // :123
            }
            const uint32_t off = ((c & 0x1F) << 8) + 1 + rl32(v, ip - base);   // :110, :131
            ++ip;
            if (op + l + 2 > len) return false;            // :133
            if (off > op) return false;                    // :139
            op += l + 2;
        }
        if (ip >= clen) break;                             // :185
    }
    return op == len;   // [stricter]: a short result
}

// a valid stream's sequences, one a call: a literal run (ml == 0: run bytes at stream offset from) or
// a back reference (ml bytes at distance off)
struct LzfIt {
    rsrc_t R;
    uint32_t at, clen, ip, base, v;
    __device__ __forceinline__ void init(rsrc_t R_, uint32_t at_, uint32_t clen_) {
        R = R_; at = at_; clen = clen_; ip = 0; base = 0;
        v = ld8(R, at + lane_id());
    }
    __device__ __forceinline__ bool next(uint32_t &from, uint32_t &run, uint32_t &off, uint32_t &ml) {
        if (ip >= clen) return false;
        if (ip - base + 3 > RR_WAVE) {
            base = ip;
            v = ld8(R, at + base + lane_id());
        }
        const uint32_t c = rl32(v, ip - base);
        ++ip;
        if (c < 32) {
            run = c + 1; from = ip; ml = 0; off = 0;
            ip += run;
        } else {
            uint32_t l = c >> 5;
            if (l == 7) { l += rl32(v, ip - base); ++ip; }
            off = ((c & 0x1F) << 8) + 1 + rl32(v, ip - base);
            ++ip;
            ml = l + 2; run = 0; from = 0;
        }
        return true;
    }
};

// the first `limit` (<= WIN) bytes of a valid stream's output into the window
__device__ __forceinline__ void lzf_to_window(rsrc_t R, uint32_t at, uint32_t clen, uint32_t limit, lds_u8 *win) {
    const uint32_t lane = lane_id();
    LzfIt it;
    it.init(R, at, clen);
    uint32_t op = 0, from, run, off, ml;
    while (op < limit && it.next(from, run, off, ml)) {
        if (ml == 0) {
            if (lane < run && op + lane < limit) win[op + lane] = (uint8_t)ld8(R, at + from + lane);
            op += run;
        } else {
            for (uint32_t r0 = 0; r0 < ml; r0 += RR_WAVE) {   // sources lie below op: written by earlier sequences
                const uint32_t j = r0 + lane, k = off >= ml ? j : j % off;
                if (j < ml && op + j < limit) win[op + j] = win[op - off + k];
            }
            op += ml;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// a valid stream's whole output (len bytes) to dst, through a resource that covers exactly it
__device__ __forceinline__ void lzf_to_global(rsrc_t R, uint32_t at, uint32_t clen, uint8_t *dst, uint32_t len) {
    const uint32_t lane = lane_id();
    const rsrc_t O = mk_rsrc(dst, len);
    LzfIt it;
    it.init(R, at, clen);
    uint32_t op = 0, from, run, off, ml;
    while (it.next(from, run, off, ml)) {
        if (ml == 0) {
            if (lane < run) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)ld8(R, at + from + lane), O, (int)(op + lane), 0, 0);
            op += run;
        } else {
            wait_stores();   // the wave's earlier output has reached the L2
            for (uint32_t r0 = 0; r0 < ml; r0 += RR_WAVE) {
                const uint32_t j = r0 + lane, k = off >= ml ? j : j % off;
                const uint8_t x = j < ml ? __builtin_amdgcn_raw_buffer_load_b8(O, (int)(op - off + k), 0, 17) : 0;
                if (j < ml) __builtin_amdgcn_raw_buffer_store_b8(x, O, (int)(op + j), 0, 0);
            }
            op += ml;
        }
    }
}

// ---- strings -------------------------------------------------------------------------------------
// rdbGenericLoadStringObject at r.p.  CHECK (the size pass): every rejection; without it the string
// is known to be valid.  Returns a status; r.p moves behind the string.
template <bool CHECK>
__device__ __forceinline__ uint32_t rd_string(Rd &r, Str &s) {
    s.kind = S_RAW; s.off = 0; s.len = 0; s.clen = 0; s.iv = 0;
    if (r.p >= r.n) return RR_RDBLOAD_E_TRUNC;
    const uint32_t avail = r.n - r.p;
    const uint32_t v = ld8(r.R, r.p + lane_id());
    bool isenc;
    uint64_t val;
    uint32_t used;
    uint32_t st = parse_len(v, 0, avail, isenc, val, used);
    if (st) return st;
    if (!isenc) {                                          // rdb.c:519-539
        if (val > avail - used) return RR_RDBLOAD_E_TRUNC;
        s.off = r.p + used;
        s.len = (uint32_t)val;
        r.p += used + (uint32_t)val;
        return RR_OK;
    }
    if (val <= 2) {                                        // RDB_ENC_INT8 / 16 / 32, :266-302
        const uint32_t w = 1u << (uint32_t)val;
        if (avail < 1 + w) return RR_RDBLOAD_E_TRUNC;
        const uint64_t x = le_lanes(v, 1, w);
        s.kind = S_INT;
        s.iv = w == 1 ? (int64_t)(int8_t)x : w == 2 ? (int64_t)(int16_t)x : (int64_t)(int32_t)x;
        s.len = dec_len(s.iv);
        r.p += 1 + w;
        return RR_OK;
    }
    if (val != 3) return RR_RDBLOAD_E_LEN;                 // :512 unknown string encoding
    uint32_t i = 1, u;
    uint64_t clen, ulen;
    bool ie;
    st = parse_len(v, i, avail - i, ie, clen, u);          // :376 (a count site: the 0xC0 form is its 6 bits)
    if (st) return st;
    i += u;
    st = parse_len(v, i, avail - i, ie, ulen, u);          // :377
    if (st) return st;
    i += u;
    if (clen > avail - i) return RR_RDBLOAD_E_TRUNC;       // :389
    if (CHECK && (ulen >= MAX_SLICE || !lzf_check(r.R, r.p + i, (uint32_t)clen, ulen))) return RR_RDBLOAD_E_LZF;
    s.kind = S_LZF;
    s.off = r.p + i;
    s.clen = (uint32_t)clen;
    s.len = (uint32_t)ulen;
    r.p += i + (uint32_t)clen;
    return RR_OK;
}

// Make the first `need` bytes of the string lookable (need <= WIN unless the string is RAW).
__device__ __forceinline__ Src materialize(const Rd &r, const Str &s, uint32_t need, lds_u8 *win) {
    if (s.kind == S_RAW) return {false, s.off};
    __builtin_amdgcn_wave_barrier();
    if (s.kind == S_INT) {                                 // ll2string's text
        if (lane_id() == 0) {
            uint64_t a = s.iv < 0 ? 0ull - (uint64_t)s.iv : (uint64_t)s.iv;
            uint32_t q = s.len;
            do { win[--q] = (uint8_t)('0' + a % 10); a /= 10; } while (a);
            if (s.iv < 0) win[0] = '-';
        }
    } else {
        lzf_to_window(r.R, s.off, s.clen, need < s.len ? need : s.len, win);
    }
    __builtin_amdgcn_wave_barrier();
    return {true, 0};
}

// string2ll (util.c:360-424) over the len <= 20 bytes at c
__device__ __forceinline__ bool str_is_ll(const Rd &r, const Src &c, uint32_t len, const lds_u8 *win, int64_t &out) {
    if (len == 0 || len > 20) return false;
    const uint32_t v = src_peek(r, c, 0, win);
    const uint32_t c0 = rl32(v, 0);
    if (len == 1 && c0 == '0') { out = 0; return true; }
    uint32_t i = 0;
    bool neg = false;
    if (c0 == '-') {
        neg = true;
        i = 1;
        if (len == 1) return false;
    }
    uint32_t ch = rl32(v, i);
    if (ch < '1' || ch > '9') return false;
    uint64_t x = ch - '0';
    for (++i; i < len; ++i) {
        ch = rl32(v, i);
        if (ch < '0' || ch > '9') return false;
        if (x > (~0ull / 10)) return false;
        x *= 10;
        if (x > (~0ull - (ch - '0'))) return false;
        x += ch - '0';
    }
    if (neg) {
        if (x > (1ull << 63)) return false;
        out = (int64_t)(0ull - x);
    } else {
        if (x > 0x7FFFFFFFFFFFFFFFull) return false;
        out = (int64_t)x;
    }
    return true;
}

// the string's bytes to dst (emit pass)
__device__ __forceinline__ void emit_string(const Rd &r, const Str &s, uint8_t *dst) {
    if (s.kind == S_RAW) wave_copy(dst, r.base + s.off, s.len);
    else if (s.kind == S_INT) { if (lane_id() == 0) dec_write(dst, s.iv); }
    else lzf_to_global(r.R, s.off, s.clen, dst, s.len);
}

}  // namespace rr
