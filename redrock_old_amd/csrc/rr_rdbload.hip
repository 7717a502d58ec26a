// rr_rdbload.hip — gfx950 kernels of include/rr_rdbload.h: RDB value payloads -> rock blobs (the
// blob desObject turns into the object rdbLoadObject builds, rdb.c:1450-1700).  Three launches:
// rdbload_size_kernel (every decision: status, CONVERT, an LZF stream's validity and exact output
// length; blob sizes into out_offsets[]), rr_launch_scan_u64, rdbload_emit_kernel (the bytes of the
// values that are valid and fit, RR_E_CAPACITY for those that do not, the call's totals).
//
// A wave per value, values strided over a capped grid.  A value is a chain of dependent length
// prefixes, so the walk is wave-uniform: every lane takes the same path, the state lives in scalar
// registers, and the lanes are used where bytes are independent.  A header is read by one 64-byte
// load, a byte a lane, and picked apart with readlane (one memory round trip per string, per
// ziplist entry, per ~20 LZF sequences); bodies are copied by the whole wave, 16 bytes a lane; an
// LZF sequence is copied by the wave, a byte a lane.  Every load of payload bytes in the size pass
// goes through a buffer resource that covers exactly the value's slice, so a corrupt length reads
// zeros, never a neighbour.  The emit pass runs the same walk over values the size pass accepted.
//
// Content the walk has to look at but that is not in the payload as it is — the decimal text of an
// integer-form string, an LZF string — is first put into the wave's LDS window (RR_RDBLOAD_LZF_NODE_MAX
// bytes): a List node in the LZF form is decompressed there and walked there; of an intset blob or a
// ziplist only the header is needed, of a Set member or a String at most 20 bytes.  An LZF string
// that is only copied is decompressed by the emit pass straight into its place in the blob.
#include <hip/hip_runtime.h>

#include "rr_rdb_device.h"
#include "rr_kernels.h"
#include "../../include/rr_rdbload.h"

using namespace rr;

namespace {

constexpr uint32_t WPB = 4;             // waves (values in flight) per workgroup
constexpr uint32_t GRID_CAP = 16384;    // workgroups
constexpr uint32_t WIN = RR_RDBLOAD_LZF_NODE_MAX;   // a wave's LDS window, bytes
constexpr uint32_t MAX_SLICE = 0x7FFFFFF0u;         // a buffer resource's reach
static_assert(WPB * WIN <= 65536 && WIN >= 64, "the windows are static LDS");

struct Opt {
    uint32_t lru, set_ie, hash_e, hash_v, zset_e, zset_v;
};

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

// ---- a List node: the strict ziplist walk (ziplist.c:300-447, parse_ziplist of rr_kernels.hip) ---
// The node's L bytes are at c.  EMIT: every entry as u32 len | bytes at out + pos.
template <bool EMIT>
__device__ __forceinline__ bool walk_node(const Rd &r, const Src &c, uint64_t L, const lds_u8 *win, uint8_t *out, uint64_t &pos,
                                          uint64_t &pay, uint64_t &nel) {
    const uint32_t lane = lane_id();
    if (L < 11) return false;
    uint32_t v = src_peek(r, c, 0, win);
    if (le_lanes(v, 0, 4) != L) return false;
    const uint32_t zltail = (uint32_t)le_lanes(v, 4, 4), zllen = (uint32_t)le_lanes(v, 8, 2);
    uint64_t p = 10, prev_raw = 0, last = 10, cnt = 0, base = 0;
    for (;;) {
        if (p >= L) return false;
        if (p - base + 14 > RR_WAVE) {
            base = p;
            v = src_peek(r, c, (uint32_t)base, win);
        }
        const uint32_t i = (uint32_t)(p - base);
        const uint32_t b0 = rl32(v, i);
        if (b0 == 0xFF) break;
        uint64_t pl;
        uint32_t pls;
        if (b0 < 254) { pl = b0; pls = 1; }
        else {
            if (p + 5 > L - 1) return false;
            pl = le_lanes(v, i + 1, 4);
            pls = 5;
        }
        if (pl != prev_raw) return false;
        const uint64_t q = p + pls;
        if (q >= L - 1) return false;
        const uint32_t enc = rl32(v, i + pls);
        uint64_t end;
        if (enc < 0xC0) {
            const uint32_t cls = enc & 0xC0;
            uint64_t ls, sl;
            if (cls == 0x00) { ls = 1; sl = enc & 0x3F; }
            else if (cls == 0x40) {
                if (q + 2 > L - 1) return false;
                ls = 2;
                sl = ((uint64_t)(enc & 0x3F) << 8) | rl32(v, i + pls + 1);
            } else {
                if (q + 5 > L - 1) return false;
                ls = 5;
                sl = be_lanes(v, i + pls + 1, 4);
            }
            const uint64_t d = q + ls;
            end = d + sl;
            if (end > L - 1) return false;
            if (EMIT) {
                uint8_t *dst = out + pos;
                if (lane == 0) put_le(dst, sl, 4);
                if (c.lds) {
                    for (uint32_t k = lane; k < (uint32_t)sl; k += RR_WAVE) dst[4 + k] = win[(uint32_t)d + k];
                } else {
                    wave_copy(dst + 4, r.base + c.off + d, (uint32_t)sl);
                }
                pay += sl;
            }
            pos += 4 + sl;
        } else {
            uint32_t isz;
            switch (enc) {
                case 0xFE: isz = 1; break;
                case 0xC0: isz = 2; break;
                case 0xF0: isz = 3; break;
                case 0xD0: isz = 4; break;
                case 0xE0: isz = 8; break;
                default:
                    if (enc >= 0xF1 && enc <= 0xFD) isz = 0;
                    else return false;
            }
            end = q + 1 + isz;
            if (end > L - 1) return false;
            const uint64_t x = le_lanes(v, i + pls + 1, isz);
            int64_t iv;
            if (isz == 0) iv = (int64_t)(enc & 0x0F) - 1;
            else if (isz == 8) iv = (int64_t)x;
            else iv = (int64_t)(x << (64 - 8 * isz)) >> (64 - 8 * isz);   // sign-extend isz bytes
            const uint32_t dl = dec_len(iv);
            if (EMIT) {
                if (lane == 0) {
                    put_le(out + pos, dl, 4);
                    dec_write(out + pos + 4, iv);   // sdsll2str
                }
                pay += dl;
            }
            pos += 4 + dl;
        }
        ++cnt;
        prev_raw = end - p;
        last = p;
        p = end;
    }
    if (p != L - 1) return false;
    if (zllen != 0xFFFF && zllen != cnt) return false;
    if (zltail != last) return false;
    nel += cnt;
    return true;
}

// ---- one value -----------------------------------------------------------------------------------
// Returns the blob's size and the status (size pass), or writes the blob at out (EMIT, a value the
// size pass accepted).  pay / nel: rr_totals.payload and n_elems of this value, added.
template <bool EMIT>
__device__ uint64_t load_value(Rd &r, uint32_t type, const Opt &O, lds_u8 *win, uint8_t *out, uint32_t &status, uint64_t &pay,
                               uint64_t &nel) {
    const uint32_t lane = lane_id();
    uint64_t pos = 5;
    bool conv = false;
    uint32_t st = RR_OK;
    Str s;
    if (EMIT && lane == 0) {
        out[0] = (uint8_t)type;
        put_le(out + 1, O.lru, 4);
    }
    if (type == RR_TYPE_STRING) {
        if ((st = rd_string<!EMIT>(r, s))) { status = st; return 0; }
        ++nel;
        bool isint = s.kind == S_INT;
        int64_t iv = s.iv;
        if (!isint && s.len >= 1 && s.len <= 20) {         // tryObjectEncoding, object.c:458
            const Src c = materialize(r, s, 20, win);
            isint = str_is_ll(r, c, s.len, win, iv);
        }
        if (isint) {
            if (EMIT && lane == 0) {
                out[5] = RR_ENC_INT;
                put_le(out + 6, (uint64_t)iv, 8);
            }
            pos = 14;
        } else {
            if (EMIT) {
                if (lane == 0) out[5] = s.len <= RR_EMBSTR_SIZE_LIMIT ? RR_ENC_EMBSTR : RR_ENC_RAW;
                emit_string(r, s, out + 6);
                pay += s.len;
            }
            pos = 6 + (uint64_t)s.len;
        }
    } else if (type == RR_TYPE_SET_HT || type == RR_TYPE_HASH_HT || type == RR_TYPE_ZSET_SKIPLIST) {
        if (r.p >= r.n) { status = RR_RDBLOAD_E_TRUNC; return 0; }
        const uint32_t hv = ld8(r.R, r.p + lane);
        bool ie;
        uint64_t n;
        uint32_t used;
        if ((st = parse_len(hv, 0, r.n - r.p, ie, n, used))) { status = st; return 0; }   // a count site
        r.p += used;
        if (EMIT && lane == 0) put_le(out + 5, n, 8);
        pos = 13;
        const uint32_t per = type == RR_TYPE_HASH_HT ? 2 : 1;
        bool all_int = type == RR_TYPE_SET_HT && n <= O.set_ie;
        uint64_t maxlen = 0;
        for (uint64_t k = 0; k < n; ++k) {
            for (uint32_t j = 0; j < per; ++j) {
                if ((st = rd_string<!EMIT>(r, s))) { status = st; return 0; }
                ++nel;
                if (!EMIT && all_int && s.kind != S_INT) {   // isSdsRepresentableAsLongLong, rdb.c:1501
                    int64_t t;
                    all_int = s.len >= 1 && s.len <= 20 && str_is_ll(r, materialize(r, s, 20, win), s.len, win, t);
                }
                if (s.len > maxlen) maxlen = s.len;
                if (EMIT) {
                    if (lane == 0) put_le(out + pos, s.len, 8);
                    emit_string(r, s, out + pos + 8);
                    pay += s.len;
                }
                pos += 8 + (uint64_t)s.len;
            }
            if (type == RR_TYPE_ZSET_SKIPLIST) {           // rdbLoadBinaryDoubleValue
                if (r.n - r.p < 8) { status = RR_RDBLOAD_E_TRUNC; return 0; }
                if (EMIT && lane < 8) out[pos + lane] = (uint8_t)ld8(r.R, r.p + lane);
                r.p += 8;
                pos += 8;
            }
        }
        if (type == RR_TYPE_SET_HT) conv = all_int;                                        // rdb.c:1481-1506
        else if (type == RR_TYPE_HASH_HT) conv = n <= O.hash_e && maxlen <= O.hash_v;      // :1567-1596
        else conv = n <= O.zset_e && maxlen <= O.zset_v;                                   // :1553-1555
    } else if (type == RR_TYPE_LIST_QUICKLIST) {
        if (r.p >= r.n) { status = RR_RDBLOAD_E_TRUNC; return 0; }
        const uint32_t hv = ld8(r.R, r.p + lane);
        bool ie;
        uint64_t n;
        uint32_t used;
        if ((st = parse_len(hv, 0, r.n - r.p, ie, n, used))) { status = st; return 0; }
        r.p += used;
        for (uint64_t k = 0; k < n; ++k) {
            if ((st = rd_string<!EMIT>(r, s))) { status = st; return 0; }
            ++nel;
            if (s.kind == S_LZF && s.len > WIN) { conv = true; continue; }   // the CPU path's (rr_rdbload.h)
            const Src c = materialize(r, s, WIN, win);
            if (!walk_node<EMIT>(r, c, s.len, win, out, pos, pay, nel)) { status = RR_RDBLOAD_E_ZIPLIST; return 0; }
        }
    } else if (type == RR_TYPE_SET_INTSET) {
        if ((st = rd_string<!EMIT>(r, s))) { status = st; return 0; }
        ++nel;
        if (!EMIT) {
            if (s.len < 8) { status = RR_RDBLOAD_E_ZIPLIST; return 0; }
            const Src c = materialize(r, s, 8, win);
            const uint32_t hv = src_peek(r, c, 0, win);
            const uint64_t enc = le_lanes(hv, 0, 4), cnt = le_lanes(hv, 4, 4);
            if ((enc != 2 && enc != 4 && enc != 8) || (uint64_t)s.len != 8 + enc * cnt) { status = RR_RDBLOAD_E_ZIPLIST; return 0; }
            conv = cnt > O.set_ie;                                                         // rdb.c:1686
        } else {
            emit_string(r, s, out + 5);
            pay += s.len;
        }
        pos = 5 + (uint64_t)s.len;
    } else {   // HASH_ZIPLIST, ZSET_ZIPLIST
        if ((st = rd_string<!EMIT>(r, s))) { status = st; return 0; }
        ++nel;
        if (!EMIT) {
            if (s.len < 11) { status = RR_RDBLOAD_E_ZIPLIST; return 0; }
            const Src c = materialize(r, s, 10, win);
            const uint32_t zllen = (uint32_t)le_lanes(src_peek(r, c, 0, win), 8, 2);
            conv = zllen == 0xFFFF || zllen / 2 > (type == RR_TYPE_HASH_ZIPLIST ? O.hash_e : O.zset_e);   // rdb.c:1692, :1698
        } else {
            if (lane == 0) put_le(out + 5, s.len, 8);
            emit_string(r, s, out + 13);
            pay += s.len;
        }
        pos = 13 + (uint64_t)s.len;
    }
    if (r.p != r.n) { status = RR_RDBLOAD_E_EXTRA; return 0; }
    if (conv) { status = RR_RDBLOAD_E_CONVERT; return 0; }
    status = RR_OK;
    return pos;
}

__device__ __forceinline__ bool known_type(uint32_t t) {
    return t == RR_TYPE_STRING || t == RR_TYPE_SET_HT || t == RR_TYPE_HASH_HT || t == RR_TYPE_ZSET_SKIPLIST ||
           t == RR_TYPE_SET_INTSET || t == RR_TYPE_ZSET_ZIPLIST || t == RR_TYPE_HASH_ZIPLIST || t == RR_TYPE_LIST_QUICKLIST;
}

__device__ __forceinline__ lds_u8 *wave_window() {
    __shared__ uint8_t windows[WPB * WIN];
    return (lds_u8 *)windows + (threadIdx.x / RR_WAVE) * WIN;
}

// blob sizes into out_offs[0, n), out_offs[n] = 0; status; and the zeroing the other two launches
// rely on (the scan's look-back words, the error word, totals)
__global__ __launch_bounds__(WPB * RR_WAVE) void rdbload_size_kernel(const uint8_t *__restrict__ data, uint64_t in_cap,
                                                                     const uint64_t *__restrict__ in_offs,
                                                                     const uint8_t *__restrict__ types, uint64_t n, Opt O,
                                                                     uint64_t *__restrict__ out_offs, uint8_t *__restrict__ status,
                                                                     uint64_t *__restrict__ zero, uint64_t nzero, rr_totals *totals) {
    lds_u8 *win = wave_window();
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t k = gtid; k < nzero; k += nthreads) zero[k] = 0;
    if (gtid == 0) {
        out_offs[n] = 0;
        totals->n_elems = totals->bytes = totals->n_bad = totals->payload = 0;
    }
    const uint64_t nwaves = nthreads / RR_WAVE;
    for (uint64_t v = first64(gtid / RR_WAVE); v < n; v += nwaves) {
        const uint32_t type = rfl(types[v]);
        const uint64_t o0 = first64(in_offs[v]), o1 = first64(in_offs[v + 1]);
        uint32_t st = RR_OK;
        uint64_t size = 0, pay = 0, nel = 0;
        if (!known_type(type)) st = RR_RDBLOAD_E_TYPE;
        else if (o0 > o1 || o1 > in_cap) st = RR_RDBLOAD_E_TRUNC;
        else if (o1 - o0 >= MAX_SLICE) st = RR_RDBLOAD_E_LEN;
        else {
            Rd r = {mk_rsrc(data + o0, (uint32_t)(o1 - o0)), data + o0, (uint32_t)(o1 - o0), 0};
            size = load_value<false>(r, type, O, win, nullptr, st, pay, nel);
        }
        if (lane_id() == 0) {
            out_offs[v] = st ? 0 : size;
            status[v] = (uint8_t)st;
        }
    }
}

// out_offs scanned.  Writes the blobs of the values that are valid and fit out_cap; RR_E_CAPACITY for
// the valid ones that do not; the totals.
__global__ __launch_bounds__(WPB * RR_WAVE) void rdbload_emit_kernel(const uint8_t *__restrict__ data,
                                                                     const uint64_t *__restrict__ in_offs,
                                                                     const uint8_t *__restrict__ types, uint64_t n, Opt O,
                                                                     const uint64_t *__restrict__ out_offs, uint8_t *out, uint64_t out_cap,
                                                                     uint8_t *status, const uint64_t *err, rr_totals *totals) {
    lds_u8 *win = wave_window();
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = nthreads / RR_WAVE;
    if (gtid == 0) totals->bytes = *err ? ~0ull : out_offs[n];
    uint64_t pay = 0, nel = 0, n_bad = 0;   // wave-uniform
    for (uint64_t v = first64(gtid / RR_WAVE); v < n; v += nwaves) {
        const uint32_t type = rfl(types[v]);
        uint32_t st = rfl(status[v]);
        if (st) { ++n_bad; continue; }
        const uint64_t b0 = first64(out_offs[v]), b1 = first64(out_offs[v + 1]);
        if (b1 > out_cap) {
            ++n_bad;
            if (lane_id() == 0) status[v] = RR_E_CAPACITY;
            continue;
        }
        const uint64_t o0 = first64(in_offs[v]), o1 = first64(in_offs[v + 1]);
        Rd r = {mk_rsrc(data + o0, (uint32_t)(o1 - o0)), data + o0, (uint32_t)(o1 - o0), 0};
        load_value<true>(r, type, O, win, out + b0, st, pay, nel);
    }
    if (lane_id() == 0) {
        if (pay) atomicAdd((unsigned long long *)&totals->payload, (unsigned long long)pay);
        if (nel) atomicAdd((unsigned long long *)&totals->n_elems, (unsigned long long)nel);
        if (n_bad) atomicAdd((unsigned long long *)&totals->n_bad, (unsigned long long)n_bad);
    }
}

uint32_t grid_for(uint64_t n) {
    const uint64_t b = (n + WPB - 1) / WPB;
    return (uint32_t)(b < GRID_CAP ? (b ? b : 1) : GRID_CAP);
}

}  // namespace

// scratch: the scan's look-back words and the error word
extern "C" uint64_t rr_rdbload_scratch_words(uint64_t n) { return rr_scan_words(n) + 1; }

extern "C" hipError_t rr_launch_rdbload(const uint8_t *data, uint64_t in_cap, const uint64_t *in_offs, const uint8_t *types,
                                        uint64_t n, const uint32_t *opt6, uint8_t *out, uint64_t out_cap, uint64_t *out_offs,
                                        uint8_t *status, uint64_t *scratch, rr_totals *totals, hipStream_t stream) {
    const uint64_t lbw = rr_scan_words(n);
    uint64_t *lb = scratch, *err = scratch + lbw;
    const Opt O = {opt6[0], opt6[1], opt6[2], opt6[3], opt6[4], opt6[5]};
    hipLaunchKernelGGL(rdbload_size_kernel, dim3(grid_for(n)), dim3(WPB * RR_WAVE), 0, stream, data, in_cap, in_offs, types, n, O,
                       out_offs, status, lb, lbw + 1, totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(out_offs, n, lb, err, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rdbload_emit_kernel, dim3(grid_for(n)), dim3(WPB * RR_WAVE), 0, stream, data, in_offs, types, n, O,
                       (const uint64_t *)out_offs, out, out_cap, status, (const uint64_t *)err, totals);
    return hipGetLastError();
}
