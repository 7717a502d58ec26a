// rr_rdbsave.hip — gfx950 kernels of include/rr_rdbsave.h: flat batch -> the bytes rdbSaveObject
// writes (rdb.c:761-900, `rdbcompression no`).  Five launches: rdb_size_kernel (payload sizes into
// offsets[], per-value status, a List's node count), rr_launch_scan_u64, rdb_emit_kernel (every type
// but the List), rdb_list_kernel<1> and <2> (the Lists, and the call's accounting).
//
// A wave per value in the size and emit kernels, values strided over a capped grid.  A value's descriptors are
// taken 64 a round, one a lane: every lane works out what its descriptor becomes and how many
// bytes it costs, a wave scan places it, the lane writes its header and a body of up to 32 bytes,
// and longer bodies are copied by the whole wave, 16 bytes a lane.
//
// A List is the serial part: whether an entry joins the tail node depends on the node's size so
// far (_quicklistNodeAllowInsert, quicklist.c:420-450), its prevlen field on the entry before it,
// and the width of the rdbSaveLen in front of a node on the node's final size.  The lanes compute
// each entry's body size and size estimate in parallel; the node split and the prevlen chain run
// as a wave-uniform loop over the round's 64 entries, reading the sizes with readlane.  A List
// is walked twice after the scan, a launch each: the first walk parks every node's final size in the first 8 bytes of
// the node's own output (a node with its length prefix is at least 14 bytes), the second reads it
// back when it opens the node, writes the prefix and places the entries behind it.
#include <hip/hip_runtime.h>

#include "rr_device.h"
#include "rr_kernels.h"

using namespace rr;

namespace {

constexpr uint32_t WPB = 4;             // waves (values in flight) per workgroup
constexpr uint32_t GRID_CAP = 16384;    // workgroups: 65536 waves, 256 per CU on 256 CUs (8 rounds of 32 resident)
constexpr uint32_t LIST_GROUP = 8;      // values a wave of rdb_list_kernel looks at per step
constexpr uint32_t SHORT_BODY = 32;     // a body of up to this many bytes is copied by its own lane

typedef uint32_t u32_ua __attribute__((aligned(1)));
struct __attribute__((packed, aligned(1))) u128_ua { uint32_t a, b, c, d; };

struct ElemV {
    uint64_t data;
    uint32_t len, kind;
};
__device__ __forceinline__ ElemV get_elem(const rr_elem *e) {
    const uint4 x = *reinterpret_cast<const uint4 *>(e);
    return {(uint64_t)x.x | ((uint64_t)x.y << 32), x.z, x.w & 0xFF};
}
__device__ __forceinline__ bool in_arena(const ElemV &e, uint64_t acap) { return e.data <= acap && e.len <= acap - e.data; }

__device__ __forceinline__ uint64_t rl64(uint64_t x, uint32_t k) {   // k wave-uniform
    return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, (int)k) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), (int)k) << 32);
}
__device__ __forceinline__ uint32_t rl32(uint32_t x, uint32_t k) { return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)k); }
__device__ __forceinline__ uint64_t first64(uint64_t x) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32);
}

// Wave64 inclusive scan of costs below 2^40 (a cost is at most 2^32 + 8), every lane active: the low
// 24 bits and the rest scanned apart by the u32 DPP scan, which needs no per-step lane predicates
// (the u64 shuffle scan keeps six of them in SGPR pairs, and they spilled here).
__device__ __forceinline__ uint64_t scan_costs(uint64_t x) {
    const uint32_t lo = wave_incl_scan_u32((uint32_t)x & 0xFFFFFFu), hi = wave_incl_scan_u32((uint32_t)(x >> 24));
    return ((uint64_t)hi << 24) + lo;
}

// the sum of every lane's x (all lanes active), in three 24-bit pieces by the same scan
__device__ __forceinline__ uint64_t sum_lanes(uint64_t x) {
    const uint32_t a = wave_incl_scan_u32((uint32_t)x & 0xFFFFFFu), b = wave_incl_scan_u32((uint32_t)(x >> 24) & 0xFFFFFFu),
                   c = wave_incl_scan_u32((uint32_t)(x >> 48));
    return (uint64_t)rl32(a, RR_WAVE - 1) + ((uint64_t)rl32(b, RR_WAVE - 1) << 24) + ((uint64_t)rl32(c, RR_WAVE - 1) << 48);
}

// ---- rdbSaveLen (rdb.c:147-178) ----
__device__ __forceinline__ uint32_t len_bytes(uint64_t len) {
    return len < 64 ? 1u : len < 16384 ? 2u : len <= 0xFFFFFFFFull ? 5u : 9u;
}
// nb <= 8 bytes of v.  Unrolled into eight predicated stores: a loop over a lane's own byte count
// is one more level of divergent control flow, and each level holds an exec mask in an SGPR pair.
__device__ __forceinline__ void put_be(uint8_t *d, uint64_t v, uint32_t nb) {
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        if (k < nb) d[k] = (uint8_t)(v >> (8 * (nb - 1 - k)));
}
__device__ __forceinline__ void put_le(uint8_t *d, uint64_t v, uint32_t nb) {
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        if (k < nb) d[k] = (uint8_t)(v >> (8 * k));
}
__device__ __forceinline__ uint32_t put_len(uint8_t *d, uint64_t len) {
    if (len < 64) { d[0] = (uint8_t)len; return 1; }
    if (len < 16384) { d[0] = (uint8_t)(0x40 | (len >> 8)); d[1] = (uint8_t)len; return 2; }
    if (len <= 0xFFFFFFFFull) { d[0] = 0x80; put_be(d + 1, len, 4); return 5; }
    d[0] = 0x81;
    put_be(d + 1, len, 8);
    return 9;
}
// ---- rdbEncodeInteger (rdb.c:241-261) ----
__device__ __forceinline__ bool is_i32(int64_t v) { return v >= -2147483648ll && v <= 2147483647ll; }
__device__ __forceinline__ uint32_t rint_bytes(int64_t v) { return v >= -128 && v <= 127 ? 2u : v >= -32768 && v <= 32767 ? 3u : 5u; }
__device__ __forceinline__ void put_rint(uint8_t *d, int64_t v) {
    const uint32_t nb = rint_bytes(v) - 1;
    d[0] = (uint8_t)(0xC0 | (nb == 1 ? 0 : nb == 2 ? 1 : 2));
    put_le(d + 1, (uint64_t)v, nb);
}
// rdbSaveRawString's integer branch (rdb.c:416-422, rdbTryIntegerEncoding :307-321): up to 11 bytes
// that are the canonical decimal (what ll2string gives back: string2ll's strict form) of an int32
__device__ __forceinline__ bool raw_is_int(const uint8_t *s, uint32_t len, int64_t &v) {
    return len <= 11 && zip_try_int(s, len, v) && is_i32(v);
}

// ---- ziplist entries (ziplist.c:332-364, :480-534) ----
__device__ __forceinline__ uint32_t zint_bytes(int64_t v) {
    return v >= 0 && v <= 12 ? 0u : v >= -128 && v <= 127 ? 1u : v >= -32768 && v <= 32767 ? 2u
         : v >= -8388608 && v <= 8388607 ? 3u : is_i32(v) ? 4u : 8u;
}
__device__ __forceinline__ uint32_t zint_enc(int64_t v) {
    const uint32_t nb = zint_bytes(v);
    return nb == 0 ? 0xF1u + (uint32_t)v : nb == 1 ? 0xFEu : nb == 2 ? 0xC0u : nb == 3 ? 0xF0u : nb == 4 ? 0xD0u : 0xE0u;
}
__device__ __forceinline__ uint32_t zstr_hdr(uint32_t len) { return len <= 0x3F ? 1u : len <= 0x3FFF ? 2u : 5u; }
// the size estimate _quicklistNodeAllowInsert adds for a pushed string of sz bytes (quicklist.c:425-441)
__device__ __forceinline__ uint64_t ql_estimate(uint64_t sz) {
    return sz + (sz < 254 ? 1 : 5) + (sz < 64 ? 1 : sz < 16384 ? 2 : 5);
}
__device__ __forceinline__ bool ql_allow(uint64_t node_sz, uint64_t est, uint32_t count, int fill) {
    const uint32_t new_sz = (uint32_t)(node_sz + est);   // unsigned int in the reference
    if (fill < 0) return new_sz <= (2048u << (uint32_t)(-fill));   // {4096 .. 65536}[-fill - 1]
    return new_sz <= 8192 && (int)count < fill;
}

// the whole wave copies len bytes (wave-uniform arguments): bytes up to dst's 16-byte boundary, then
// 16 bytes a lane (unaligned loads inside [src, src + len), aligned stores), then the tail bytes
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *__restrict__ src, uint32_t len) {
    const uint32_t lane = lane_id();
    uint32_t head = (uint32_t)(0 - (uintptr_t)dst) & 15;
    if (head > len) head = len;
    if (lane < head) dst[lane] = src[lane];
    const uint32_t body = (len - head) & ~15u;
    dst += head;   // 16-byte aligned from here
    src += head;
    for (uint64_t k = (uint64_t)lane * 16; k < body; k += RR_WAVE * 16) {
        const u128_ua x = *reinterpret_cast<const u128_ua *>(src + k);
        *reinterpret_cast<uint4 *>(dst + k) = make_uint4(x.a, x.b, x.c, x.d);
    }
    if (lane < len - head - body) dst[body + lane] = src[body + lane];
}

// a lane's long bodies, one after the other by the whole wave
__device__ __forceinline__ void copy_long(uint8_t *dst, const uint8_t *__restrict__ src, uint32_t len, bool mine) {
    uint64_t m = __ballot(mine);
    while (m) {
        const uint32_t k = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        wave_copy(reinterpret_cast<uint8_t *>(rl64((uint64_t)(uintptr_t)dst, k)),
                  reinterpret_cast<const uint8_t *>(rl64((uint64_t)(uintptr_t)src, k)), rl32(len, k));
    }
}

struct Batch {
    const rr_elem *__restrict__ elems;
    uint64_t elem_cap;
    const uint8_t *__restrict__ arena;
    uint64_t arena_cap;
    int fill;
};

// ---- every type but the List --------------------------------------------------------------
// Returns the payload's size, 0 for an unsaveable value (no saveable value is empty).  EMIT writes
// it at out; pay adds up the lane's STR / ZLRAW bytes.
template <bool EMIT>
__device__ uint64_t save_plain(const Batch &B, uint32_t type, uint32_t enc, uint32_t eb, uint32_t n, uint8_t *out, uint64_t &pay) {
    const uint32_t lane = lane_id();
    uint32_t used = n;
    uint64_t pos = 0;
    switch (type) {
        case RR_TYPE_STRING:
            if (n != 1 || (enc != RR_ENC_RAW && enc != RR_ENC_INT && enc != RR_ENC_EMBSTR)) return 0;
            break;
        case RR_TYPE_HASH_ZIPLIST:
        case RR_TYPE_ZSET_ZIPLIST:
            if (n < 1) return 0;
            used = 1;
            break;
        case RR_TYPE_SET_HT: pos = len_bytes(n); break;
        case RR_TYPE_HASH_HT:
        case RR_TYPE_ZSET_SKIPLIST:
            if (n & 1) return 0;
            pos = len_bytes(n / 2);
            break;
        case RR_TYPE_SET_INTSET:
            if (enc != 2 && enc != 4 && enc != 8) return 0;
            pos = len_bytes(8 + (uint64_t)n * enc) + 8;
            break;
        default: return 0;
    }
    if (EMIT && lane == 0) {
        if (type == RR_TYPE_SET_HT) put_len(out, n);
        if (type == RR_TYPE_HASH_HT || type == RR_TYPE_ZSET_SKIPLIST) put_len(out, n / 2);
        if (type == RR_TYPE_SET_INTSET) {
            const uint32_t l = put_len(out, 8 + (uint64_t)n * enc);
            put_le(out + l, enc, 4);
            put_le(out + l + 4, n, 4);
        }
    }
    const rr_elem *el = B.elems + eb;
    for (uint32_t left = used; left; left = left > RR_WAVE ? left - RR_WAVE : 0, el += RR_WAVE) {
        const uint32_t j = lane;   // (a pair's member and score keep their parity: rounds are even)
        const bool active = lane < left;
        ElemV e = {0, 0, 0};
        if (active) e = get_elem(el + lane);
        // what the descriptor becomes: 0 raw string, 1 rdb integer, 2 decimal text, 3 fixed LE bytes
        uint32_t form = 0, fixed = 0;
        uint64_t cost = 0;
        int64_t iv = 0;
        bool ok = true;
        if (active) {
            bool want_str = true;
            if (type == RR_TYPE_STRING && enc == RR_ENC_INT) {
                want_str = false;
                ok = e.kind == RR_K_INT;
                iv = (int64_t)e.data;
                form = is_i32(iv) ? 1 : 2;
                cost = form == 1 ? rint_bytes(iv) : 1 + dec_len(iv);
            } else if (type == RR_TYPE_SET_INTSET) {
                want_str = false;
                iv = (int64_t)e.data;
                ok = e.kind == RR_K_INT && (enc == 8 || (iv >= -(1ll << (8 * enc - 1)) && iv < (1ll << (8 * enc - 1))));
                form = 3;
                cost = fixed = enc;
            } else if (type == RR_TYPE_ZSET_SKIPLIST && (j & 1)) {
                want_str = false;
                ok = e.kind == RR_K_SCORE;
                iv = (int64_t)e.data;
                form = 3;
                cost = fixed = 8;
            }
            if (want_str) {
                const bool zl = type == RR_TYPE_HASH_ZIPLIST || type == RR_TYPE_ZSET_ZIPLIST;
                ok = e.kind == (zl ? RR_K_ZLRAW : RR_K_STR) && in_arena(e, B.arena_cap);
                if (ok) {
                    pay += e.len;
                    if (raw_is_int(B.arena + e.data, e.len, iv)) {
                        form = 1;
                        cost = rint_bytes(iv);
                    } else {
                        cost = (uint64_t)len_bytes(e.len) + e.len;
                    }
                }
            }
        }
        if (__ballot(active && !ok)) return 0;
        const uint64_t incl = scan_costs(cost);
        uint8_t *dbody = nullptr;   // where a raw string's bytes go
        if (EMIT && active) {
            uint8_t *d = out + pos + incl - cost;
            if (form == 1) put_rint(d, iv);
            else if (form == 2) dec_write(d + put_len(d, dec_len(iv)), iv);
            else if (form == 3) put_le(d, (uint64_t)iv, fixed);
            else {
                dbody = d + put_len(d, e.len);
                if (e.len <= SHORT_BODY)
                    for (uint32_t k = 0; k < e.len; ++k) dbody[k] = B.arena[e.data + k];
            }
        }
        if (EMIT) copy_long(dbody, B.arena + e.data, e.len, active && form == 0 && e.len > SHORT_BODY);
        pos += rl64(incl, RR_WAVE - 1);
    }
    return pos;
}

// ---- the List -------------------------------------------------------------------------------
// MODE 0: sizes (returns the payload size, nodes = the node count); 1: the emit kernel's first walk
// (parks each node's size at its place in out); 2: its second walk (writes the payload).
// `nodes` is an input of modes 1 and 2.
__device__ __forceinline__ void park_size(uint8_t *p, uint64_t v) {
    if (lane_id() == 0) put_le(p, v, 8);
}
__device__ __forceinline__ uint64_t parked_size(const uint8_t *p) {
    const volatile uint8_t *q = p;
    uint64_t v = 0;
    for (uint32_t k = 0; k < 8; ++k) v |= (uint64_t)q[k] << (8 * k);
    return first64(v);
}

template <int MODE>
__device__ uint64_t save_list(const Batch &B, uint32_t eb, uint32_t n, uint8_t *out, uint32_t &nodes, uint64_t &pay) {
    const uint32_t lane = lane_id();
    // wave-uniform state of the tail node
    bool open = false;
    uint64_t node_sz = 0;       // its ziplist's bytes so far (header and end byte included)
    uint32_t count = 0;
    uint32_t prevraw = 0;       // raw length of its last entry (unsigned int in ziplist.c:745, :760)
    uint32_t tail_rel = 0;      // offset of its last entry in the ziplist (zltail)
    uint64_t node_at = 0;       // where its rdbSaveLen starts in the payload
    uint32_t pfx = 0;           // bytes of the rdbSaveLen in front of its ziplist (MODE 2)
    uint32_t nnodes = 0;
    if (MODE != 0) {
        node_at = len_bytes(nodes);
        if (MODE == 2 && lane == 0) put_len(out, nodes);
    }

    auto close_node = [&]() {
        if (MODE == 1) park_size(out + node_at, node_sz);
        if (MODE == 2 && lane == 0) {
            uint8_t *z = out + node_at + pfx;
            put_le(z, (uint32_t)node_sz, 4);
            put_le(z + 4, tail_rel, 4);
            put_le(z + 8, count, 2);
            z[node_sz - 1] = 0xFF;
        }
        node_at += len_bytes(node_sz) + node_sz;
        ++nnodes;
    };

    const rr_elem *el = B.elems + eb;
    for (uint32_t left = n; left; left = left > RR_WAVE ? left - RR_WAVE : 0, el += RR_WAVE) {
        const bool active = lane < left;
        ElemV e = {0, 0, 0};
        bool ok = true, isint = false;
        int64_t iv = 0;
        uint64_t body = 0, est = 0;
        if (active) {
            e = get_elem(el + lane);
            if (e.kind == RR_K_INT) {           // pushed as its decimal text (sdsll2str), which always parses back
                isint = true;
                iv = (int64_t)e.data;
                est = ql_estimate(dec_len(iv));
            } else if (e.kind == RR_K_STR && in_arena(e, B.arena_cap)) {
                isint = zip_try_int(B.arena + e.data, e.len, iv);
                est = ql_estimate(e.len);
                if (MODE == 2) pay += e.len;
            } else {
                ok = false;
            }
            body = isint ? 1 + zint_bytes(iv) : (uint64_t)zstr_hdr(e.len) + e.len;
        }
        if (__ballot(active && !ok)) return 0;
        const uint32_t cnt = left < RR_WAVE ? left : RR_WAVE;
        uint64_t my_at = 0;
        uint32_t my_prev = 0;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint64_t est_k = rl64(est, k), body_k = rl64(body, k);
            if (!open || !ql_allow(node_sz, est_k, count, B.fill)) {
                if (open) close_node();
                open = true;
                node_sz = 11;
                count = 0;
                prevraw = 0;
                if (MODE == 2) {
                    const uint64_t fin = parked_size(out + node_at);
                    if (lane == 0) put_len(out + node_at, fin);
                    pfx = len_bytes(fin);
                }
            }
            const uint64_t raw = (count == 0 || prevraw < 254 ? 1 : 5) + body_k;
            tail_rel = (uint32_t)(node_sz - 1);
            if (MODE == 2 && lane == k) {
                my_at = node_at + pfx + node_sz - 1;
                my_prev = count == 0 ? 0 : prevraw;
            }
            node_sz += raw;
            prevraw = (uint32_t)raw;
            ++count;
        }
        if (MODE == 2) {
            uint8_t *d = out + my_at;
            if (active) {
                if (my_prev < 254) *d++ = (uint8_t)my_prev;
                else { *d++ = 254; put_le(d, my_prev, 4); d += 4; }
                if (isint) {
                    *d++ = (uint8_t)zint_enc(iv);
                    put_le(d, (uint64_t)iv, zint_bytes(iv));
                } else {
                    if (e.len <= 0x3F) *d++ = (uint8_t)e.len;
                    else if (e.len <= 0x3FFF) { *d++ = (uint8_t)(0x40 | (e.len >> 8)); *d++ = (uint8_t)e.len; }
                    else { *d++ = 0x80; put_be(d, e.len, 4); d += 4; }
                    if (e.len <= SHORT_BODY)
                        for (uint32_t k = 0; k < e.len; ++k) d[k] = B.arena[e.data + k];
                }
            }
            copy_long(d, B.arena + e.data, e.len, active && !isint && e.len > SHORT_BODY);
        }
    }
    if (open) close_node();
    if (MODE == 0) {
        nodes = nnodes;
        return len_bytes(nnodes) + node_at;
    }
    return node_at;
}

__device__ __forceinline__ bool value_ok(const uint4 &x, uint64_t elem_cap) {
    const uint32_t vstatus = (x.x >> 16) & 0xFFFF;
    return vstatus == RR_OK && (uint64_t)x.w + (uint64_t)x.z <= elem_cap;
}

// sizes into offsets[0, n), offsets[n] = 0; status 0 / RR_E_ENCODE; types; a List's node count;
// and the zeroing the other two launches rely on (the scan's look-back words, the error word, totals)
__global__ __launch_bounds__(WPB * RR_WAVE) void rdb_size_kernel(const rr_value *__restrict__ values, uint64_t n, Batch B,
                                                                 uint64_t *__restrict__ offsets, uint8_t *__restrict__ types,
                                                                 uint8_t *__restrict__ status, uint32_t *__restrict__ nnodes,
                                                                 uint64_t *__restrict__ zero, uint64_t nzero, rr_totals *totals) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t k = gtid; k < nzero; k += nthreads) zero[k] = 0;
    if (gtid == 0) {
        offsets[n] = 0;
        totals->n_elems = totals->bytes = totals->n_bad = totals->payload = 0;
    }
    const uint64_t nwaves = nthreads / RR_WAVE;
    uint64_t pay = 0;
    for (uint64_t v = gtid / RR_WAVE; v < n; v += nwaves) {
        const uint4 x = *reinterpret_cast<const uint4 *>(values + v);
        const uint32_t type = x.x & 0xFF, enc = (x.x >> 8) & 0xFF;
        uint64_t size = 0;
        uint32_t nodes = 0;
        if (value_ok(x, B.elem_cap)) {
            if (type == RR_TYPE_LIST_QUICKLIST) {
                size = save_list<0>(B, x.w, x.z, nullptr, nodes, pay);
                if (size == 0) nodes = 0;
            } else {
                size = save_plain<false>(B, type, enc, x.w, x.z, nullptr, pay);
            }
        }
        if (lane_id() == 0) {
            offsets[v] = size;
            types[v] = (uint8_t)type;
            status[v] = size ? RR_OK : RR_E_ENCODE;
            nnodes[v] = nodes;
        }
    }
}

// offsets scanned.  Writes the payloads of the values that fit data_cap, every type but the List
// (rdb_list_kernel), and adds up their STR / ZLRAW bytes.
__global__ __launch_bounds__(WPB * RR_WAVE) void rdb_emit_kernel(const rr_value *__restrict__ values, uint64_t n, Batch B,
                                                                 const uint64_t *__restrict__ offsets, uint8_t *__restrict__ out,
                                                                 uint64_t data_cap, rr_totals *totals) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = nthreads / RR_WAVE;
    uint64_t pay = 0;
    for (uint64_t v = gtid / RR_WAVE; v < n; v += nwaves) {
        const uint4 x = *reinterpret_cast<const uint4 *>(values + v);
        const uint32_t type = x.x & 0xFF, enc = (x.x >> 8) & 0xFF;
        const uint64_t o0 = offsets[v], o1 = offsets[v + 1];
        if (o1 == o0 || o1 > data_cap || type == RR_TYPE_LIST_QUICKLIST) continue;   // unsaveable / does not fit / a List
        save_plain<true>(B, type, enc, x.w, x.z, out + o0, pay);
    }
    pay = sum_lanes(pay);
    if (lane_id() == 0 && pay) atomicAdd((unsigned long long *)&totals->payload, (unsigned long long)pay);
}

// The Lists that the emit kernel left out, in two launches: MODE 1 parks every node's final size at
// the node's place in out, MODE 2 reads it back and writes the payload (the launch boundary orders
// the two).  A wave looks at LIST_GROUP values a step, a lane each, and walks the Lists among them one
// after the other (a small group: the walks of one wave are serial).  MODE 1, which reads every record anyway, also does the call's accounting: a value past
// data_cap gets RR_E_CAPACITY, and rr_totals.n_elems, n_bad and bytes are set.
template <int MODE>
__global__ __launch_bounds__(WPB * RR_WAVE) void rdb_list_kernel(const rr_value *__restrict__ values, uint64_t n, Batch B,
                                                                 const uint64_t *__restrict__ offsets, uint8_t *out,
                                                                 uint64_t data_cap, const uint32_t *__restrict__ nnodes,
                                                                 uint8_t *__restrict__ status, const uint64_t *err, rr_totals *totals) {
    const uint64_t nwaves = (uint64_t)gridDim.x * blockDim.x / RR_WAVE;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / RR_WAVE;
    const uint32_t lane = lane_id();
    uint64_t pay = 0, n_bad = 0, n_el = 0;   // per lane
    if (MODE == 1 && wave == 0 && lane == 0) totals->bytes = *err ? ~0ull : offsets[n];
    for (uint64_t base = wave * LIST_GROUP; base < n; base += nwaves * LIST_GROUP) {
        const uint64_t v = base + lane;
        uint32_t eb = 0, ne = 0, nodes = 0;
        uint64_t o0 = 0;
        bool mine = false;
        if (lane < LIST_GROUP && v < n) {
            const uint4 x = *reinterpret_cast<const uint4 *>(values + v);
            const uint64_t o1 = offsets[v + 1];
            o0 = offsets[v];
            eb = x.w;
            ne = x.z;
            mine = (x.x & 0xFF) == RR_TYPE_LIST_QUICKLIST && o1 > o0 && o1 <= data_cap;   // saveable and it fits
            if (mine) nodes = nnodes[v];
            if (MODE == 1) {
                n_el += ne;
                if (o1 == o0) ++n_bad;                     // RR_E_ENCODE, by the size kernel
                else if (o1 > data_cap) { ++n_bad; status[v] = RR_E_CAPACITY; }
            }
        }
        uint64_t m = __ballot(mine);
        while (m) {
            const uint32_t k = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            uint32_t nd = rl32(nodes, k);
            save_list<MODE>(B, rl32(eb, k), rl32(ne, k), out + rl64(o0, k), nd, pay);
        }
    }
    if (MODE == 1) {
        n_bad = sum_lanes(n_bad);
        n_el = sum_lanes(n_el);
        if (lane == 0 && n_bad) atomicAdd((unsigned long long *)&totals->n_bad, (unsigned long long)n_bad);
        if (lane == 0 && n_el) atomicAdd((unsigned long long *)&totals->n_elems, (unsigned long long)n_el);
    } else {
        pay = sum_lanes(pay);
        if (lane == 0 && pay) atomicAdd((unsigned long long *)&totals->payload, (unsigned long long)pay);
    }
}

uint32_t grid_for(uint64_t n) {
    const uint64_t b = (n + WPB - 1) / WPB;
    return (uint32_t)(b < GRID_CAP ? (b ? b : 1) : GRID_CAP);
}

}  // namespace

// scratch: the scan's look-back words, the error word, then a u32 per value (a List's node count)
extern "C" uint64_t rr_rdbsave_scratch_words(uint64_t n) { return rr_scan_words(n) + 1 + (n + 1) / 2 + 1; }

extern "C" hipError_t rr_launch_rdbsave(const rr_value *values, const rr_elem *elems, uint64_t elem_cap, const uint8_t *arena,
                                        uint64_t arena_cap, uint64_t n, int list_fill, uint8_t *out, uint64_t cap,
                                        uint64_t *offsets, uint8_t *types, uint8_t *status, uint64_t *scratch,
                                        rr_totals *totals, hipStream_t stream) {
    const uint64_t lbw = rr_scan_words(n);
    uint64_t *lb = scratch, *err = scratch + lbw;
    uint32_t *nnodes = reinterpret_cast<uint32_t *>(err + 1);
    const Batch B = {elems, elem_cap, arena, arena_cap, list_fill};
    hipLaunchKernelGGL(rdb_size_kernel, dim3(grid_for(n)), dim3(WPB * RR_WAVE), 0, stream, values, n, B, offsets, types, status,
                       nnodes, lb, lbw + 1, totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(offsets, n, lb, err, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rdb_emit_kernel, dim3(grid_for(n)), dim3(WPB * RR_WAVE), 0, stream, values, n, B,
                       (const uint64_t *)offsets, out, cap, totals);
    e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    const uint32_t lgrid = grid_for((n + LIST_GROUP - 1) / LIST_GROUP);
    hipLaunchKernelGGL(rdb_list_kernel<1>, dim3(lgrid), dim3(WPB * RR_WAVE), 0, stream, values, n, B, (const uint64_t *)offsets, out,
                       cap, (const uint32_t *)nnodes, status, (const uint64_t *)err, totals);
    hipLaunchKernelGGL(rdb_list_kernel<2>, dim3(lgrid), dim3(WPB * RR_WAVE), 0, stream, values, n, B, (const uint64_t *)offsets, out,
                       cap, (const uint32_t *)nnodes, status, (const uint64_t *)err, totals);
    return hipGetLastError();
}
