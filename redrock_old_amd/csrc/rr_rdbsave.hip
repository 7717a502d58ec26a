// rr_rdbsave.hip — gfx950 kernels of include/rr_rdbsave.h: flat batch -> the bytes rdbSaveObject
// writes (rdb.c:761-900; with RR_RDBSAVE_LZF its strings in the LZF form, "LZF" below).  Five launches: rdb_size_kernel (payload sizes into
// offsets[], per-value status, a List's node count), rr_launch_scan_u64, rdb_emit_kernel (every type
// but the List), rdb_list_kernel<1> and <2> (the Lists, and the call's accounting).
//
// The stage's shape is rr_stage_device.h's (size, scan, emit), with loops of its own: a value's index
// is not made wave-uniform here, the Lists have launches of their own, and the size and emit kernels
// come in an LZF instantiation each.  The leaves (the zeroing, scan_costs, sum_lanes, copy_bodies,
// value_ok, the grid) are the shared ones.
//
// A wave per value in the size and emit kernels.  A value's descriptors are
// taken 64 a round, one a lane: every lane works out what its descriptor becomes and how many
// bytes it costs, a wave scan places it, the lane writes its header, and the bodies are copy_bodies'.
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

#include "rr_flat_device.h"
#include "rr_rdb_device.h"
#include "rr_stage_device.h"

using namespace rr;

namespace {

constexpr uint32_t WPB = 4;             // waves (values in flight) per workgroup
constexpr uint32_t GRID_CAP = 16384;    // workgroups: 65536 waves, 256 per CU on 256 CUs (8 rounds of 32 resident)
constexpr uint32_t LIST_GROUP = 8;      // values a wave of rdb_list_kernel looks at per step

// the size estimate _quicklistNodeAllowInsert adds for a pushed string of sz bytes (quicklist.c:425-441)
__device__ __forceinline__ uint64_t ql_estimate(uint64_t sz) {
    return sz + (sz < 254 ? 1 : 5) + (sz < 64 ? 1 : sz < 16384 ? 2 : 5);
}
__device__ __forceinline__ bool ql_allow(uint64_t node_sz, uint64_t est, uint32_t count, int fill) {
    const uint32_t new_sz = (uint32_t)(node_sz + est);   // unsigned int in the reference
    if (fill < 0) return new_sz <= (2048u << (uint32_t)(-fill));   // {4096 .. 65536}[-fill - 1]
    return new_sz <= 8192 && (int)count < fill;
}

// ---- LZF (rdbSaveLzfStringObject, rdb.c:348-364; the stream format of lzf_d.c:68-184) -------
// One string a wave, the strings of a round one after the other (lz4_comp_kernel's structure, rr_lz4.hip).
// 64 consecutive positions a round: every lane takes the 3 bytes at its position and looks for
// an earlier position with the same 3 bytes, first among the lower lanes of the round (a direct
// lane-against-lane search, nearest first: the only search a string of up to 64 bytes gets, and
// what finds the period of a run), then in an LDS table of the latest position of each hash.  The
// first lane with a match wins, the wave extends it (up to 264 bytes), the literals in front of it
// and the back reference are written, and the next round starts behind the match.
//
// Short strings: a table entry is generation << 16 | position, and an entry of another generation
// reads as empty, so a string does not clear the table; it takes a new generation (a wave clears
// its table before its first string and once every 65,535 generations).  A position is relative to
// the string's current 64 KiB chunk, and a chunk takes a new generation too.
//
// Nothing depends on timing, on addresses or on what the table held before: the table's update is
// a maximum (insert_latest), entries of other generations are never matched, source bytes are
// read a byte at a time through a buffer resource that covers exactly the string.  So a string's
// stream is a function of its bytes, and the size pass and the emit pass, which both run this
// code, agree on it.  Every loop advances ip or exits.
#ifndef RR_LZF_HASH_LOG
#define RR_LZF_HASH_LOG 11             // log2 of the table's entries (u32): 8 KiB of LDS a wave at 11
#endif
constexpr uint32_t LZF_HLOG = RR_LZF_HASH_LOG, LZF_HSIZE = 1u << LZF_HLOG;
static_assert(LZF_HLOG >= 6 && LZF_HLOG <= 13, "LZF hash table: WPB * 4 << log bytes of LDS a workgroup");
constexpr uint32_t LZF_MIN_LEN = 21;           // rdb.c:426: len > 20
constexpr uint32_t LZF_MAX_LEN = 0x7FFFFFF0u;  // a buffer resource's reach; longer strings stay raw
constexpr uint32_t LZF_WINDOW = 8192, LZF_MAX_MATCH = 264, LZF_RUN = 32, LZF_CHUNK = 1u << 16;

__device__ __forceinline__ uint32_t lzf_ld24(rsrc_t R, uint32_t k) {
    return ld8(R, k) | (ld8(R, k + 1) << 8) | (ld8(R, k + 2) << 16);
}
__device__ __forceinline__ uint32_t lzf_hash(uint32_t x) { return (x * 2654435761u) >> (32 - LZF_HLOG); }

// tab[h] = the largest of the words the lanes with `ins` hold for h (all above what the table
// holds).  Lanes with the same hash store to the same entry and one of them lands; the lanes that
// hold a larger word store again, so the result is the maximum whichever store the hardware lets
// win.  At most 64 passes.
__device__ __forceinline__ void insert_latest(lds_u32 *tab, bool ins, uint32_t h, uint32_t word) {
    for (;;) {
        const uint32_t cur = ins ? tab[h] : 0u;
        ins = ins && cur < word;
        if (!__ballot(ins)) return;
        if (ins) tab[h] = word;
    }
}

struct Lzf {
    lds_u32 *tab;    // the wave's table
    uint32_t gen;    // the generation in use; 0: the table has not been cleared yet
    __device__ __forceinline__ void next_gen() {
        if (gen == 0 || gen == 0xFFFFu) {
            for (uint32_t k = lane_id(); k < LZF_HSIZE; k += RR_WAVE) tab[k] = 0;
            gen = 0;
        }
        ++gen;
    }
};

// One sequence at stream position op: lits literal bytes from `from` in runs of up to 32
// (lzf_d.c:77-101: a control byte c < 32, then c + 1 bytes), then (ml != 0) a back reference of ml
// bytes at distance off (lzf_d.c:103-160: l = ml - 2 in the control byte's top 3 bits, 7 meaning
// 7 + the next byte; then off - 1 in 13 bits).  Returns the bytes it takes.
template <bool WRITE>
__device__ __forceinline__ uint32_t lzf_sequence(rsrc_t R, rsrc_t O, uint32_t op, uint32_t from, uint32_t lits, uint32_t off,
                                                 uint32_t ml) {
    const uint32_t lane = lane_id();
    const uint32_t nl = lits + (lits + LZF_RUN - 1) / LZF_RUN;
    const uint32_t l = ml - 2, nm = ml == 0 ? 0u : l < 7 ? 2u : 3u;
    if (WRITE) {
        for (uint32_t k = lane; k < lits; k += RR_WAVE) {
            const uint32_t at = op + k + k / LZF_RUN;
            if (k % LZF_RUN == 0) {
                const uint32_t run = lits - k < LZF_RUN ? lits - k : LZF_RUN;
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(run - 1), O, (int)at, 0, 0);
            }
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)ld8(R, from + k), O, (int)(at + 1), 0, 0);
        }
        const uint32_t o = off - 1;
        const uint32_t v = l < 7 ? ((l << 5) | (o >> 8)) | ((o & 0xFF) << 8)
                                 : (0xE0u | (o >> 8)) | ((l - 7) << 8) | ((o & 0xFF) << 16);
        if (lane < nm) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(v >> (8 * lane)), O, (int)(op + nl + lane), 0, 0);
    }
    return nl + nm;
}

// The LZF stream of the len bytes at src (wave-uniform arguments, LZF_MIN_LEN <= len <
// LZF_MAX_LEN, the bytes inside the arena).  Returns its length, or 0 when it would pass len - 4
// (rdb.c:354-359: the string is then written raw).  WRITE: the stream goes to dst, which has room
// for `room` bytes (what the size pass returned; stores past it are dropped by the resource).
template <bool WRITE>
__device__ __forceinline__ uint32_t lzf_compress(Lzf &Z, const uint8_t *src, uint32_t len, uint8_t *dst, uint32_t room) {
    const uint32_t lane = lane_id();
    const rsrc_t R = mk_rsrc(src, len), O = mk_rsrc(dst, WRITE ? room : 0u);
    const uint32_t most = len - 4;
    uint32_t ip = 0, anchor = 0, op = 0, cb = 0;
    Z.next_gen();
    while (ip + 3 <= len) {
        if (ip - cb >= LZF_CHUNK) {   // a new 64 KiB chunk; pending literals carry over
            cb = ip;
            Z.next_gen();
        }
        const uint32_t P = ip + lane;
        const bool valid = P + 3 <= len && P - cb < LZF_CHUNK;
        const uint32_t x = valid ? lzf_ld24(R, P) : 0u, h = lzf_hash(x);
        // the nearest lower lane of the round with the same 3 bytes (a lower lane of a valid one is valid)
        uint32_t near = 0;
        for (uint32_t d = 1; d < RR_WAVE; ++d) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, d, RR_WAVE);
            if (valid && near == 0 && lane >= d && y == x) near = d;
            if (!__ballot(valid && near == 0 && lane > d)) break;
        }
        // else the latest position of the earlier rounds with this hash
        const uint32_t e = valid && near == 0 ? Z.tab[h] : 0u;
        const uint32_t c = near ? P - near : cb + (e & 0xFFFFu);
        const bool may = valid && near == 0 && (e >> 16) == Z.gen && c < P && P - c <= LZF_WINDOW;
        const bool hit = near != 0 || (may && lzf_ld24(R, c) == x);
        const uint64_t bal = __ballot(hit);
        const uint32_t sl = bal ? (uint32_t)__builtin_ctzll(bal) : RR_WAVE;
        insert_latest(Z.tab, valid && lane <= sl, h, (Z.gen << 16) | (P - cb));
        __builtin_amdgcn_wave_barrier();
        if (!bal) {
            ip += RR_WAVE;
            const uint32_t lits = (ip < len ? ip : len) - anchor;
            if (op + lits + (lits + LZF_RUN - 1) / LZF_RUN > most) return 0;
            continue;
        }
        const uint32_t ms = ip + sl, mc = rl32(c, sl);
        // bytes equal behind the first 3, up to 264 in all and the string's end; 64 lanes a step
        uint32_t ml = 3;
        for (;;) {
            const uint32_t k = ml + lane;
            const bool stop = k >= LZF_MAX_MATCH || ms + k >= len || ld8(R, mc + k) != ld8(R, ms + k);
            const uint64_t sb = __ballot(stop);
            if (sb) { ml += (uint32_t)__builtin_ctzll(sb); break; }
            ml += RR_WAVE;
        }
        op += lzf_sequence<WRITE>(R, O, op, anchor, ms - anchor, ms - mc, ml);
        if (op > most) return 0;
        ip = ms + ml;
        anchor = ip;
    }
    if (anchor < len) op += lzf_sequence<WRITE>(R, O, op, anchor, len - anchor, 0, 0);
    return op <= most ? op : 0;
}

struct Batch {
    const rr_elem *__restrict__ elems;
    uint64_t elem_cap;
    const uint8_t *__restrict__ arena;
    uint64_t arena_cap;
    int fill;
};

// What the LZF instantiations keep beside the batch: the wave's compressor, and a u32 per
// descriptor in the context's scratch where the size pass leaves the stream length of the
// descriptor's string (0: written raw) for the emit pass.  Values that share a descriptor store the
// same number there: it depends on the descriptor's bytes only.
struct LzfCtx {
    Lzf Z;
    uint32_t *clens;
};

// ---- every type but the List --------------------------------------------------------------
// Returns the payload's size, 0 for an unsaveable value (no saveable value is empty).  EMIT writes
// it at out; pay adds up the lane's STR / ZLRAW bytes.  LZF: every rdbSaveRawString site of more than
// 20 bytes tries the LZF form (rdb.c:426-431); the round's eligible strings are compressed by the
// whole wave one after the other, in the size pass to learn their cost, in the emit pass to their place.
template <bool EMIT, bool LZF>
__device__ uint64_t save_plain(const Batch &B, LzfCtx &X, uint32_t type, uint32_t enc, uint32_t eb, uint32_t n, uint8_t *out,
                               uint64_t &pay) {
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
        // what the descriptor becomes: 0 raw string, 1 rdb integer, 2 decimal text, 3 fixed LE bytes,
        // 4 LZF string
        uint32_t form = 0, fixed = 0, clen = 0;
        bool is_str = false;
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
                    is_str = true;
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
        if (LZF) {
            const bool elig = is_str && form == 0 && e.len >= LZF_MIN_LEN && e.len < LZF_MAX_LEN;
            uint32_t *slot = X.clens + eb + (uint32_t)(el - (B.elems + eb)) + lane;
            if (EMIT) {
                if (elig) clen = *slot;
            } else {
                uint64_t m = __ballot(elig);
                while (m) {
                    const uint32_t k = (uint32_t)__builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t c = lzf_compress<false>(X.Z, B.arena + rl64(e.data, k), rl32(e.len, k), nullptr, 0);
                    if (lane == k) clen = c;
                }
                if (elig) *slot = clen;
            }
            if (clen) {   // 0xC3 | rdbSaveLen(clen) | rdbSaveLen(len) | stream (rdbSaveLzfBlob, rdb.c:323-346)
                form = 4;
                cost = 1 + (uint64_t)len_bytes(clen) + len_bytes(e.len) + clen;
            }
        }
        const uint64_t incl = scan_costs(cost);
        uint8_t *dbody = nullptr;   // where a raw string's bytes go
        if (EMIT && active) {
            uint8_t *d = out + pos + incl - cost;
            if (form == 1) put_rint(d, iv);
            else if (form == 2) dec_write(d + put_len(d, dec_len(iv)), iv);
            else if (form == 3) put_le(d, (uint64_t)iv, fixed);
            else if (LZF && form == 4) {
                d[0] = 0xC3;   // (RDB_ENCVAL << 6) | RDB_ENC_LZF
                d += 1 + put_len(d + 1, clen);
                dbody = d + put_len(d, e.len);
            } else {
                dbody = d + put_len(d, e.len);
            }
        }
        if (EMIT) copy_bodies(dbody, B.arena + e.data, e.len, active && form == 0);
        if (EMIT && LZF) {
            uint64_t m = __ballot(active && form == 4);
            while (m) {
                const uint32_t k = (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                lzf_compress<true>(X.Z, B.arena + rl64(e.data, k), rl32(e.len, k),
                                   reinterpret_cast<uint8_t *>(rl64((uint64_t)(uintptr_t)dbody, k)), rl32(clen, k));
            }
        }
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
                }
            }
            copy_bodies(d, B.arena + e.data, e.len, active && !isint);
        }
    }
    if (open) close_node();
    if (MODE == 0) {
        nodes = nnodes;
        return len_bytes(nnodes) + node_at;
    }
    return node_at;
}

// the LZF instantiations' per-wave state: a table of the workgroup's LDS each (none without LZF)
template <bool LZF>
__device__ __forceinline__ LzfCtx lzf_ctx(uint32_t *clens) {
    LzfCtx X = {{nullptr, 0}, clens};
    if constexpr (LZF) {
        __shared__ uint32_t lzf_tabs[WPB * LZF_HSIZE];
        X.Z.tab = (lds_u32 *)lzf_tabs + (threadIdx.x / RR_WAVE) * LZF_HSIZE;
    }
    return X;
}

// sizes into offsets[0, n), offsets[n] = 0; status 0 / RR_E_ENCODE; types; a List's node count;
// and the stage's zeroing.
// LZF: also the stream length of every eligible string, into clens.
template <bool LZF>
__global__ __launch_bounds__(WPB * RR_WAVE) void rdb_size_kernel(const rr_value *__restrict__ values, uint64_t n, Batch B,
                                                                 uint64_t *__restrict__ offsets, uint8_t *__restrict__ types,
                                                                 uint8_t *__restrict__ status, uint32_t *__restrict__ nnodes,
                                                                 uint64_t *__restrict__ zero, uint64_t nzero, rr_totals *totals,
                                                                 uint32_t *clens) {
    LzfCtx X = lzf_ctx<LZF>(clens);
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    zero_stage_words(gtid, nthreads, zero, nzero, &offsets[n], totals);
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
                size = save_plain<false, LZF>(B, X, type, enc, x.w, x.z, nullptr, pay);
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
template <bool LZF>
__global__ __launch_bounds__(WPB * RR_WAVE) void rdb_emit_kernel(const rr_value *__restrict__ values, uint64_t n, Batch B,
                                                                 const uint64_t *__restrict__ offsets, uint8_t *__restrict__ out,
                                                                 uint64_t data_cap, rr_totals *totals, uint32_t *clens) {
    LzfCtx X = lzf_ctx<LZF>(clens);
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = nthreads / RR_WAVE;
    uint64_t pay = 0;
    for (uint64_t v = gtid / RR_WAVE; v < n; v += nwaves) {
        const uint4 x = *reinterpret_cast<const uint4 *>(values + v);
        const uint32_t type = x.x & 0xFF, enc = (x.x >> 8) & 0xFF;
        const uint64_t o0 = offsets[v], o1 = offsets[v + 1];
        if (o1 == o0 || o1 > data_cap || type == RR_TYPE_LIST_QUICKLIST) continue;   // unsaveable / does not fit / a List
        save_plain<true, LZF>(B, X, type, enc, x.w, x.z, out + o0, pay);
    }
    add_totals(totals, sum_lanes(pay), 0, 0);
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
        add_totals(totals, sum_lanes(pay), 0, 0);
    }
}

}  // namespace

// scratch: the scan's look-back words, the error word, then a u32 per value (a List's node count),
// then, with RR_RDBSAVE_LZF only (lzf_elems = elem_cap, else 0), a u32 per descriptor (LzfCtx)
extern "C" uint64_t rr_rdbsave_scratch_words(uint64_t n, uint64_t lzf_elems) {
    return rr_scan_words(n) + 1 + (n + 1) / 2 + 1 + (lzf_elems + 1) / 2;
}

extern "C" hipError_t rr_launch_rdbsave(const rr_value *values, const rr_elem *elems, uint64_t elem_cap, const uint8_t *arena,
                                        uint64_t arena_cap, uint64_t n, int list_fill, int lzf, uint8_t *out, uint64_t cap,
                                        uint64_t *offsets, uint8_t *types, uint8_t *status, uint64_t *scratch,
                                        rr_totals *totals, hipStream_t stream) {
    const uint64_t lbw = rr_scan_words(n);
    uint64_t *lb = scratch, *err = scratch + lbw;
    uint32_t *nnodes = reinterpret_cast<uint32_t *>(err + 1);
    uint32_t *clens = lzf ? reinterpret_cast<uint32_t *>(err + 1 + (n + 1) / 2 + 1) : nullptr;
    const Batch B = {elems, elem_cap, arena, arena_cap, list_fill};
    const uint32_t grid = capped_grid(n, WPB, GRID_CAP);   // a wave a value
    hipLaunchKernelGGL(lzf ? rdb_size_kernel<true> : rdb_size_kernel<false>, dim3(grid), dim3(WPB * RR_WAVE), 0, stream,
                       values, n, B, offsets, types, status, nnodes, lb, lbw + 1, totals, clens);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(offsets, n, lb, err, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf ? rdb_emit_kernel<true> : rdb_emit_kernel<false>, dim3(grid), dim3(WPB * RR_WAVE), 0, stream,
                       values, n, B, (const uint64_t *)offsets, out, cap, totals, clens);
    e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    const uint32_t lgrid = capped_grid(n, WPB * LIST_GROUP, GRID_CAP);
    hipLaunchKernelGGL(rdb_list_kernel<1>, dim3(lgrid), dim3(WPB * RR_WAVE), 0, stream, values, n, B, (const uint64_t *)offsets, out,
                       cap, (const uint32_t *)nnodes, status, (const uint64_t *)err, totals);
    hipLaunchKernelGGL(rdb_list_kernel<2>, dim3(lgrid), dim3(WPB * RR_WAVE), 0, stream, values, n, B, (const uint64_t *)offsets, out,
                       cap, (const uint32_t *)nnodes, status, (const uint64_t *)err, totals);
    return hipGetLastError();
}
