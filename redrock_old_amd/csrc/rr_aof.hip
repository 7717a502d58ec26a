// rr_aof.hip — gfx950 kernels of include/rr_aof.h: flat batch -> the RESP commands
// rewriteAppendOnlyFileRio writes (aof.c:1302-1389, :921-1135).  The stage is rr_stage_device.h's
// (size, scan, emit): aof_size_kernel, aof_emit_kernel.
//
// One command of up to 64 items
// is one wave round: lane j takes item j (one descriptor, or a pair), works out its one or two bulk
// strings and what they cost, a wave scan places the item behind the command's head, the lane writes
// its "$len\r\n" heads, its decimals and score texts, and the bodies are copy_bodies'.
// The command's head ("*argc", the verb, the key) is lane
// 0's, the key's bytes the whole wave's.
//
// A score is printed by rr_d2string_impl.h, a lane a score, and a ziplist's score entry is read by
// rr_strtod_impl.h first; both keep their multi-word state in LDS, lane l's word k at [64 k + l], and
// the text goes to a 32-byte LDS slot per lane, as in rr_rdbzset.hip.  The size pass and the emit
// pass run the same statements, so they agree on every length.
//
// A wave's LDS is the states (8704) + the slots (2048) = 10752 bytes, four waves a workgroup.
#include <hip/hip_runtime.h>

#include "rr_flat_device.h"
#include "rr_stage_device.h"
#include "../../include/rr_aof.h"
#include "../../include/rr_d2string.h"

#define RR_D2S_FN __device__ __forceinline__
#define RR_D2S_WORD rr::lds_u32
#define RR_D2S_STRIDE RR_WAVE
#define RR_D2S_CHAR rr::lds_u8
#include "rr_strtod_impl.h"

using namespace rr;

namespace {

constexpr uint32_t WPB = 4;                                    // waves (values in flight) per workgroup
constexpr uint32_t GRID_CAP = RR_AOF_MAX_WAVES / WPB;
constexpr uint32_t SLOT = RR_D2STRING_SLOT;
constexpr uint32_t BIG_LDS = 4 * RR_D2S_WORDS * RR_WAVE, TXT_LDS = SLOT * RR_WAVE, WAVE_LDS = BIG_LDS + TXT_LDS;
static_assert(RR_D2STRING_MAX < SLOT && WPB * WAVE_LDS <= 65536, "static LDS");
static_assert(RR_AOF_ITEMS_PER_CMD == RR_WAVE, "a command is one wave round");

struct Batch {
    const rr_elem *__restrict__ elems;
    uint64_t elem_cap;
    const uint8_t *__restrict__ arena;
    uint64_t arena_cap;
};
struct Lds {
    lds_u32 *big;   // this lane's state
    lds_u8 *txt;    // this lane's slot
};

// ---- rio.c:406-445 ----
__device__ __forceinline__ uint32_t ndig(uint32_t v) { return dec_len((int64_t)v); }
// "$len\r\n" | len bytes | "\r\n"
__device__ __forceinline__ uint64_t bulk_cost(uint32_t len) { return 5ull + ndig(len) + len; }
__device__ __forceinline__ uint8_t *put_crlf(uint8_t *d) {
    d[0] = '\r';
    d[1] = '\n';
    return d + 2;
}
__device__ __forceinline__ uint8_t *put_count(uint8_t *d, uint8_t prefix, uint32_t v) {   // rioWriteBulkCount
    *d++ = prefix;
    d += dec_write(d, (int64_t)v);
    return put_crlf(d);
}
__device__ __forceinline__ uint8_t *put_lit(uint8_t *d, const char *s, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) d[k] = (uint8_t)s[k];
    return d + n;
}

// a lane's bulk string: nothing, len arena bytes at data, the decimal of (int64) data, or the len
// bytes of the lane's text slot
enum : uint32_t { B_NONE = 0, B_BYTES = 1, B_INT = 2, B_TEXT = 3 };
struct Bulk {
    uint32_t kind, len;
    uint64_t data;
};
__device__ __forceinline__ Bulk bulk_of(const ElemV &e) {
    if (e.kind == RR_K_INT) return {B_INT, dec_len((int64_t)e.data), e.data};
    return {B_BYTES, e.len, e.data};
}
__device__ __forceinline__ uint64_t cost_of(const Bulk &b) { return b.kind == B_NONE ? 0 : bulk_cost(b.len); }
// writes the bulk at d but for a body of arena bytes, whose place is *body (copy_bodies)
__device__ __forceinline__ uint8_t *put_bulk(uint8_t *d, const Bulk &b, const Lds &Z, uint8_t *&body) {
    body = nullptr;
    if (b.kind == B_NONE) return d;
    d = put_count(d, '$', b.len);
    if (b.kind == B_INT) dec_write(d, (int64_t)b.data);
    else if (b.kind == B_TEXT) {
        for (uint32_t k = 0; k < b.len; ++k) d[k] = Z.txt[k];
    } else {
        body = d;
    }
    return put_crlf(d + b.len);
}

struct Verb {
    const char *text;   // the verb's bulk string
    uint32_t len;
};

// the command's head: "*argc\r\n" | verb | the key's bulk string
__device__ __forceinline__ uint64_t head_cost(uint32_t argc, const Verb &V, uint32_t kl) { return 3ull + ndig(argc) + V.len + bulk_cost(kl); }
__device__ __forceinline__ void put_head(uint8_t *d, uint32_t argc, const Verb &V, const uint8_t *key, uint32_t kl) {
    uint8_t *body = d + 3 + ndig(argc) + V.len + 3 + ndig(kl);
    if (lane_id() == 0) {
        d = put_count(d, '*', argc);
        d = put_lit(d, V.text, V.len);
        put_count(d, '$', kl);
        put_crlf(body + kl);
    }
    wave_copy(body, key, kl);
}

// One value's commands: returns their size with status RR_OK (size pass), or writes them at out (EMIT,
// a value the size pass took).  Anything else: RR_E_ENCODE or RR_AOF_E_CPU, size 0.  expire -1: none.
template <bool EMIT>
__device__ uint64_t aof_value(const Batch &B, const Lds &Z, uint32_t type, uint32_t enc, uint32_t eb, uint32_t n,
                              const uint8_t *key, uint32_t kl, int64_t expire, uint8_t *out, uint32_t &status, uint64_t &pay) {
    const uint32_t lane = lane_id();
    constexpr uint32_t STR = 1u << RR_K_STR, INT = 1u << RR_K_INT, SCORE = 1u << RR_K_SCORE;
    uint32_t per = 1, first = 0, a0 = STR, a1 = 0;   // descriptors an item, the first item's descriptor, the kinds taken
    bool zs = false, cpu = false;                    // an item is member, score: written score first
    Verb V = {"$4\r\nSADD\r\n", 10};
    status = RR_E_ENCODE;
    switch (type) {
        case RR_TYPE_STRING:
            if (n != 1 || (enc != RR_ENC_RAW && enc != RR_ENC_INT && enc != RR_ENC_EMBSTR)) return 0;
            a0 = enc == RR_ENC_INT ? INT : STR;
            V = {"$3\r\nSET\r\n", 9};
            break;
        case RR_TYPE_LIST_QUICKLIST:
            a0 = STR | INT;
            V = {"$5\r\nRPUSH\r\n", 11};
            break;
        case RR_TYPE_SET_INTSET:
            if (enc != 2 && enc != 4 && enc != 8) return 0;
            a0 = INT;
            break;
        case RR_TYPE_SET_HT: break;
        case RR_TYPE_HASH_HT:
            per = 2;
            a1 = STR;
            V = {"$5\r\nHMSET\r\n", 11};
            break;
        case RR_TYPE_ZSET_SKIPLIST:
            per = 2;
            a1 = SCORE;
            zs = true;
            V = {"$4\r\nZADD\r\n", 10};
            break;
        case RR_TYPE_HASH_ZIPLIST:
        case RR_TYPE_ZSET_ZIPLIST: {
            if (n < 1) return 0;
            const ElemV z = get_elem(B.elems + eb);
            if (z.kind != RR_K_ZLRAW || !in_arena(z, B.arena_cap)) return 0;
            cpu = n == 1 && z.len != 11;             // the ZLRAW alone, and not the empty ziplist
            per = 2;
            first = 1;
            a0 = a1 = STR | INT;
            zs = type == RR_TYPE_ZSET_ZIPLIST;
            V = zs ? Verb{"$4\r\nZADD\r\n", 10} : Verb{"$5\r\nHMSET\r\n", 11};
            break;
        }
        default: return 0;
    }
    if ((n - first) % per) return 0;
    uint64_t pos = 0;
    const rr_elem *el = B.elems + eb + first;
    for (uint32_t left = (n - first) / per; left; left = left > RR_WAVE ? left - RR_WAVE : 0, el += per * RR_WAVE) {
        const uint32_t c = left < RR_WAVE ? left : RR_WAVE;
        const bool active = lane < c;
        ElemV e0 = {0, 0, 0}, e1 = {0, 0, 0};
        bool ok = true;
        if (active) {
            e0 = get_elem(el + per * lane);
            ok = e0.kind < 4 && ((a0 >> e0.kind) & 1) && (e0.kind != RR_K_STR || in_arena(e0, B.arena_cap));
            if (per == 2) {
                e1 = get_elem(el + 2 * lane + 1);
                ok = ok && e1.kind < 4 && ((a1 >> e1.kind) & 1) && (e1.kind != RR_K_STR || in_arena(e1, B.arena_cap));
            }
            if (type == RR_TYPE_SET_INTSET && enc != 8) {
                const int64_t iv = (int64_t)e0.data, lim = 1ll << (8 * enc - 1);
                ok = ok && iv >= -lim && iv < lim;
            }
        }
        if (__ballot(active && !ok)) {
            status = RR_E_ENCODE;
            return 0;
        }
        if (cpu) continue;                           // only the kinds of the rest are looked at
        Bulk b0 = {B_NONE, 0, 0}, b1 = {B_NONE, 0, 0};
        if (active) {
            if (zs) {
                // zzlGetScore (t_zset.c:721-741): strtod of a string entry, (double) of an integer one
                uint64_t bits = e1.data;
                bool have = true;
                if (e1.kind == RR_K_INT) {
                    const int64_t iv = (int64_t)e1.data;
                    bits = rr_s2d_from_u64(iv < 0, iv < 0 ? 0ull - (uint64_t)iv : (uint64_t)iv, Z.big);
                } else if (e1.kind == RR_K_STR) {
                    have = e1.len <= RR_AOF_SCORE_TEXT_MAX && rr_s2d_parse(B.arena + e1.data, e1.len, &bits, Z.big);
                }
                if ((bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) have = false;   // NaN
                if (have) b0 = {B_TEXT, (uint32_t)rr_d2s_print(Z.txt, bits, Z.big), 0};
                ok = have;
                b1 = bulk_of(e0);
            } else {
                b0 = bulk_of(e0);
                if (per == 2) b1 = bulk_of(e1);
            }
        }
        if (__ballot(active && !ok)) {
            cpu = true;
            continue;
        }
        const uint64_t cost = cost_of(b0) + cost_of(b1);
        const uint64_t incl = scan_costs(cost);
        const uint32_t argc = 2 + c * per;
        const uint64_t head = head_cost(argc, V, kl);
        if (EMIT) {
            put_head(out + pos, argc, V, key, kl);
            uint8_t *body0 = nullptr, *body1 = nullptr;
            if (active) {
                uint8_t *d = out + pos + head + incl - cost;
                d = put_bulk(d, b0, Z, body0);
                put_bulk(d, b1, Z, body1);
                pay += (b0.kind == B_BYTES ? b0.len : 0) + (b1.kind == B_BYTES ? b1.len : 0);
            }
            copy_bodies(body0, B.arena + b0.data, b0.len, body0 != nullptr);
            copy_bodies(body1, B.arena + b1.data, b1.len, body1 != nullptr);
        }
        pos += head + rl64(incl, RR_WAVE - 1);
    }
    if (cpu) {
        status = RR_AOF_E_CPU;
        return 0;
    }
    if (expire != -1) {                              // aof.c:1365-1370
        const Verb P = {"$9\r\nPEXPIREAT\r\n", 15};
        const uint64_t head = head_cost(3, P, kl);
        const uint32_t tl = dec_len(expire);
        if (EMIT) {
            put_head(out + pos, 3, P, key, kl);
            if (lane == 0) {
                uint8_t *d = put_count(out + pos + head, '$', tl);
                dec_write(d, expire);
                put_crlf(d + tl);
            }
        }
        pos += head + bulk_cost(tl);
    }
    status = RR_OK;
    return pos;
}

__device__ __forceinline__ Lds wave_lds() {
    __shared__ __attribute__((aligned(16))) uint8_t lds[WPB * WAVE_LDS];
    lds_u8 *b = (lds_u8 *)lds + (threadIdx.x / RR_WAVE) * WAVE_LDS;
    return {(lds_u32 *)b + lane_id(), b + BIG_LDS + SLOT * lane_id()};
}

// sizes into offsets[0, n), offsets[n] = 0; status; and the stage's zeroing
__global__ __launch_bounds__(WPB * RR_WAVE) void aof_size_kernel(const rr_value *__restrict__ values, uint64_t n, Batch B,
                                                                 const uint64_t *__restrict__ key_offs, uint64_t key_cap,
                                                                 const int64_t *__restrict__ expires, uint64_t *__restrict__ offsets,
                                                                 uint8_t *__restrict__ status, uint64_t *__restrict__ zero,
                                                                 uint64_t nzero, rr_totals *totals) {
    const Lds Z = wave_lds();
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    zero_stage_words(gtid, nthreads, zero, nzero, &offsets[n], totals);
    const uint64_t nwaves = nthreads / RR_WAVE;
    uint64_t pay = 0;
    for (uint64_t v = first64(gtid / RR_WAVE); v < n; v += nwaves) {
        const uint4 x = *reinterpret_cast<const uint4 *>(values + v);
        const uint32_t type = rfl(x.x & 0xFF), enc = rfl((x.x >> 8) & 0xFF);
        uint64_t size = 0;
        uint32_t st = RR_E_ENCODE;
        if (value_ok(x, B.elem_cap)) {
            const uint64_t k0 = first64(key_offs[v]), k1 = first64(key_offs[v + 1]);
            const bool kok = slice_ok(k0, k1, key_cap);
            const int64_t ex = expires ? (int64_t)first64((uint64_t)expires[v]) : -1;
            size = aof_value<false>(B, Z, type, enc, rfl(x.w), rfl(x.z), nullptr, kok ? (uint32_t)(k1 - k0) : 0u, ex, nullptr, st, pay);
            if (st != RR_E_ENCODE && !kok) {
                st = RR_RDBFILE_E_KEY;
                size = 0;
            }
        }
        if (lane_id() == 0) {
            offsets[v] = size;
            status[v] = (uint8_t)st;
        }
    }
}

// offsets scanned.  Writes the commands of the values that fit data_cap; RR_E_CAPACITY for those that
// do not; the totals.
__global__ __launch_bounds__(WPB * RR_WAVE) void aof_emit_kernel(const rr_value *__restrict__ values, uint64_t n, Batch B,
                                                                 const uint8_t *__restrict__ keys,
                                                                 const uint64_t *__restrict__ key_offs,
                                                                 const int64_t *__restrict__ expires,
                                                                 const uint64_t *__restrict__ offsets, uint8_t *out,
                                                                 uint64_t data_cap, uint8_t *status, const uint64_t *err,
                                                                 rr_totals *totals) {
    const Lds Z = wave_lds();
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = nthreads / RR_WAVE;
    if (gtid == 0) totals->bytes = *err ? ~0ull : offsets[n];
    uint64_t pay = 0, n_bad = 0, n_el = 0;   // pay a lane's, the others wave-uniform
    for (uint64_t v = first64(gtid / RR_WAVE); v < n; v += nwaves) {
        const uint4 x = *reinterpret_cast<const uint4 *>(values + v);
        const uint32_t type = rfl(x.x & 0xFF), enc = rfl((x.x >> 8) & 0xFF);
        n_el += rfl(x.z);
        uint32_t st = rfl(status[v]);
        if (st) { ++n_bad; continue; }
        const uint64_t o0 = first64(offsets[v]), o1 = first64(offsets[v + 1]);
        if (o1 > data_cap) {
            ++n_bad;
            if (lane_id() == 0) status[v] = RR_E_CAPACITY;
            continue;
        }
        if (o1 == o0) continue;              // an empty aggregate without an expiry
        const uint64_t k0 = first64(key_offs[v]), k1 = first64(key_offs[v + 1]);
        const int64_t ex = expires ? (int64_t)first64((uint64_t)expires[v]) : -1;
        aof_value<true>(B, Z, type, enc, rfl(x.w), rfl(x.z), keys + k0, (uint32_t)(k1 - k0), ex, out + o0, st, pay);
    }
    add_totals(totals, sum_lanes(pay), n_el, n_bad);
}

}  // namespace

// scratch: the scan's look-back words, the error word
extern "C" uint64_t rr_aof_scratch_words(uint64_t n) { return rr_scan_words(n) + 1; }

extern "C" hipError_t rr_launch_aof(const rr_value *values, const rr_elem *elems, uint64_t elem_cap, const uint8_t *arena,
                                    uint64_t arena_cap, uint64_t n, const uint8_t *keys, const uint64_t *key_offs, uint64_t key_cap,
                                    const int64_t *expires, uint8_t *out, uint64_t cap, uint64_t *offsets, uint8_t *status,
                                    uint64_t *scratch, rr_totals *totals, hipStream_t stream) {
    const uint64_t lbw = rr_scan_words(n);
    uint64_t *lb = scratch, *err = scratch + lbw;
    const Batch B = {elems, elem_cap, arena, arena_cap};
    const uint32_t grid = capped_grid(n, WPB, GRID_CAP);
    hipLaunchKernelGGL(aof_size_kernel, dim3(grid), dim3(WPB * RR_WAVE), 0, stream, values, n, B, key_offs, key_cap, expires,
                       offsets, status, lb, lbw + 1, totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(offsets, n, lb, err, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(aof_emit_kernel, dim3(grid), dim3(WPB * RR_WAVE), 0, stream, values, n, B, keys, key_offs, expires,
                       (const uint64_t *)offsets, out, cap, status, (const uint64_t *)err, totals);
    return hipGetLastError();
}
