// rr_rdbconvert.hip — gfx950 kernels of include/rr_rdbconvert.h: the values rr_rdbload_batch left
// with RR_RDBLOAD_E_CONVERT, in the encoding rdbLoadObject picks for them (rdb.c:1476-1600): a Set of
// integers as an intset, a small Hash and a small ZSet as ziplists.  The stage is rr_stage_device.h's
// with its attempted list in front (flags, scan, compaction, then size, scan, emit over the list):
// rdbconvert_size_kernel takes every decision, rdbconvert_emit_kernel writes the bytes; at most
// RR_RDBCONVERT_MAX_WAVES waves a launch.
//
// The walk is rr_rdbload.hip's (rr_rdbload_device.h): wave-uniform, every load of payload
// bytes in the size pass through a buffer resource over exactly the value's slice, so a value that
// is not what its load_status claims reads zeros, never a neighbour, and ends as E_CONVERT.
//
// Sorting is a rank sort in the wave's LDS: element i goes to the slot that is the number of
// elements before it in the order (ties by index, so the ranks are a permutation); a lane an
// element, every lane reading the same other element at a time (an LDS broadcast).  n is at most
// RR_RDBCONVERT_MAX_N, so that is 8 elements a lane and n reads each.  A Set sorts its int64 values
// and drops the duplicates behind it; a ZSet sorts (score, member) with a table of member offsets
// and lengths, the member bytes compared in the payload when scores tie.  Both passes sort: the size
// pass needs the intset's length and width and the ziplist's prevlen chain, and a permutation kept in
// scratch for the emit pass would cost what the second sort costs.
#include <hip/hip_runtime.h>

#include "rr_rdbconvert_device.h"
#include "rr_kernels.h"

using namespace rr;

namespace {

constexpr uint32_t WPB = 4;                            // waves (values in flight) per workgroup
constexpr uint32_t GRID_CAP = RR_RDBCONVERT_MAX_WAVES / WPB;   // workgroups
// a wave's LDS: the sort arrays | window (rr_rdbconvert_device.h)
constexpr uint32_t WAVE_LDS = SORT_LDS + PEEK;
static_assert(WPB * WAVE_LDS <= 65536 && WAVE_LDS % 8 == 0, "static LDS");
static_assert(RR_RDBCONVERT_MAX_WAVES % WPB == 0, "whole workgroups");

__device__ __forceinline__ Lds wave_lds() {
    __shared__ __attribute__((aligned(16))) uint8_t lds[WPB * WAVE_LDS];
    return sort_lds((lds_u8 *)lds + (threadIdx.x / RR_WAVE) * WAVE_LDS);
}

// ---- one value -------------------------------------------------------------------------------------
// Returns the blob's size, with status RR_OK and the new type (size pass), or writes the blob at out
// (EMIT, a value the size pass converted).  Anything else: status RR_RDBLOAD_E_CONVERT, size 0.
// pay / nel: rr_totals.payload and n_elems of this value, added.
template <bool EMIT>
__device__ uint64_t convert_value(Rd &r, uint32_t type, const Opt &O, const Lds &W, uint8_t *out, uint32_t &status, uint32_t &otype,
                                  uint64_t &pay, uint64_t &nel) {
    const uint32_t lane = lane_id();
    status = RR_RDBLOAD_E_CONVERT;
    otype = 0;
    if (type != RR_TYPE_SET_HT && type != RR_TYPE_HASH_HT && type != RR_TYPE_ZSET_SKIPLIST) return 0;
    if (r.p >= r.n) return 0;
    const uint32_t hv = ld8(r.R, r.p + lane);
    bool ie;
    uint64_t n;
    uint32_t used;
    if (parse_len(hv, 0, r.n - r.p, ie, n, used)) return 0;   // a count site
    r.p += used;
    Str s;
    uint64_t size;
    if (type == RR_TYPE_SET_HT) {                              // rdb.c:1481-1506
        if (n > O.set_ie || n > MAXN) return 0;
        const uint32_t cnt_in = (uint32_t)n;
        for (uint32_t k = 0; k < cnt_in; ++k) {
            if (rd_string<!EMIT>(r, s)) return 0;
            int64_t v = s.iv;
            if (s.kind != S_INT && !(s.len >= 1 && s.len <= 20 && str_is_ll(r, materialize(r, s, 20, W.win), s.len, W.win, v)))
                return 0;                                      // isSdsRepresentableAsLongLong :1501
            if (lane == 0) W.key[k] = (uint64_t)v;
        }
        if (r.p != r.n) return 0;
        wave_sync();
        for (uint32_t i = lane; i < cnt_in; i += RR_WAVE) {    // intsetSearch's slot for every value at once
            const int64_t ki = (int64_t)W.key[i];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < cnt_in; ++j) {
                const int64_t kj = (int64_t)W.key[j];
                rank += (kj < ki || (kj == ki && j < i)) ? 1u : 0u;
            }
            W.sorted[rank] = (uint64_t)ki;
        }
        wave_sync();
        uint32_t enc = 2;                                      // intsetNew; _intsetValueEncoding of the extremes
        if (cnt_in) {
            const int64_t lo = (int64_t)first64(W.sorted[0]), hi = (int64_t)first64(W.sorted[cnt_in - 1]);
            enc = (lo < -2147483648ll || hi > 2147483647ll) ? 8u : (lo < -32768 || hi > 32767) ? 4u : 2u;
        }
        uint32_t cnt = 0;
        for (uint32_t b = 0; b < cnt_in; b += RR_WAVE) {       // a value already there is dropped (intset.c:219)
            const uint32_t k = b + lane;
            const bool in = k < cnt_in;
            const uint64_t vk = in ? W.sorted[k] : 0;
            const bool uniq = in && (k == 0 || W.sorted[k - 1] != vk);
            const uint64_t m = __ballot(uniq);
            if (EMIT && uniq) put_le(out + 13 + (uint64_t)(cnt + __popcll(m & ((1ull << lane) - 1))) * enc, vk, enc);
            cnt += (uint32_t)__popcll(m);
        }
        if (EMIT && lane == 0) {
            put_le(out + 5, enc, 4);
            put_le(out + 9, cnt, 4);
        }
        otype = RR_TYPE_SET_INTSET;
        size = 13 + (uint64_t)enc * cnt;
        pay += 8 + (uint64_t)enc * cnt;
        nel += cnt_in;
        wave_sync();   // the next value's keys go over these
    } else {
        Zl z = {10, 0, 10};
        uint8_t *zb = out + 13;
        uint32_t entries;
        if (type == RR_TYPE_HASH_HT) {                         // rdb.c:1567-1596
            if (n > O.hash_e) return 0;
            entries = 2 * (uint32_t)n;
            for (uint32_t k = 0; k < entries; ++k) {
                if (rd_string<!EMIT>(r, s)) return 0;
                if (s.len > O.hash_v) return 0;                // :1586
                zl_push<EMIT>(r, s, z, zb, W.win);
            }
            if (r.p != r.n) return 0;
            nel += entries;
            otype = RR_TYPE_HASH_ZIPLIST;
        } else {                                               // rdb.c:1517-1555
            if (n > O.zset_e || n > MAXN) return 0;
            const uint32_t cnt_in = (uint32_t)n;
            entries = 2 * cnt_in;
            if (!zset_read<!EMIT, false>(r, cnt_in, O, W)) return 0;
            zset_rank_sort(r.R, W, cnt_in);
            for (uint32_t k = 0; k < cnt_in; ++k) {                // zsetConvert :1221-1230, zzlInsertAt :1035-1038
                const uint32_t i = rfl(W.ord[k]);
                const uint64_t bits = first64(W.key[i]);
                s = zset_member(W, i);
                zl_push<EMIT>(r, s, z, zb, W.win);
                int64_t iv;
                const uint32_t cls = score_class(bits, iv);
                if (cls == SC_INT) zl_push_int<EMIT>(z, zb, iv);
                else {
                    const uint32_t tl = cls == SC_INF ? 3u : cls == SC_NINF ? 4u : 2u;
                    const uint64_t d = zl_str_hdr<EMIT>(z, zb, tl);
                    if (EMIT && lane == 0) {
                        uint8_t *t = zb + d;
                        if (cls == SC_NZERO) { t[0] = '-'; t[1] = '0'; }
                        else {
                            if (cls == SC_NINF) *t++ = '-';
                            t[0] = 'i'; t[1] = 'n'; t[2] = 'f';
                        }
                    }
                    zl_advance(z, d + tl);
                }
            }
            nel += cnt_in;
            otype = RR_TYPE_ZSET_ZIPLIST;
            wave_sync();
        }
        const uint64_t total = z.pos + 1;
        if (total >= MAX_SLICE) { otype = 0; return 0; }
        if (EMIT && lane == 0) {
            put_le(out + 5, total, 8);
            put_le(zb, total, 4);
            put_le(zb + 4, z.last, 4);
            put_le(zb + 8, entries, 2);
            zb[z.pos] = 0xFF;
        }
        pay += total;
        size = 13 + total;
    }
    if (EMIT && lane == 0) {
        out[0] = (uint8_t)otype;
        put_le(out + 1, O.lru, 4);
    }
    status = RR_OK;
    return size;
}

// attempted: what rr_rdbload_batch left with E_CONVERT
struct ConvertAttempted {
    const uint8_t *__restrict__ load_status;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return load_status[i] == RR_RDBLOAD_E_CONVERT; }
};

// blob sizes into out_offs[], status and out_types of the list's values (att[n] of them)
__global__ __launch_bounds__(WPB * RR_WAVE) void rdbconvert_size_kernel(const uint8_t *__restrict__ data, uint64_t in_cap,
                                                                        const uint64_t *__restrict__ in_offs,
                                                                        const uint8_t *__restrict__ types, uint64_t n,
                                                                        const uint32_t *__restrict__ list,
                                                                        const uint64_t *__restrict__ att, Opt O,
                                                                        uint64_t *__restrict__ out_offs, uint8_t *__restrict__ out_types,
                                                                        uint8_t *__restrict__ status) {
    const Lds W = wave_lds();
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = (uint64_t)gridDim.x * blockDim.x / RR_WAVE;
    const uint64_t m = first64(att[n]);
    for (uint64_t k = first64(gtid / RR_WAVE); k < m; k += nwaves) {
        const uint64_t v = rfl(list[k]);
        const uint32_t type = rfl(types[v]);
        const uint64_t o0 = first64(in_offs[v]), o1 = first64(in_offs[v + 1]);
        uint32_t st = RR_RDBLOAD_E_CONVERT, ot = 0;
        uint64_t size = 0, pay = 0, nel = 0;
        // (slice_ok and rd_of written out: through the helpers this kernel's walk is scheduled differently, 76 bytes longer)
        if (o0 <= o1 && o1 <= in_cap && o1 - o0 < MAX_SLICE) {
            Rd r = {mk_rsrc(data + o0, (uint32_t)(o1 - o0)), data + o0, (uint32_t)(o1 - o0), 0};
            size = convert_value<false>(r, type, O, W, nullptr, st, ot, pay, nel);
        }
        if (lane_id() == 0 && st == RR_OK) {
            out_offs[v] = size;
            out_types[v] = (uint8_t)ot;
            status[v] = RR_OK;
        }
    }
}

// out_offs scanned.  Writes the blobs of the converted values that fit out_cap; RR_E_CAPACITY for
// those that do not; the totals.
__global__ __launch_bounds__(WPB * RR_WAVE) void rdbconvert_emit_kernel(const uint8_t *__restrict__ data,
                                                                        const uint64_t *__restrict__ in_offs,
                                                                        const uint8_t *__restrict__ types, uint64_t n,
                                                                        const uint32_t *__restrict__ list,
                                                                        const uint64_t *__restrict__ att, Opt O,
                                                                        const uint64_t *__restrict__ out_offs, uint8_t *out,
                                                                        uint64_t out_cap, uint8_t *status, const uint64_t *err1,
                                                                        const uint64_t *err2, rr_totals *totals) {
    const Lds W = wave_lds();
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = (uint64_t)gridDim.x * blockDim.x / RR_WAVE;
    if (gtid == 0) totals->bytes = (*err1 | *err2) ? ~0ull : out_offs[n];
    const uint64_t m = first64(att[n]);
    uint64_t pay = 0, nel = 0, n_bad = 0;   // wave-uniform
    for (uint64_t k = first64(gtid / RR_WAVE); k < m; k += nwaves) {
        const uint64_t v = rfl(list[k]);
        uint32_t st = rfl(status[v]), ot;
        if (st) { ++n_bad; continue; }
        const uint64_t b0 = first64(out_offs[v]), b1 = first64(out_offs[v + 1]);
        if (b1 > out_cap) {
            ++n_bad;
            if (lane_id() == 0) status[v] = RR_E_CAPACITY;
            continue;
        }
        const uint32_t type = rfl(types[v]);
        const uint64_t o0 = first64(in_offs[v]), o1 = first64(in_offs[v + 1]);
        Rd r = rd_of(data, o0, o1);
        convert_value<true>(r, type, O, W, out + b0, st, ot, pay, nel);
    }
    add_totals(totals, pay, nel, n_bad);
}

}  // namespace

extern "C" uint64_t rr_rdbconvert_scratch_words(uint64_t n) { return AttScratch::words(n); }

extern "C" hipError_t rr_launch_rdbconvert(const uint8_t *data, uint64_t in_cap, const uint64_t *in_offs, const uint8_t *types,
                                           const uint8_t *load_status, uint64_t n, const uint32_t *opt6, uint8_t *out,
                                           uint64_t out_cap, uint64_t *out_offs, uint8_t *out_types, uint8_t *status,
                                           uint64_t *scratch, rr_totals *totals, hipStream_t stream) {
    const AttScratch S(scratch, n);
    const Opt O = opt_of(opt6);
    const uint32_t grid = capped_grid(n, WPB, GRID_CAP);   // a wave a value
    hipError_t e = launch_attempted(ConvertAttempted{load_status}, n, S, out_offs, out_types, status, RR_RDBLOAD_E_CONVERT,
                                    RR_RDBCONVERT_SKIP, totals, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rdbconvert_size_kernel, dim3(grid), dim3(WPB * RR_WAVE), 0, stream, data, in_cap, in_offs, types, n,
                       (const uint32_t *)S.list, (const uint64_t *)S.att, O, out_offs, out_types, status);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(out_offs, n, S.lb2, S.err2, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rdbconvert_emit_kernel, dim3(grid), dim3(WPB * RR_WAVE), 0, stream, data, in_offs, types, n,
                       (const uint32_t *)S.list, (const uint64_t *)S.att, O, (const uint64_t *)out_offs, out, out_cap, status,
                       (const uint64_t *)S.err1, (const uint64_t *)S.err2, totals);
    return hipGetLastError();
}
