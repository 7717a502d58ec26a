// rr_rdbzset.hip — gfx950 kernels of include/rr_d2string.h and include/rr_rdbzset.h: d2string with an
// exact %.17g, and the small ZSets rr_rdbconvert_batch left because a score needs it.
//
// The printer is rr_d2string_impl.h, the host's statements, a lane a score.  Its multi-word state (34
// words a score) is not a private array, which a loop's index would send to scratch: every wave has
// 34 x 64 words of LDS, lane l's word k at [64 k + l], so a lane's words all lie in bank l mod 32 and
// lanes at different k never collide; the text goes to a 32-byte LDS slot per lane (the length in its
// last byte).  d2string_kernel prints 64 scores a wave and copies the slots' written bytes out, 64
// consecutive bytes an instruction.
//
// The stage is rr_stage_device.h's with its attempted list in front, as rr_rdbconvert.hip's.  Reading
// the payload and the rank sort are rr_rdbconvert_device.h's.  Then, 64 ranks at a time, the lanes print the 64 scores into the slots
// and the wave pushes member, text, member, text ... from them: the text through string2ll like any
// string (zipTryEncoding), so "17" and "4503599627370496" are integer entries and "1.5" is not.
//
// A wave's LDS is the sort arrays (9216) + window (64) + state (8704) + slots (2048) = 20032 bytes:
// two waves a workgroup, four workgroups of the 160 KiB a CU, two waves a SIMD.
#include <hip/hip_runtime.h>

#include "rr_rdbconvert_device.h"
#include "rr_kernels.h"
#include "../../include/rr_d2string.h"
#include "../../include/rr_rdbzset.h"

#define RR_D2S_FN __device__ __forceinline__
#define RR_D2S_WORD rr::lds_u32
#define RR_D2S_STRIDE RR_WAVE
#define RR_D2S_CHAR rr::lds_u8
#include "rr_d2string_impl.h"

using namespace rr;

namespace {

constexpr uint32_t SLOT = RR_D2STRING_SLOT;                    // a text's LDS slot: the text, its length in the last byte
constexpr uint32_t BIG_LDS = 4 * RR_D2S_WORDS * RR_WAVE;       // the wave's multi-word states
constexpr uint32_t TXT_LDS = SLOT * RR_WAVE;
static_assert(RR_D2STRING_MAX < SLOT, "the length byte");

// ---- rr_d2string_batch ---------------------------------------------------------------------------------
constexpr uint32_t D2S_WPB = 4;
constexpr uint32_t D2S_WAVE_LDS = BIG_LDS + TXT_LDS;

__global__ __launch_bounds__(D2S_WPB * RR_WAVE) void d2string_kernel(const uint64_t *__restrict__ bits, uint64_t n,
                                                                     uint8_t *__restrict__ text, uint8_t *__restrict__ len) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[D2S_WPB * D2S_WAVE_LDS];
    const uint32_t lane = lane_id();
    lds_u8 *b = (lds_u8 *)lds + (threadIdx.x / RR_WAVE) * D2S_WAVE_LDS;
    lds_u32 *big = (lds_u32 *)b + lane;
    lds_u8 *txt = b + BIG_LDS;
    const uint64_t nwaves = (uint64_t)gridDim.x * D2S_WPB;
    for (uint64_t base = ((uint64_t)blockIdx.x * D2S_WPB + threadIdx.x / RR_WAVE) * RR_WAVE; base < n; base += nwaves * RR_WAVE) {
        const uint64_t i = base + lane;
        uint32_t l = 0;
        if (i < n) {
            l = (uint32_t)rr_d2s_print(txt + SLOT * lane, bits[i], big);
            len[i] = (uint8_t)l;
        }
        txt[SLOT * lane + SLOT - 1] = (uint8_t)l;
        wave_sync();
        const uint64_t left = n - base;                        // slots of this round that exist
        for (uint32_t k = lane; k < TXT_LDS; k += RR_WAVE) {
            const uint32_t slot = k / SLOT, at = k % SLOT;
            if (slot < left && at < txt[SLOT * slot + SLOT - 1]) text[(base + slot) * SLOT + at] = txt[k];
        }
        wave_sync();   // the next round's texts go over these
    }
}

// ---- rr_rdbzset_batch ----------------------------------------------------------------------------------
constexpr uint32_t WPB = 2;                                    // waves (values in flight) per workgroup
constexpr uint32_t GRID_CAP = RR_RDBCONVERT_MAX_WAVES / WPB;
// a wave's LDS: the sort arrays | window | states | slots.  str_is_ll looks at 64 bytes from a slot's
// start, so the last slots' look ends in what follows: the next wave's arrays, or the pad
constexpr uint32_t WAVE_LDS = SORT_LDS + PEEK + BIG_LDS + TXT_LDS;
static_assert(WPB * WAVE_LDS + RR_WAVE <= 65536 && WAVE_LDS % 8 == 0 && (SORT_LDS + PEEK) % 4 == 0, "static LDS");

struct ZLds {
    Lds s;
    lds_u32 *big;   // this lane's state
    lds_u8 *txt;
};
__device__ __forceinline__ ZLds wave_lds() {
    __shared__ __attribute__((aligned(16))) uint8_t lds[WPB * WAVE_LDS + RR_WAVE];
    lds_u8 *b = (lds_u8 *)lds + (threadIdx.x / RR_WAVE) * WAVE_LDS;
    return {sort_lds(b), (lds_u32 *)(b + SORT_LDS + PEEK) + lane_id(), b + SORT_LDS + PEEK + BIG_LDS};
}

// One ZSet_2 payload as a ZSET_ZIPLIST blob: returns its size with status RR_OK (size pass), or writes
// it at out (EMIT, a value the size pass converted).  Anything else: RR_RDBLOAD_E_CONVERT, size 0.
template <bool EMIT>
__device__ uint64_t zset_value(Rd &r, const Opt &O, const ZLds &Z, uint8_t *out, uint32_t &status, uint64_t &pay, uint64_t &nel) {
    const uint32_t lane = lane_id();
    const Lds &W = Z.s;
    status = RR_RDBLOAD_E_CONVERT;
    if (r.p >= r.n) return 0;
    const uint32_t hv = ld8(r.R, r.p + lane);
    bool ie;
    uint64_t n;
    uint32_t used;
    if (parse_len(hv, 0, r.n - r.p, ie, n, used)) return 0;   // a count site
    r.p += used;
    if (n > O.zset_e || n > MAXN) return 0;                    // rdb.c:1517-1555
    const uint32_t cnt_in = (uint32_t)n;
    if (!zset_read<!EMIT, true>(r, cnt_in, O, W)) return 0;
    zset_rank_sort(r.R, W, cnt_in);
    Zl z = {10, 0, 10};
    uint8_t *zb = out + 13;
    for (uint32_t base = 0; base < cnt_in; base += RR_WAVE) {
        const uint32_t m = cnt_in - base < RR_WAVE ? cnt_in - base : RR_WAVE;
        if (lane < m) {                                        // d2string of the scores at ranks base .. base + m, a lane each
            const uint32_t l = (uint32_t)rr_d2s_print(Z.txt + SLOT * lane, W.key[W.ord[base + lane]], Z.big);
            Z.txt[SLOT * lane + SLOT - 1] = (uint8_t)l;
        }
        wave_sync();
        for (uint32_t j = 0; j < m; ++j) {                     // zsetConvert :1221-1230, zzlInsertAt :1035-1038
            const Str s = zset_member(W, rfl(W.ord[base + j]));
            zl_push<EMIT>(r, s, z, zb, W.win);
            lds_u8 *t = Z.txt + SLOT * j;
            const uint32_t tl = rfl(t[SLOT - 1]);
            int64_t iv;
            if (tl <= 20 && str_is_ll(r, Src{true, 0}, tl, t, iv)) zl_push_int<EMIT>(z, zb, iv);
            else {
                const uint64_t d = zl_str_hdr<EMIT>(z, zb, tl);
                if (EMIT && lane < tl) zb[d + lane] = t[lane];
                zl_advance(z, d + tl);
            }
        }
        wave_sync();   // the next round's texts, or the next value's keys, go over these
    }
    const uint64_t total = z.pos + 1;
    if (total >= MAX_SLICE) return 0;
    if (EMIT && lane == 0) {
        out[0] = RR_TYPE_ZSET_ZIPLIST;
        put_le(out + 1, O.lru, 4);
        put_le(out + 5, total, 8);
        put_le(zb, total, 4);
        put_le(zb + 4, z.last, 4);
        put_le(zb + 8, 2 * cnt_in, 2);
        zb[z.pos] = 0xFF;
    }
    pay += total;
    nel += cnt_in;
    status = RR_OK;
    return 13 + total;
}

// attempted: the ZSet_2 values rr_rdbconvert_batch left with E_CONVERT
struct ZsetAttempted {
    const uint8_t *__restrict__ types, *__restrict__ convert_status;
    __device__ __forceinline__ bool operator()(uint64_t i) const {
        return convert_status[i] == RR_RDBLOAD_E_CONVERT && types[i] == RR_TYPE_ZSET_SKIPLIST;
    }
};

// blob sizes into out_offs[] and status of the list's values (att[n] of them)
__global__ __launch_bounds__(WPB * RR_WAVE) void rdbzset_size_kernel(const uint8_t *__restrict__ data, uint64_t in_cap,
                                                                     const uint64_t *__restrict__ in_offs, uint64_t n,
                                                                     const uint32_t *__restrict__ list, const uint64_t *__restrict__ att,
                                                                     Opt O, uint64_t *__restrict__ out_offs, uint8_t *__restrict__ status) {
    const ZLds Z = wave_lds();
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = (uint64_t)gridDim.x * blockDim.x / RR_WAVE;
    const uint64_t m = first64(att[n]);
    for (uint64_t k = first64(gtid / RR_WAVE); k < m; k += nwaves) {
        const uint64_t v = rfl(list[k]);
        const uint64_t o0 = first64(in_offs[v]), o1 = first64(in_offs[v + 1]);
        uint32_t st = RR_RDBLOAD_E_CONVERT;
        uint64_t size = 0, pay = 0, nel = 0;
        if (slice_ok(o0, o1, in_cap)) {
            Rd r = rd_of(data, o0, o1);
            size = zset_value<false>(r, O, Z, nullptr, st, pay, nel);
        }
        if (lane_id() == 0 && st == RR_OK) {
            out_offs[v] = size;
            status[v] = RR_OK;
        }
    }
}

// out_offs scanned.  Writes the blobs of the converted values that fit out_cap; RR_E_CAPACITY for
// those that do not; the totals.
__global__ __launch_bounds__(WPB * RR_WAVE) void rdbzset_emit_kernel(const uint8_t *__restrict__ data,
                                                                     const uint64_t *__restrict__ in_offs, uint64_t n,
                                                                     const uint32_t *__restrict__ list, const uint64_t *__restrict__ att,
                                                                     Opt O, const uint64_t *__restrict__ out_offs, uint8_t *out,
                                                                     uint64_t out_cap, uint8_t *status, const uint64_t *err1,
                                                                     const uint64_t *err2, rr_totals *totals) {
    const ZLds Z = wave_lds();
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = (uint64_t)gridDim.x * blockDim.x / RR_WAVE;
    if (gtid == 0) totals->bytes = (*err1 | *err2) ? ~0ull : out_offs[n];
    const uint64_t m = first64(att[n]);
    uint64_t pay = 0, nel = 0, n_bad = 0;   // wave-uniform
    for (uint64_t k = first64(gtid / RR_WAVE); k < m; k += nwaves) {
        const uint64_t v = rfl(list[k]);
        uint32_t st = rfl(status[v]);
        if (st) { ++n_bad; continue; }
        const uint64_t b0 = first64(out_offs[v]), b1 = first64(out_offs[v + 1]);
        if (b1 > out_cap) {
            ++n_bad;
            if (lane_id() == 0) status[v] = RR_E_CAPACITY;
            continue;
        }
        const uint64_t o0 = first64(in_offs[v]), o1 = first64(in_offs[v + 1]);
        Rd r = rd_of(data, o0, o1);
        zset_value<true>(r, O, Z, out + b0, st, pay, nel);
    }
    add_totals(totals, pay, nel, n_bad);
}

}  // namespace

extern "C" hipError_t rr_launch_d2string(const uint64_t *bits, uint64_t n, uint8_t *text, uint8_t *len, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t b = (n + D2S_WPB * RR_WAVE - 1) / (D2S_WPB * RR_WAVE);
    hipLaunchKernelGGL(d2string_kernel, dim3((uint32_t)(b < 16384 ? b : 16384)), dim3(D2S_WPB * RR_WAVE), 0, stream, bits, n, text, len);
    return hipGetLastError();
}

extern "C" uint64_t rr_rdbzset_scratch_words(uint64_t n) { return AttScratch::words(n); }

extern "C" hipError_t rr_launch_rdbzset(const uint8_t *data, uint64_t in_cap, const uint64_t *in_offs, const uint8_t *types,
                                        const uint8_t *convert_status, uint64_t n, const uint32_t *opt6, uint8_t *out,
                                        uint64_t out_cap, uint64_t *out_offs, uint8_t *status, uint64_t *scratch, rr_totals *totals,
                                        hipStream_t stream) {
    const AttScratch S(scratch, n);
    const Opt O = opt_of(opt6);
    const uint32_t grid = capped_grid(n, WPB, GRID_CAP);   // a wave a value
    hipError_t e = launch_attempted(ZsetAttempted{types, convert_status}, n, S, out_offs, nullptr, status, RR_RDBLOAD_E_CONVERT,
                                    RR_RDBZSET_SKIP, totals, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rdbzset_size_kernel, dim3(grid), dim3(WPB * RR_WAVE), 0, stream, data, in_cap, in_offs, n,
                       (const uint32_t *)S.list, (const uint64_t *)S.att, O, out_offs, status);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(out_offs, n, S.lb2, S.err2, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rdbzset_emit_kernel, dim3(grid), dim3(WPB * RR_WAVE), 0, stream, data, in_offs, n,
                       (const uint32_t *)S.list, (const uint64_t *)S.att, O, (const uint64_t *)out_offs, out, out_cap, status,
                       (const uint64_t *)S.err1, (const uint64_t *)S.err2, totals);
    return hipGetLastError();
}
