// rr_rdbmerge.hip — gfx950 kernels of include/rr_rdbloadall.h: the blob batches of the three load
// stages gathered into one.
//
// The stage is rr_stage_device.h's: sizes, scan, emit.
//
//   merge_size_kernel   a thread a value (there is no walk): the selection rule from the three
//                       statuses, the holding stage's slice checked, the size into offs[v], the merged
//                       status and out_types, and where the bytes come from into src[v]
//                       (stage << 62 | the slice's start; 0: nothing to write).  Zeroes the scan's words.
//   merge_emit_kernel   a pure gather, partitioned by the OUTPUT: a wave owns SPAN bytes of out->data
//                       at a time (16-byte aligned, spans strided over a capped grid).  Row by row
//                       (64 lanes x 16 bytes) the wave finds the values that reach into the row by a
//                       64-ary search of the merged offsets (one load a step, the lanes probing 64
//                       places), each lane finds the value under its own 16 bytes by a binary search
//                       between the two, assembles its 16 bytes from the (unaligned) source segments
//                       and stores them aligned.  A value that crosses rows or spans is copied by every
//                       wave whose rows it touches, so a 1 GiB String costs no wave more than a short one.
//                       Its prologue, a thread a value, gives RR_E_CAPACITY to what ends past the
//                       capacity and sums the totals.
//
// A 16-byte piece that holds a byte which must stay as it was (of a value that is not written, or past
// the written end) is stored byte by byte; every other piece is one 16-byte store.  Source reads are 16
// bytes inside [data, data + data_cap) of the holding batch, shifted when the segment ends in the
// batch's last 15 bytes.
#include <hip/hip_runtime.h>

#include "rr_stage_device.h"
#include "../../include/rr_rdbloadall.h"

using namespace rr;

namespace {

constexpr uint32_t WPB = 4;                                   // waves a workgroup
constexpr uint32_t SPAN = RR_RDBMERGE_SPAN;                   // bytes of the output a wave owns at a time
constexpr uint32_t ROW = RR_WAVE * 16;                        // bytes a wave stores an instruction
constexpr uint32_t GRID_CAP = RR_RDBMERGE_MAX_WAVES / WPB;
constexpr uint64_t SRC_AT = (1ull << 62) - 1;                 // src[v]: stage << 62 | the slice's start
static_assert(SPAN % ROW == 0, "whole rows");

struct Stage {
    const uint8_t *__restrict__ data;
    const uint64_t *__restrict__ offs;
    const uint8_t *__restrict__ status;
    uint64_t cap;
};

__global__ __launch_bounds__(256) void merge_size_kernel(Stage A, Stage B, Stage C, const uint8_t *__restrict__ types,
                                                         const uint8_t *__restrict__ conv_types, uint64_t n,
                                                         uint64_t *__restrict__ offs, uint64_t *__restrict__ src,
                                                         uint8_t *__restrict__ out_types, uint8_t *__restrict__ status,
                                                         uint64_t *__restrict__ zero, uint64_t nzero, rr_totals *totals) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    zero_stage_words(gtid, nthreads, zero, nzero, &offs[n], totals);
    for (uint64_t i = gtid; i < n; i += nthreads) {
        uint32_t st = A.status[i], k = 0;
        const auto holds = [](uint32_t s) { return s == RR_OK || s == RR_E_CAPACITY; };
        if (holds(st)) k = 1;
        else if (st == RR_RDBLOAD_E_CONVERT) {
            const uint32_t s2 = B.status[i];
            if (holds(s2)) k = 2, st = s2;
            else if (s2 == RR_RDBLOAD_E_CONVERT) {
                const uint32_t s3 = C.status[i];
                if (holds(s3)) k = 3, st = s3;
            }
        }
        uint64_t size = 0, from = 0;
        uint32_t type = 0xFF;
        if (k) {
            const uint64_t *__restrict__ ho = k == 1 ? A.offs : k == 2 ? B.offs : C.offs;   // (fields, not a Stage: no private copy)
            const uint64_t hcap = k == 1 ? A.cap : k == 2 ? B.cap : C.cap;
            const uint64_t o0 = ho[i], o1 = ho[i + 1];
            if (o0 > o1 || (st == RR_OK && o1 > hcap)) st = RR_RDBMERGE_E_SLICE;
            else {
                size = o1 - o0;
                type = k == 1 ? types[i] : k == 2 ? conv_types[i] : (uint32_t)RR_TYPE_ZSET_ZIPLIST;
                if (st == RR_OK) from = ((uint64_t)k << 62) | o0;
            }
        }
        offs[i] = size;
        src[i] = from;
        status[i] = (uint8_t)st;
        if (out_types) out_types[i] = (uint8_t)type;
    }
}

// the first v in [lo, hi] with offs[v + 1] > t, by the whole wave (wave-uniform arguments; offs[hi + 1] > t):
// the lanes probe 64 places a step, the first step the 64 values at lo
__device__ __forceinline__ uint64_t wave_find(const uint64_t *__restrict__ offs, uint64_t lo, uint64_t hi, uint64_t t) {
    const uint32_t lane = lane_id();
    uint64_t step = 1;
    while (lo < hi) {
        const uint64_t p = lo + lane * step;
        const bool past = p >= hi || offs[p + 1] > t;          // p >= hi: true by the contract
        const uint64_t b = __ballot(past);
        if (b == 0) lo += 63 * step + 1;                       // (64 probes below hi, none past t)
        else {
            const uint32_t f = (uint32_t)__builtin_ctzll(b);
            const uint64_t top = lo + f * step;
            if (top < hi) hi = top;
            if (f) lo += (f - 1) * step + 1;
        }
        step = (hi - lo) / RR_WAVE + 1;
    }
    return lo;
}
// the same by one lane (its own arguments): a binary search
__device__ __forceinline__ uint64_t lane_find(const uint64_t *__restrict__ offs, uint64_t lo, uint64_t hi, uint64_t t) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (offs[mid + 1] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// len (1..16) bytes at data[at ..), at + len <= cap, in the low bytes of the result; reads inside [data, data + cap)
__device__ __forceinline__ unsigned __int128 load_seg(const uint8_t *__restrict__ data, uint64_t cap, uint64_t at, uint32_t len) {
    if (cap >= 16) {
        const uint64_t a = at + 16 <= cap ? at : cap - 16;
        const u128_ua x = *reinterpret_cast<const u128_ua *>(data + a);
        const unsigned __int128 v = ((unsigned __int128)(((uint64_t)x.d << 32) | x.c) << 64) | (((uint64_t)x.b << 32) | x.a);
        return v >> (8 * (uint32_t)(at - a));
    }
    unsigned __int128 v = 0;
    for (uint32_t k = 0; k < len; ++k) v |= (unsigned __int128)data[at + k] << (8 * k);
    return v;
}

// offs scanned.  The gather, and in front of it the per-value end of the stage: RR_E_CAPACITY, the totals.
__global__ __launch_bounds__(WPB * RR_WAVE) void merge_emit_kernel(Stage A, Stage B, Stage C, uint64_t n,
                                                                   const uint64_t *__restrict__ offs,
                                                                   const uint64_t *__restrict__ src, uint8_t *__restrict__ out,
                                                                   uint64_t out_cap, uint8_t *__restrict__ status,
                                                                   const uint64_t *err, rr_totals *totals) {
    const uint32_t lane = lane_id();
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t total = first64(offs[n]);
    if (gtid == 0) totals->bytes = *err ? ~0ull : total;
    uint64_t pay = 0, nel = 0, n_bad = 0;
    for (uint64_t i = gtid; i < n; i += nthreads) {
        uint32_t st = status[i];
        const uint64_t b0 = offs[i], b1 = offs[i + 1];
        if (st == RR_OK && b1 > out_cap) status[i] = (uint8_t)(st = RR_E_CAPACITY);
        if (st) ++n_bad;
        else {
            pay += b1 - b0;
            nel += (src[i] >> 62) >= 2;
        }
    }
    add_totals(totals, sum_lanes(pay), sum_lanes(nel), sum_lanes(n_bad));

    const uint64_t end = total < out_cap ? total : out_cap;    // nothing at or past it is written
    const uint64_t wave = first64(gtid / RR_WAVE), nwaves = nthreads / RR_WAVE;
    for (uint64_t s0 = wave * SPAN; s0 < end; s0 += nwaves * SPAN) {
        const uint64_t s1 = end - s0 < SPAN ? end : s0 + SPAN;
        uint64_t vrow = wave_find(offs, 0, n - 1, s0);         // the value under the row's first byte
        for (uint64_t r0 = s0; r0 < s1; r0 += ROW) {
            const uint64_t r1 = s1 - r0 < ROW ? s1 : r0 + ROW;
            const uint64_t vlast = wave_find(offs, vrow, n - 1, r1 - 1);   // under its last byte
            const uint64_t c0 = r0 + 16 * lane;
            if (c0 < r1) {
                const uint64_t c1 = r1 - c0 < 16 ? r1 : c0 + 16;
                uint64_t v = lane_find(offs, vrow, vlast, c0);
                unsigned __int128 acc = 0;
                uint32_t have = 0;                             // bit k: byte k of the piece is written
                for (uint64_t pos = c0;;) {
                    const uint64_t b0 = offs[v], b1 = offs[v + 1], e = b1 < c1 ? b1 : c1;
                    const uint64_t from = src[v];
                    const uint32_t k = (uint32_t)(from >> 62), len = (uint32_t)(e - pos), sh = (uint32_t)(pos - c0);
                    if (k && b1 <= out_cap) {
                        const uint8_t *__restrict__ hdata = k == 1 ? A.data : k == 2 ? B.data : C.data;
                        const uint64_t hcap = k == 1 ? A.cap : k == 2 ? B.cap : C.cap;
                        const unsigned __int128 x = load_seg(hdata, hcap, (from & SRC_AT) + (pos - b0), len);
                        acc |= x << (8 * sh);                  // (bytes of x past len land past the segment: masked below or overwritten)
                        acc &= len + sh >= 16 ? ~(unsigned __int128)0 : (((unsigned __int128)1 << (8 * (len + sh))) - 1);
                        have |= ((1u << len) - 1) << sh;
                    }
                    pos = e;
                    if (pos >= c1) break;
                    v = lane_find(offs, v + 1, vlast, pos);    // past the values of size 0
                }
                if (have == 0xFFFF)
                    *reinterpret_cast<uint4 *>(out + c0) = make_uint4((uint32_t)acc, (uint32_t)(acc >> 32), (uint32_t)(acc >> 64), (uint32_t)(acc >> 96));
                else
                    for (uint32_t k = 0; k < 16; ++k)
                        if (have >> k & 1) out[c0 + k] = (uint8_t)(acc >> (8 * k));
            }
            vrow = vlast;   // the next row begins in it or behind it
        }
    }
}

__global__ void stage_bytes_kernel(const uint64_t *a, const uint64_t *b, const uint64_t *c, uint64_t n, uint64_t *dst) {
    if (threadIdx.x < 3) dst[threadIdx.x] = (threadIdx.x == 0 ? a : threadIdx.x == 1 ? b : c)[n];
}

}  // namespace

// scratch: the scan's look-back words | its error word | src[n]
extern "C" uint64_t rr_rdbmerge_scratch_words(uint64_t n) { return rr_scan_words(n) + 1 + n; }

extern "C" hipError_t rr_launch_rdbmerge(const rr_blob_batch *in1, const uint8_t *s1, const rr_blob_batch *in2, const uint8_t *s2,
                                         const uint8_t *conv_types, const rr_blob_batch *in3, const uint8_t *s3,
                                         const uint8_t *types, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_offs,
                                         uint8_t *out_types, uint8_t *status, uint64_t *scratch, rr_totals *totals,
                                         hipStream_t stream) {
    const Stage A = {in1->data, in1->offsets, s1, in1->data_cap}, B = {in2->data, in2->offsets, s2, in2->data_cap},
                C = {in3->data, in3->offsets, s3, in3->data_cap};
    uint64_t *lb = scratch, *err = lb + rr_scan_words(n), *src = err + 1;
    hipLaunchKernelGGL(merge_size_kernel, dim3(capped_grid(n, 256, 16384)), dim3(256), 0, stream, A, B, C, types, conv_types, n,
                       out_offs, src, out_types, status, lb, (uint64_t)(src - lb), totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(out_offs, n, lb, err, stream);
    if (e != hipSuccess) return e;
    const uint64_t spans = (out_cap + SPAN - 1) / SPAN, values = (n + 255) / 256;   // the gather's spans, the prologue's values
    hipLaunchKernelGGL(merge_emit_kernel, dim3(capped_grid(spans > values * WPB ? spans : values * WPB, WPB, GRID_CAP)),
                       dim3(WPB * RR_WAVE), 0, stream, A, B, C, n, (const uint64_t *)out_offs, (const uint64_t *)src, out, out_cap,
                       status, (const uint64_t *)err, totals);
    return hipGetLastError();
}

extern "C" hipError_t rr_launch_rdbmerge_stage_bytes(const uint64_t *o1, const uint64_t *o2, const uint64_t *o3, uint64_t n,
                                                     uint64_t *dst, hipStream_t stream) {
    hipLaunchKernelGGL(stage_bytes_kernel, dim3(1), dim3(64), 0, stream, o1, o2, o3, n, dst);
    return hipGetLastError();
}
