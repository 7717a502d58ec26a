// rr_stage_device.h — the stage around a per-value codec, shared by the kernels that turn n values
// into n variable-sized outputs: size launch, rr_launch_scan_u64, emit launch.
//
//   size   a wave a value, values strided over a capped grid: the value's output size into offs[v] and
//          its status; the first kernel of a call also zeroes what the later launches rely on (the
//          scan's look-back and error words, offs[n], the call's totals): zero_stage_words.
//   scan   offs[] becomes the outputs' starts, offs[n] their end; a wait that was cut sets the error word.
//   emit   the same walk over the values the size pass accepted, each writing at its start; a value
//          that ends past the capacity gets RR_E_CAPACITY; the totals.
//
// Every stage keeps its own loops, WPB and LDS; what is here is what the loops are made of, one
// definition each ("The stage skeleton", says why the loops themselves are not here).
//
// The attempted list (rr_rdbconvert.hip, rr_rdbzset.hip): the values a stage works on are the rare
// class of a batch, so three launches in front (flag_kernel, scan, compact_kernel) leave their
// indices, in order, in a list the size and emit kernels walk: AttScratch, launch_attempted.
#pragma once
#include "rr_device.h"
#include "rr_kernels.h"

namespace rr {

// ---- leaves ----------------------------------------------------------------------------------------
constexpr uint64_t MAX_SLICE = 0x7FFFFFF0ull;   // a buffer resource's reach
constexpr uint32_t SHORT_BODY = 32;             // a body of up to this many bytes is copied by its own lane

// [o0, o1) is a slice of cap bytes that a buffer resource can cover
__device__ __forceinline__ bool slice_ok(uint64_t o0, uint64_t o1, uint64_t cap) { return o0 <= o1 && o1 <= cap && o1 - o0 < MAX_SLICE; }

// a flat batch's value record x (one 16-byte load): decoded without error, its descriptors inside elems
__device__ __forceinline__ bool value_ok(const uint4 &x, uint64_t elem_cap) {
    const uint32_t vstatus = (x.x >> 16) & 0xFFFF;
    return vstatus == RR_OK && (uint64_t)x.w + (uint64_t)x.z <= elem_cap;
}

// Wave64 inclusive scan of costs below 2^40 (a cost is at most 2^32 + 8), every lane active: the low
// 24 bits and the rest scanned apart by the u32 DPP scan, which needs no per-step lane predicates
// (the u64 shuffle scan keeps six of them in SGPR pairs, and they spilled in rr_rdbsave.hip).
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

// a lane's body: by the lane itself when short, else by the whole wave, the lanes' bodies in turn
__device__ __forceinline__ void copy_bodies(uint8_t *dst, const uint8_t *__restrict__ src, uint32_t len, bool mine) {
    if (mine && len <= SHORT_BODY)
        for (uint32_t k = 0; k < len; ++k) dst[k] = src[k];
    wave_copy_each(dst, src, len, mine && len > SHORT_BODY);
}

// a wave's share of the call's totals (wave-uniform arguments), by lane 0
__device__ __forceinline__ void add_totals(rr_totals *totals, uint64_t pay, uint64_t nel, uint64_t n_bad) {
    if (lane_id() != 0) return;
    if (pay) atomicAdd((unsigned long long *)&totals->payload, (unsigned long long)pay);
    if (nel) atomicAdd((unsigned long long *)&totals->n_elems, (unsigned long long)nel);
    if (n_bad) atomicAdd((unsigned long long *)&totals->n_bad, (unsigned long long)n_bad);
}

// The first kernel's prologue, by the whole grid (thread gtid of nthreads): zero[0, nzero) (the scans'
// look-back and error words), *end (the word behind the sizes, which the scan turns into their total)
// and the call's result (rr_totals, rr_rdbfile_result).  The later launches of the stream rely on it.
template <typename Res>
__device__ __forceinline__ void zero_stage_words(uint64_t gtid, uint64_t nthreads, uint64_t *__restrict__ zero, uint64_t nzero,
                                                 uint64_t *end, Res *res) {
    for (uint64_t k = gtid; k < nzero; k += nthreads) zero[k] = 0;
    if (gtid == 0) {
        *end = 0;
        *res = Res{};
    }
}

// workgroups for n items, per_block a workgroup, at least one and at most cap (a grid stride beyond)
inline uint32_t capped_grid(uint64_t n, uint64_t per_block, uint32_t cap) {
    const uint64_t b = (n + per_block - 1) / per_block;
    return (uint32_t)(b < cap ? (b ? b : 1) : cap);
}

// ---- the attempted list ----------------------------------------------------------------------------
// P(i): value i is attempted.  att[i] = P(i) (att[n] = 0); what a value keeps when nothing more is
// done with it: size 0, type 0 (out_types may be NULL), status `tried` if attempted, else `skip`; and
// the stage's zeroing, both scans' words.
template <class Pred>
__global__ __launch_bounds__(256) void flag_kernel(Pred P, uint64_t n, uint64_t *__restrict__ att, uint64_t *__restrict__ out_offs,
                                                   uint8_t *__restrict__ out_types, uint8_t *__restrict__ status, uint8_t tried,
                                                   uint8_t skip, uint64_t *__restrict__ zero, uint64_t nzero, rr_totals *totals) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    zero_stage_words(gtid, nthreads, zero, nzero, &out_offs[n], totals);
    if (gtid == 0) att[n] = 0;
    for (uint64_t i = gtid; i < n; i += nthreads) {
        const bool a = P(i);
        att[i] = a ? 1 : 0;
        out_offs[i] = 0;
        if (out_types) out_types[i] = 0;
        status[i] = a ? tried : skip;
    }
}
// att scanned: list[att[i]] = i for the attempted values
template <class Pred>
__global__ __launch_bounds__(256) void compact_kernel(Pred P, uint64_t n, const uint64_t *__restrict__ att, uint32_t *__restrict__ list) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthreads)
        if (P(i)) list[att[i]] = (uint32_t)i;
}

// such a stage's scratch: two scans' look-back and error words, att[n + 1], list[n] (u32)
struct AttScratch {
    uint64_t *lb1, *err1, *lb2, *err2, *att;
    uint32_t *list;
    AttScratch(uint64_t *scratch, uint64_t n) {
        const uint64_t lbw = rr_scan_words(n);
        lb1 = scratch, err1 = lb1 + lbw, lb2 = err1 + 1, err2 = lb2 + lbw, att = err2 + 1;
        list = (uint32_t *)(att + n + 1);
    }
    static uint64_t words(uint64_t n) { return 2 * (rr_scan_words(n) + 1) + (n + 1) + (n + 1) / 2 + 1; }
};

// flags, scan, compaction: S.list and S.att[n] are what the size and emit launches walk
template <class Pred>
inline hipError_t launch_attempted(Pred P, uint64_t n, const AttScratch &S, uint64_t *out_offs, uint8_t *out_types, uint8_t *status,
                                   uint8_t tried, uint8_t skip, rr_totals *totals, hipStream_t stream) {
    const uint32_t grid = capped_grid(n, 256, 16384);   // a thread a value
    hipLaunchKernelGGL(flag_kernel<Pred>, dim3(grid), dim3(256), 0, stream, P, n, S.att, out_offs, out_types, status, tried, skip,
                       S.lb1, (uint64_t)(S.att - S.lb1), totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(S.att, n, S.lb1, S.err1, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(compact_kernel<Pred>, dim3(grid), dim3(256), 0, stream, P, n, (const uint64_t *)S.att, S.list);
    return hipGetLastError();
}

}  // namespace rr
