// rr_flat_device.h — device helpers shared by the kernels that work on flat batches.  The decode
// and encode kernels use all of it; rr_rdbsave.hip uses ElemV, get_elem and in_arena.
#pragma once
#include "../../include/rr_serdes.h"
#include "rr_device.h"

#ifndef RR_ABLATE   // timing-only ablations (tools/, wrong results): 1-6 the decode's, 7-10 the
#define RR_ABLATE 0       // encode's; each is listed beside the kernels it changes
#endif

namespace rr {

// a descriptor (rr_elem) in registers: one 16-byte load
struct ElemV {
    uint64_t data;
    uint32_t len;
    uint32_t kind;
};
__device__ __forceinline__ ElemV get_elem(const rr_elem *e) {
    uint4 w = *reinterpret_cast<const uint4 *>(e);
    return ElemV{(uint64_t)w.x | ((uint64_t)w.y << 32), w.z, w.w & 0xFF};
}
// a STR / ZLRAW descriptor's payload lies inside the caller's arena
__device__ __forceinline__ bool in_arena(const ElemV &e, uint64_t acap) { return e.data <= acap && e.len <= acap - e.data; }

template <uint32_t NT>
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t x, uint64_t *wsum, uint64_t &total) {
    // (the wave scan in DPP when no lane's value reaches 2^26: the wave's sum fits 32 bits)
    const uint64_t incl = wave_incl_scan_fast(x);
    const uint32_t wv = threadIdx.x / RR_WAVE;
    if (lane_id() == RR_WAVE - 1) wsum[wv] = incl;
    lds_barrier();
    uint64_t pre = 0, t = 0;
#pragma unroll
    for (uint32_t k = 0; k < NT / RR_WAVE; ++k) {
        const uint64_t s = wsum[k];
        pre += k < wv ? s : 0;
        t += s;
    }
    total = t;
    return pre + incl - x;
}

// Block 0 also zeroes the pipeline's per-call words (look-back state, fixup header) and the
// totals: later kernels of the same stream use them, so no separate launch is needed.
__device__ __forceinline__ void zero_call_words(uint64_t *words, uint32_t nwords, rr_totals *tot) {
    if (blockIdx.x != 0) return;
    for (uint32_t k = threadIdx.x; k < nwords; k += blockDim.x) words[k] = 0;
    if (tot && threadIdx.x < 4) reinterpret_cast<uint64_t *>(tot)[threadIdx.x] = 0;
}

// the decode's windows / the encode's 256-value blocks per group sum
constexpr uint32_t WGROUP = 16;   // (64: ~260 same-address atomics per group sum on config 1)

// ---- small batches (decode_small_kernel, encode_small_kernel): one workgroup, one launch ----
constexpr uint32_t SMALL_NT = 1024, SMALL_VPT = 4, SMALL_N = SMALL_NT * SMALL_VPT;
constexpr uint32_t SMALL_BYTES = 128 * 1024;   // (one workgroup: up to 160 KiB of LDS)
// batches of at most this many values: one wave per value (the class walks on a wave / the
// whole wave emitting one value); larger ones one lane per value (the exact parser / the byte
// emitter) — which the host takes only for values of at most SMALL_LANE_BYTES on average
// (rr_small_decode_fits): a lane walking a 500-byte value costs ~20 us (round 4: 64 config-4
// values took 368 us through the lane path)
constexpr uint32_t SMALL_GW = 256;
constexpr uint64_t SMALL_LANE_BYTES = 64;

// The host entry points wait for a one-launch kernel by spinning on a word of their mapped
// staging instead of a stream synchronisation (~4 us less per call).  The producer form of
// MI355X_MICROARCH.md (inter-workgroup visibility, "valid forms"): every wave waits for its
// OWN stores to be acknowledged (s_waitcnt vmcnt(0): on gfx950 __syncthreads() is a bare
// s_barrier that waits for nothing in flight), then the barrier, so lane 0 signals only after
// every wave's records, descriptors and totals have landed; lane 0's ONE system-scope release
// (one L2 writeback), an explicit vmcnt(0) wait after it (the compiler may drop its own wait
// after the writeback when the scoreboard looks empty), and the store of the call's sequence
// number.  (A system fence in every thread — sixteen waves, sixteen L2 writebacks — cost ~8 us
// a call: tools/micro/lat_probe.hip, launch + spin 19.4 us against 11.4 us between HIP events.)
__device__ __forceinline__ void signal_done(uint32_t *done, uint32_t seq) {
    if (!done) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // (system scope)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(done, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace rr
