// rr_util.hip — small gfx950 kernels beside the decode / encode pipelines: the shard helpers of
// rr_shard.c, the streaming copy kernel (the roofline anchor) and the look-back scan of u64 sizes
// (rr_launch_scan_u64: the snappy and lz4 kernels' block lengths).
#include <hip/hip_runtime.h>

#include "rr_device.h"
#include "rr_kernels.h"

using namespace rr;

// ---------------------------------------------------------------------------------------- shards
// Multi-GPU sharding (rr_shard.c): values are independent, so a batch splits
// into contiguous value ranges balanced by bytes, shard k starting at the first value whose
// first byte is at or after k * total / g.  Three small kernels serve rr_shard.c:

// plan[4k..4k+3] = {v0, v1, b0, b1} of shard k (thread k: two lower-bound searches)
__global__ __launch_bounds__(64) void shard_plan_kernel(const uint64_t *__restrict__ offsets, uint64_t n, uint32_t g,
                                                        uint64_t *__restrict__ plan) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= g) return;
    const uint64_t total = offsets[n];
    uint64_t cut[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const uint32_t kk = k + e;
        if (kk == 0) { cut[e] = 0; continue; }
        if (kk == g) { cut[e] = n; continue; }
        const uint64_t target = (uint64_t)(((unsigned __int128)total * kk) / g);
        uint64_t lo = 0, hi = n;   // first v in [0, n) with offsets[v] >= target, else n
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (offsets[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        cut[e] = lo;
    }
    plan[4 * (uint64_t)k + 0] = cut[0];
    plan[4 * (uint64_t)k + 1] = cut[1];
    plan[4 * (uint64_t)k + 2] = offsets[cut[0]];
    plan[4 * (uint64_t)k + 3] = offsets[cut[1]];
}

// words[0, n) = 0 (the graph-captured decode's sums, re-zeroed at every replay: a captured
// hipMemsetAsync measured as not re-running on replay on this stack, tools/graph_diag.py)
__global__ __launch_bounds__(256) void zero_words_kernel(uint64_t *__restrict__ words, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        words[i] = 0;
}
extern "C" hipError_t rr_launch_zero_words(uint64_t *words, uint64_t n, hipStream_t stream) {
    if (!n) return hipSuccess;
    const uint64_t b = (n + 255) / 256;
    hipLaunchKernelGGL(zero_words_kernel, dim3((uint32_t)(b < 256 ? b : 256)), dim3(256), 0, stream, words, n);
    return hipGetLastError();
}

// offsets[i] -= sub (a received shard's offsets, relative to its first byte)
__global__ __launch_bounds__(256) void offsets_rebase_kernel(uint64_t *__restrict__ offs, uint64_t count, uint64_t sub) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) offs[i] -= sub;
}

// A decoded shard placed in the whole batch: elem_base += elem_add; the arena offsets of STR /
// ZLRAW descriptors += byte_add (the arena mirrors the blob buffer, so a shard's arena is the
// whole arena's slice at the shard's first byte).  The zero-filled slots of a malformed value
// (kind STR, data 0, len 0 — no real string starts at byte 0 of a value) stay zero.
__global__ __launch_bounds__(256) void flat_rebase_kernel(rr_value *__restrict__ values, uint64_t n,
                                                          rr_elem *__restrict__ elems, uint64_t ne,
                                                          uint64_t elem_add, uint64_t byte_add) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n || i < ne; i += stride) {
        if (i < n) {
            uint4 v = reinterpret_cast<uint4 *>(values)[i];
            v.w += (uint32_t)elem_add;
            reinterpret_cast<uint4 *>(values)[i] = v;
        }
        if (i < ne) {
            uint4 e = reinterpret_cast<uint4 *>(elems)[i];
            const uint32_t kind = e.w & 0xFF;
            const uint64_t d = (uint64_t)e.x | ((uint64_t)e.y << 32);
            if ((kind == RR_K_STR || kind == RR_K_ZLRAW) && (d | e.z) != 0) {
                const uint64_t d2 = d + byte_add;
                e.x = (uint32_t)d2;
                e.y = (uint32_t)(d2 >> 32);
                reinterpret_cast<uint4 *>(elems)[i] = e;
            }
        }
    }
}

extern "C" hipError_t rr_launch_shard_plan(const uint64_t *offsets, uint64_t n, uint32_t g, uint64_t *plan,
                                           hipStream_t stream) {
    hipLaunchKernelGGL(shard_plan_kernel, dim3((g + 63) / 64), dim3(64), 0, stream, offsets, n, g, plan);
    return hipGetLastError();
}
extern "C" hipError_t rr_launch_offsets_rebase(uint64_t *offs, uint64_t count, uint64_t sub, hipStream_t stream) {
    if (count == 0 || sub == 0) return hipSuccess;
    hipLaunchKernelGGL(offsets_rebase_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, stream, offs, count,
                       sub);
    return hipGetLastError();
}
extern "C" hipError_t rr_launch_flat_rebase(rr_value *values, uint64_t n, rr_elem *elems, uint64_t ne, uint64_t elem_add,
                                            uint64_t byte_add, hipStream_t stream) {
    const uint64_t m = n > ne ? n : ne;
    if (m == 0 || (elem_add == 0 && byte_add == 0)) return hipSuccess;
    uint64_t blocks = (m + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(flat_rebase_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, values, n, elems, ne, elem_add,
                       byte_add);
    return hipGetLastError();
}

// ---- streaming device copy: the roofline anchor (SURVEY.md §8d "a measured device copy-kernel
// bandwidth on the box") -----------------------------------------------------------------------
// The same bytes-per-lane shape the decode's window copy uses: 16-byte buffer loads, COPY_U of
// them in flight per lane before any store, nontemporal 16-byte stores; a workgroup per
// COPY_U * 256 * 16 bytes (≫ 256 CUs' worth of workgroups), blocks dealt over the XCDs in
// order.  Bytes past the end read as zeros and their stores are dropped (buffer range), so
// there is no tail branch.  Used by bench.py as `copy_ref`; no part of the serdes path.
//
// Shapes (rr_copy_shape, tools/time_copy.py): U 16-byte loads in flight per lane, NT threads, a
// workgroup per U * NT * 16 bytes (one pass) or a resident grid striding over the buffer, and
// nontemporal (aux 2) or default-policy stores.
template <uint32_t U, uint32_t NT, bool NTS, bool NTL = false>
__global__ __launch_bounds__(NT) void copy_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                  uint64_t bytes) {
    constexpr uint64_t TILE = (uint64_t)U * NT * 16;
    for (uint64_t base = (uint64_t)blockIdx.x * TILE; base < bytes; base += (uint64_t)gridDim.x * TILE) {
        const uint64_t left = bytes - base;
        const uint32_t span = left < TILE ? (uint32_t)left : (uint32_t)TILE;
        const rsrc_t RS = mk_rsrc(src + base, span), RD = mk_rsrc(dst + base, span);
        u32x4 x[U];
#pragma unroll
        for (uint32_t k = 0; k < U; ++k)
            x[k] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(RS, (int)((threadIdx.x + k * NT) * 16), 0,
                                                                                 NTL ? 2 : 0));
#pragma unroll
        for (uint32_t k = 0; k < U; ++k)
            __builtin_amdgcn_raw_buffer_store_b128(x[k], RD, (int)((threadIdx.x + k * NT) * 16), 0, NTS ? 2 : 0);
    }
}

template <uint32_t U, uint32_t NT, bool NTS, bool NTL = false>
static hipError_t launch_copy_shape(uint8_t *dst, const uint8_t *src, uint64_t bytes, uint32_t grid, hipStream_t stream) {
    const uint64_t tiles = (bytes + (uint64_t)U * NT * 16 - 1) / ((uint64_t)U * NT * 16);
    if (grid == 0 || grid > tiles) grid = (uint32_t)tiles;
    hipLaunchKernelGGL((copy_kernel<U, NT, NTS, NTL>), dim3(grid), dim3(NT), 0, stream, src, dst, bytes);
    return hipGetLastError();
}

// shape: 0 = the default below; 1-8 = the alternatives timed by tools/time_copy.py (diagnostics).
// Measured (497 MB, read + write bytes): 4 granules per thread with nontemporal loads and stores
// 6.36 TB/s, 1 per thread 6.30, nontemporal stores only 5.85-5.89 (2 or 4 per thread), 8 per
// thread (round 3's) 5.56, a resident-size grid 5.72.
extern "C" hipError_t rr_launch_copy_shape(uint8_t *dst, const uint8_t *src, uint64_t bytes, int shape,
                                           hipStream_t stream) {
    if (bytes == 0) return hipSuccess;
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    switch (shape) {
        case 1: return launch_copy_shape<8, 256, true>(dst, src, bytes, 0, stream);   // (round 3's)
        case 2: return launch_copy_shape<4, 256, true>(dst, src, bytes, 0, stream);
        case 3: return launch_copy_shape<2, 256, true>(dst, src, bytes, 0, stream);
        case 4: return launch_copy_shape<1, 256, true>(dst, src, bytes, 0, stream);
        case 5: return launch_copy_shape<4, 256, true, true>(dst, src, bytes, 0, stream);
        case 6: return launch_copy_shape<2, 512, true>(dst, src, bytes, 0, stream);
        case 7: return launch_copy_shape<4, 1024, true>(dst, src, bytes, 0, stream);
        case 8: return launch_copy_shape<4, 256, true>(dst, src, bytes, (uint32_t)cus * 16, stream);
        default: return launch_copy_shape<4, 256, true, true>(dst, src, bytes, 0, stream);   // (= 5: 6.36 TB/s)
    }
}

extern "C" hipError_t rr_launch_copy(uint8_t *dst, const uint8_t *src, uint64_t bytes, hipStream_t stream) {
    return rr_launch_copy_shape(dst, src, bytes, 0, stream);
}

// ---- exclusive scan of u64 sizes (rr_launch_scan_u64: the snappy and lz4 block lengths) ----
// 4096 values per 256-thread workgroup, tile ids from an atomic ticket (so a tile only waits
// on tiles already running), decoupled look-back between tiles (two-level, rr_device.h).
namespace {

constexpr uint32_t SCAN_PER_THREAD = 16;
constexpr uint32_t SCAN_TILE = 256 * SCAN_PER_THREAD;
uint64_t scan_tiles(uint64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

__global__ __launch_bounds__(256) void scan_kernel(uint64_t *__restrict__ counts, uint64_t n, uint64_t *lb,
                                                   uint32_t ntiles, uint64_t *err) {
    __shared__ uint64_t wsum[4];
    __shared__ uint64_t sh_prefix;
    __shared__ uint32_t sh_tile;
    uint64_t *ticket = lb;
    uint64_t *state = lb + 1;
    uint64_t *groups = state + ntiles;
    if (threadIdx.x == 0) sh_tile = (uint32_t)atomicAdd((unsigned long long *)ticket, 1ull);
    __syncthreads();
    const uint32_t tile = sh_tile;
    const uint64_t base = (uint64_t)tile * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_PER_THREAD;
    uint64_t x[SCAN_PER_THREAD];
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER_THREAD; ++k) {
        x[k] = base + k < n ? counts[base + k] : 0;
        sum += x[k];
    }
    const uint64_t incl = wave_incl_scan_fast(sum);
    const uint32_t w = threadIdx.x / RR_WAVE;
    if (lane_id() == RR_WAVE - 1) wsum[w] = incl;
    __syncthreads();
    uint64_t wpre = 0, agg = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        if (k < w) wpre += wsum[k];
        agg += wsum[k];
    }
    if (w == 0) {
        const uint64_t pre = lookback(state, groups, tile, ntiles, agg, err);
        if (lane_id() == 0) sh_prefix = pre;
    }
    __syncthreads();
    uint64_t run = sh_prefix + wpre + incl - sum;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER_THREAD; ++k) {
        if (base + k < n) counts[base + k] = run;
        run += x[k];
    }
    if (tile == ntiles - 1 && threadIdx.x == 255) counts[n] = sh_prefix + agg;
}

}  // namespace

// ---- the look-back scan for other launchers (rr_snappy.hip, rr_lz4.hip) ---------------------
// x[0..n) -> exclusive prefix in place, x[n] = total; lb (rr_scan_words(n) words) must be zero
// and x[n] must be 0 beforehand (the caller's first kernel does both, as count_kernel does).
extern "C" uint64_t rr_scan_words(uint64_t n) {
    const uint64_t st = scan_tiles(n);
    return 1 + st + (st + LB_GROUP - 1) / LB_GROUP;
}
extern "C" hipError_t rr_launch_scan_u64(uint64_t *x, uint64_t n, uint64_t *lb, uint64_t *err, hipStream_t stream) {
    const uint32_t st = (uint32_t)scan_tiles(n);
    if (st) hipLaunchKernelGGL(scan_kernel, dim3(st), dim3(256), 0, stream, x, n, lb, st, err);
    return hipGetLastError();
}
