// rr_rdbread.hip — gfx950 kernels of include/rr_rdbread.h: the records of an RDB stream, whose
// extents the host index found (rr_rdbread_api.c), split into what rdbLoadRio's loop (rdb.c:2072-2242)
// hands on for each key: the prefix opcodes' values, the type, the key's bytes and the value's
// payload in rr_rdbload_batch's input shape; and the verdict on the stream's checksum (:2298-2311).
//
// The shape is rr_stage_device.h's (size, scan, emit), with loops of its own: a record has two
// outputs, so one scan runs over key sizes | payload sizes in the call's scratch, the emit kernel
// writes both offsets arrays, and the call reports through rr_rdbfile_result.  split_size_kernel takes
// every decision (the status, the key's loaded length, which for an LZF key means walking its stream,
// the payload's length); split_emit_kernel writes the keys and payloads that are valid and fit.
//
// The key is read by the reader the RDB load
// kernels share (rr_rdbload_device.h: parse_len, rd_string, emit_string, the LZF routines), and that
// reader is wave-uniform: a header is one 64-byte load, a byte a lane, picked apart with readlane,
// the state lives in scalar registers, and the lanes copy.  The prefix opcodes are read the same way,
// as many as one 64-byte load holds.  Every load of record bytes in the size pass goes through a
// buffer resource that covers exactly [rec_start, rec_end), so a wrong length reads zeros, never a
// neighbour; the emit pass walks records the size pass accepted.  The payload is wave_copy's:
// bytes up to the destination's 16-byte boundary, 16 bytes a lane, the tail bytes.
#include <hip/hip_runtime.h>

#include "rr_rdbload_device.h"
#include "rr_kernels.h"
#include "../../include/rr_rdbread.h"

using namespace rr;

namespace {

constexpr uint32_t WPB = 4;                                   // waves (records in flight) per workgroup
constexpr uint32_t GRID_CAP = RR_RDBREAD_MAX_WAVES / WPB;     // workgroups
static_assert(RR_RDBREAD_LANE_BYTES == 16 && RR_RDBREAD_WAVE_STEP == RR_WAVE * 16, "wave_copy's shape");

// what the prefix opcodes and the type byte say
struct Pre {
    uint32_t type;
    int32_t freq;       // -1: none
    int64_t expire;     // -1: none
    uint64_t idle;      // ~0: none
};
__device__ __forceinline__ Pre no_pre() { return {0u, -1, -1ll, ~0ull}; }

// The prefix opcodes and the type at r.p (rdb.c:2079-2104, :2231); r.p moves behind the type.  One
// 64-byte load serves every opcode that lies whole in it (an opcode and its argument: 10 bytes at
// most).  A repeated opcode overwrites the earlier one, as the reference's loop does.
__device__ __forceinline__ uint32_t rd_prefix(Rd &r, Pre &P) {
    P = no_pre();
    uint32_t base = r.p;
    uint32_t v = ld8(r.R, base + lane_id());
    for (;;) {
        if (r.p >= r.n) return RR_RDBREAD_E_TRUNC;
        if (r.p - base + 10 > RR_WAVE) {
            base = r.p;
            v = ld8(r.R, base + lane_id());
        }
        const uint32_t avail = r.n - r.p, i = r.p - base;
        const uint32_t op = rl32(v, i);
        if (op == 0xFD) {                                      // EXPIRETIME: int32 seconds (rdbLoadTime), times 1000
            if (avail < 5) return RR_RDBREAD_E_TRUNC;
            P.expire = (int64_t)(int32_t)(uint32_t)le_lanes(v, i + 1, 4) * 1000;
            r.p += 5;
        } else if (op == 0xFC) {                               // EXPIRETIME_MS
            if (avail < 9) return RR_RDBREAD_E_TRUNC;
            P.expire = (int64_t)le_lanes(v, i + 1, 8);
            r.p += 9;
        } else if (op == 0xF9) {                               // FREQ
            if (avail < 2) return RR_RDBREAD_E_TRUNC;
            P.freq = (int32_t)rl32(v, i + 1);
            r.p += 2;
        } else if (op == 0xF8) {                               // IDLE: rdbLoadLen, a count site
            bool ie;
            uint64_t val;
            uint32_t used;
            const uint32_t st = parse_len(v, i + 1, avail - 1, ie, val, used);
            if (st) return st == RR_RDBLOAD_E_TRUNC ? RR_RDBREAD_E_TRUNC : RR_RDBREAD_E_OPCODE;
            P.idle = val;
            r.p += 1 + used;
        } else if (op == 0xF7 || op == 0xFA || op == 0xFB || op == 0xFE || op == 0xFF) {
            return RR_RDBREAD_E_OPCODE;
        } else {
            P.type = op;
            r.p += 1;
            return RR_OK;
        }
    }
}

// y[0, n) the keys' sizes, y[n, 2n) the payloads', y[2n] = 0 (the scan's total); the per-record arrays;
// and the stage's zeroing
__global__ __launch_bounds__(WPB * RR_WAVE) void split_size_kernel(const uint8_t *__restrict__ data, uint64_t data_cap,
                                                                   const uint64_t *__restrict__ rec_start,
                                                                   const uint64_t *__restrict__ rec_end, uint64_t n,
                                                                   uint64_t *__restrict__ y, rr_rdbread_out O,
                                                                   uint64_t *__restrict__ zero, uint64_t nzero,
                                                                   rr_rdbfile_result *result) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    zero_stage_words(gtid, nthreads, zero, nzero, &y[2 * n], result);
    const uint64_t nwaves = nthreads / RR_WAVE;
    for (uint64_t v = first64(gtid / RR_WAVE); v < n; v += nwaves) {
        const uint64_t s = first64(rec_start[v]), e = first64(rec_end[v]);
        uint32_t st = RR_RDBREAD_E_SLICE;
        uint64_t ksize = 0, psize = 0;
        Pre P = no_pre();
        if (slice_ok(s, e, data_cap)) {
            Rd r = rd_of(data, s, e);
            st = rd_prefix(r, P);
            if (!st) {
                Str k;
                st = rd_string<true>(r, k);                    // the key, :2231
                if (st) st = st == RR_RDBLOAD_E_TRUNC ? RR_RDBREAD_E_TRUNC : RR_RDBREAD_E_KEY;
                else {
                    ksize = k.len;
                    psize = r.n - r.p;
                }
            }
            if (st) P = no_pre();
        }
        if (lane_id() == 0) {
            y[v] = ksize;
            y[n + v] = psize;
            O.types[v] = (uint8_t)P.type;
            O.expires[v] = P.expire;
            O.idle[v] = P.idle;
            O.freq[v] = (int16_t)P.freq;
            O.status[v] = (uint8_t)st;
        }
    }
}

// y scanned: y[v] key v's start, y[n] the keys' total, y[n + v] - y[n] payload v's start.
__global__ __launch_bounds__(WPB * RR_WAVE) void split_emit_kernel(const uint8_t *__restrict__ data,
                                                                   const uint64_t *__restrict__ rec_start,
                                                                   const uint64_t *__restrict__ rec_end, uint64_t n,
                                                                   const uint64_t *__restrict__ y, rr_rdbread_out O,
                                                                   const uint64_t *err, rr_rdbfile_result *result) {
    const uint32_t lane = lane_id();
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = nthreads / RR_WAVE;
    const uint64_t ktot = first64(y[n]), ptot = first64(y[2 * n]) - ktot;
    const uint64_t kcap = O.keys.data_cap, pcap = O.payloads.data_cap;
    if (gtid == 0) {
        result->bytes = *err ? ~0ull : ptot;
        result->status = ktot > kcap || ptot > pcap ? RR_E_CAPACITY : RR_OK;
        O.keys.offsets[n] = ktot;
        O.payloads.offsets[n] = ptot;
    }
    uint64_t n_bad = 0;   // wave-uniform
    for (uint64_t v = first64(gtid / RR_WAVE); v < n; v += nwaves) {
        const uint64_t k0 = first64(y[v]), k1 = first64(y[v + 1]);
        const uint64_t p0 = first64(y[n + v]) - ktot, p1 = first64(y[n + v + 1]) - ktot;
        if (lane == 0) {
            O.keys.offsets[v] = k0;
            O.payloads.offsets[v] = p0;
        }
        if (rfl(O.status[v])) { ++n_bad; continue; }
        if (k1 > kcap || p1 > pcap) {
            ++n_bad;
            if (lane == 0) O.status[v] = RR_E_CAPACITY;
            continue;
        }
        const uint64_t s = first64(rec_start[v]), e = first64(rec_end[v]);
        Rd r = rd_of(data, s, e);
        Pre P;
        Str k;
        rd_prefix(r, P);
        rd_string<false>(r, k);
        emit_string(r, k, O.keys.data + k0);
        if (p1 > p0) wave_copy(O.payloads.data + p0, r.base + r.p, (uint32_t)(p1 - p0));
    }
    if (lane == 0 && n_bad) atomicAdd((unsigned long long *)&result->n_bad, (unsigned long long)n_bad);
}

// The computed checksum against the 8 little-endian bytes at ck (rdb.c:2298-2311); one wave.
__global__ __launch_bounds__(RR_WAVE) void verdict_kernel(const uint8_t *__restrict__ ck, uint64_t bytes,
                                                          const uint64_t *__restrict__ state, rr_rdbfile_result *result) {
    const uint32_t lane = lane_id();
    const uint32_t b = lane < 8 ? (uint32_t)ck[lane] : 0u;
    const uint64_t want = le_lanes(b, 0, 8), got = first64(state[0]);
    const uint32_t st = want == 0 ? RR_RDBREAD_NO_CKSUM : want == got ? RR_OK : RR_RDBDUMP_E_CRC;
    if (lane == 0) {
        result->bytes = bytes;
        result->n_bad = st == RR_RDBDUMP_E_CRC;
        result->status = st;
        result->rsv = 0;
    }
}

}  // namespace

// scratch: y[2n + 1] | the scan's look-back words | the error word
extern "C" uint64_t rr_rdbread_scratch_words(uint64_t n) { return 2 * n + 1 + rr_scan_words(2 * n) + 1; }

extern "C" hipError_t rr_launch_rdbread_split(const uint8_t *data, uint64_t data_cap, const uint64_t *rec_start,
                                              const uint64_t *rec_end, uint64_t n, const rr_rdbread_out *out, uint64_t *scratch,
                                              rr_rdbfile_result *result, hipStream_t stream) {
    const uint64_t lbw = rr_scan_words(2 * n);
    uint64_t *y = scratch, *lb = y + 2 * n + 1, *err = lb + lbw;
    const uint32_t grid = capped_grid(n, WPB, GRID_CAP);   // a wave a record
    hipLaunchKernelGGL(split_size_kernel, dim3(grid), dim3(WPB * RR_WAVE), 0, stream, data, data_cap, rec_start, rec_end, n, y,
                       *out, lb, lbw + 1, result);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(y, 2 * n, lb, err, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(split_emit_kernel, dim3(grid), dim3(WPB * RR_WAVE), 0, stream, data, rec_start, rec_end, n,
                       (const uint64_t *)y, *out, (const uint64_t *)err, result);
    return hipGetLastError();
}

extern "C" hipError_t rr_launch_rdbread_verdict(const uint8_t *ck, uint64_t bytes, const uint64_t *state, rr_rdbfile_result *result,
                                                hipStream_t stream) {
    hipLaunchKernelGGL(verdict_kernel, dim3(1), dim3(RR_WAVE), 0, stream, ck, bytes, state, result);
    return hipGetLastError();
}
