// rr_lz4.hip — LZ4 block compression / decompression of RocksDB data blocks on gfx950, beside
// rr_snappy.hip (include/rr_lz4.h states the format and the acceptance rule).
//
// One wave per block for both directions, as the snappy kernels: a block is a serial chain of
// sequences, the wave's 64 lanes work inside each step, parallelism comes from many blocks in
// flight.
//
//   (rr_snappy.hip)   the varint32 length preambles and the scan that turns them into offsets
//   lz4_dec_kernel    wave per block.  The compressed bytes staged at the end of an LDS window in
//                     one round of loads, the output assembled in place from the window's start
//                     and written out once.  The sequence chain (token, literal length, offset,
//                     match length, every test of the acceptance rule) is uniform scalar code on
//                     two LDS reads a sequence; the copies are the wave's: literals 16 bytes a
//                     lane, a match by out[op + j] = out[op - offset + j mod offset].  A block
//                     whose input or output exceeds the window, or whose output would catch up
//                     with the compressed bytes not yet read, goes through lz4_walk's other
//                     instantiation: input and output in global memory, the same chain, the same
//                     verdicts.
//   lz4_bound_kernel  thread per block: the output slot sizes
//   lz4_comp_kernel   wave per block.  Two hash tables in LDS (RR_LZ4_HASH_LOG): the latest
//                     position of each hash (16 bits), and a quarter as many entries with the
//                     chunk's first position of each hash beside 16 more hash bits.  64 consecutive
//                     positions hashed and probed a round, the first lane whose candidate (the
//                     latest, else the first) matches wins, the match extended 64 bytes a step.
//                     Nothing depends on timing: the tables' updates are a max and a min (see
//                     insert(), insert_first()), so the same input gives the same bytes on
//                     every run.
//   (rr_snappy.hip)   slots -> packed output
//
// Every loop advances its input position or exits; no wave waits on another.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "rr_device.h"
#include "rr_kernels.h"
#include "../../include/rr_lz4.h"

using namespace rr;

namespace {

constexpr uint32_t WAVE = RR_WAVE;
// LDS window per wave of the decompressor (the block decompressed in place in it), as
// rr_snappy.hip's: 18 KiB holds RocksDB's 16 KiB blocks plus a 2 KiB last entry, 8 waves per CU
#ifndef RR_LZ4_DEC_WIN
#define RR_LZ4_DEC_WIN 18432
#endif
constexpr uint32_t LZ4_DEC_WIN = RR_LZ4_DEC_WIN;
static_assert(LZ4_DEC_WIN % 16 == 0 && LZ4_DEC_WIN >= 1024 && LZ4_DEC_WIN <= 65536 - 64, "window bytes");
// log2 of the entries of the compressor's hash table of latest positions (u16: 8 KiB of LDS per
// wave at 12); the table of first positions has a quarter as many, 32 bits each (4 KiB)
#ifndef RR_LZ4_HASH_LOG
#define RR_LZ4_HASH_LOG 12
#endif
constexpr uint32_t HLOG = RR_LZ4_HASH_LOG, HSIZE = 1u << HLOG;
static_assert(HLOG >= 8 && HLOG <= 14, "hash table size");
constexpr uint32_t FLOG = HLOG - 2, FSIZE = 1u << FLOG;
constexpr uint32_t CHUNK = 1u << 16;   // positions a table entry can hold
constexpr uint32_t MINMATCH = 4, LASTLITERALS = 5, MFLIMIT = 12, FASTLOOP = 64;   // lz4.c:189-195
constexpr uint32_t BAIL = 0xFF;        // (internal) leave the LDS window for the global path

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4_t lds_u32x4;

// ---- decompression ------------------------------------------------------------------------

// Forward copy inside the LDS window by the whole wave: len bytes from s to d, d <= s or the two
// ranges apart.  Up to 64 bytes a byte a lane; longer: bytes to a 4-aligned destination, then
// 16 bytes a lane a round from five aligned source dwords (every lane's reads of a round before
// its writes; a round writes below what later rounds read), then the last < 4 bytes.
__device__ __forceinline__ void lds_copy(lds_u8 *win, uint32_t s, uint32_t d, uint32_t len) {
    lds_u32 *win32 = (lds_u32 *)win;
    const uint32_t lane = lane_id();
    if (len <= WAVE) {
        const uint8_t x = lane < len ? win[s + lane] : 0;
        if (lane < len) win[d + lane] = x;
        return;
    }
    const uint32_t h = (4u - (d & 3)) & 3;
    const uint8_t hx = lane < h ? win[s + lane] : 0;
    if (lane < h) win[d + lane] = hx;
    const uint32_t q0 = s + h, d0 = d + h, body = len - h, nd = body >> 2, a0 = q0 >> 2, sh = q0 & 3;
    for (uint32_t i = 0; i < nd; i += 4 * WAVE) {
        const uint32_t k = i + 4 * lane, sa = k < nd ? a0 + k : 0u;   // (idle lanes: word 0)
        const uint32_t x0 = win32[sa], x1 = win32[sa + 1], x2 = win32[sa + 2], x3 = win32[sa + 3], x4 = win32[sa + 4];
        lds_u32 *w = win32 + (d0 >> 2) + k;
        if (k < nd) w[0] = __builtin_amdgcn_alignbyte(x1, x0, sh);
        if (k + 1 < nd) w[1] = __builtin_amdgcn_alignbyte(x2, x1, sh);
        if (k + 2 < nd) w[2] = __builtin_amdgcn_alignbyte(x3, x2, sh);
        if (k + 3 < nd) w[3] = __builtin_amdgcn_alignbyte(x4, x3, sh);
    }
    const uint32_t t0 = h + 4 * nd, tl = len - t0;
    const uint8_t tx = lane < tl ? win[s + t0 + lane] : 0;
    if (lane < tl) win[d + t0 + lane] = tx;
}

// The block in the LDS window: compressed bytes at win[D + p] (p: position in the block's buffer
// resource), output at win[0, N).
struct LdsMem {
    lds_u8 *win;
    uint32_t D;
    // 5+ bytes at input position p (uniform), low byte first
    __device__ __forceinline__ uint64_t rd(uint32_t p) const {
        const lds_u32 *w = (const lds_u32 *)win;
        const uint32_t a = D + p;
        const uint32_t lo = rfl(w[a >> 2]), hi = rfl(w[(a >> 2) + 1]);
        return (((uint64_t)hi << 32) | lo) >> (8 * (a & 3));
    }
    // len literal bytes from input p to output op; false: the output has caught up with the input
    __device__ __forceinline__ bool literals(uint32_t p, uint32_t op, uint32_t len) {
        if (op > D + p) return false;
        lds_copy(win, D + p, op, len);
        return true;
    }
    // len bytes from offset back at output op; next: the first input byte not read yet
    __device__ __forceinline__ bool match(uint32_t op, uint32_t off, uint32_t len, uint32_t next) {
        if (op + len > D + next) return false;
        if (off >= len && len > WAVE) {
            lds_copy(win, op - off, op, len);
            return true;
        }
        const uint32_t lane = lane_id();
        for (uint32_t r = 0; r < len; r += WAVE) {   // (every source byte lies before op: the rounds are independent)
            const uint32_t j = r + lane, k = off >= len ? j : j % off;
            const uint8_t x = j < len ? win[op - off + k] : 0;
            if (j < len) win[op + j] = x;
        }
        return true;
    }
};

// The block in global memory: input through R, output through Ro (bounded to the block's own
// output range); a match reads its source back through the L2 once the wave's stores have drained.
struct GlobalMem {
    rsrc_t R, Ro;
    __device__ __forceinline__ uint64_t rd(uint32_t p) const {
        const uint32_t a = p & ~3u;
        const uint32_t lo = rfl(__builtin_amdgcn_raw_buffer_load_b32(R, (int)a, 0, 0));
        const uint32_t hi = rfl(__builtin_amdgcn_raw_buffer_load_b32(R, (int)a + 4, 0, 0));
        return (((uint64_t)hi << 32) | lo) >> (8 * (p & 3));
    }
    __device__ __forceinline__ bool literals(uint32_t p, uint32_t op, uint32_t len) {
        const uint32_t lane = lane_id();
        for (uint32_t i = 0; i < len; i += 4 * WAVE) {   // four bytes a lane in flight
            uint8_t x[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                const uint32_t k = i + u * WAVE + lane;
                x[u] = k < len ? __builtin_amdgcn_raw_buffer_load_b8(R, (int)(p + k), 0, 0) : 0;
            }
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                const uint32_t k = i + u * WAVE + lane;
                if (k < len) __builtin_amdgcn_raw_buffer_store_b8(x[u], Ro, (int)(op + k), 0, 0);
            }
        }
        return true;
    }
    __device__ __forceinline__ bool match(uint32_t op, uint32_t off, uint32_t len, uint32_t) {
        const uint32_t lane = lane_id();
        wait_stores();   // the wave's earlier output has reached the L2
        for (uint32_t r = 0; r < len; r += WAVE) {
            const uint32_t j = r + lane, k = off >= len ? j : j % off;
            const uint8_t x = j < len ? __builtin_amdgcn_raw_buffer_load_b8(Ro, (int)(op - off + k), 0, 17) : 0;
            if (j < len) __builtin_amdgcn_raw_buffer_store_b8(x, Ro, (int)(op + j), 0, 0);
        }
        return true;
    }
};

// A length extension (read_variable_length, lz4.c:1629-1649): bytes added up from p on while
// they are 255; stops after the byte that brings p to lim (hit: that happened).  Uniform.
template <class Mem>
__device__ __forceinline__ uint64_t length_ext(const Mem &m, uint32_t &p, uint32_t lim, bool &hit) {
    uint64_t sum = 0;
    hit = false;
    for (;;) {
        uint64_t t = m.rd(p);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t s = (uint32_t)t & 0xFF;
            t >>= 8;
            ++p;
            sum += s;
            if (p >= lim) { hit = true; return sum; }
            if (s != 255) return sum;
        }
    }
}

// The acceptance rule of include/rr_lz4.h (LZ4_decompress_generic, lz4.c:1658-2072; the tests
// carry the lines), on a raw block at input positions [ip, end) with announced length N > 0,
// end > ip.  Returns RR_LZ4_* or BAIL.  All uniform; positions are compared by sums (no
// subtraction below zero), lengths in 64 bits (an extension adds up to 255 a byte).
template <class Mem>
__device__ uint32_t lz4_walk(Mem &m, uint32_t ip, const uint32_t end, const uint32_t N) {
    uint32_t op = 0;
    bool fast = N >= FASTLOOP;   // lz4.c:1711
    for (;;) {
        const uint32_t token = (uint32_t)m.rd(ip) & 0xFF;   // lz4.c:1721 / 1849 (ip < end, see the end of the loop)
        ++ip;
        uint64_t L = token >> 4, M = token & 15;
        // the shortcuts that skip the end tests of a run: lz4.c:1751 (fast loop), 1863-1865
        const bool shrt = L != 15 && ip + 16 < end && (fast || op + 32 <= N);
        if (L == 15) {
            if (ip + 15 >= end) return RR_LZ4_E_TRUNC;   // initial check, lz4.c:1634 (1729 / 1898)
            bool hit;
            L += length_ext(m, ip, end - 15, hit);        // (reaching the limit is no error here, lz4.c:1730 / 1899)
        }
        if (fast && !shrt && ((token >> 4) != 15 || op + L + 32 > N || ip + L + 32 > end)) fast = false;   // lz4.c:1738, 1751
        if (!shrt && (op + L + MFLIMIT > N || ip + L + (2 + 1 + LASTLITERALS) > end)) {   // lz4.c:1910: the last run
            if (ip + L > end) return RR_LZ4_E_TRUNC;      // lz4.c:1945
            if (op + L > N) return RR_LZ4_E_OVERFLOW;
            if (ip + L != end) return op + L + MFLIMIT > N ? RR_LZ4_E_OVERFLOW : RR_LZ4_E_TRUNC;
            if (!m.literals(ip, op, (uint32_t)L)) return BAIL;
            return op + (uint32_t)L == N ? RR_LZ4_OK : RR_LZ4_E_LENGTH;   // (deviation: LZ4 returns the smaller count)
        }
        // (here ip + L + 2 <= end and op + L <= N: the run and the offset are inside the block)
        if (!m.literals(ip, op, (uint32_t)L)) return BAIL;
        ip += (uint32_t)L;
        op += (uint32_t)L;
        const uint32_t off = (uint32_t)m.rd(ip) & 0xFFFF;   // lz4.c:1764 / 1873 / 1963
        ip += 2;
        bool quick = shrt && M != 15 && off >= 8 && off <= op;   // lz4.c:1788-1798 / 1878-1888: no end test
        if (M == 15) {
            bool hit;
            M += length_ext(m, ip, end - LASTLITERALS + 1, hit);   // lz4.c:1774 / 1972 (end >= ip + 1 + 4 here? see below)
            if (hit) return RR_LZ4_E_TRUNC;
        }
        M += MINMATCH;
        if (off == 0) return RR_LZ4_E_OFFSET;             // (deviation: 1.9.2 copies garbage, lz4.c:2030-2031)
        if (off > op) return RR_LZ4_E_OFFSET;             // lz4.c:1773 / 1801 / 1981
        if (fast && op + M + FASTLOOP >= N) {             // lz4.c:1778 / 1783: the safe loop from here on
            fast = false;
            quick = false;
        }
        if (!fast && !quick && op + M + LASTLITERALS > N) return RR_LZ4_E_OVERFLOW;   // lz4.c:2047
        // (op + M <= N: the fast loop keeps 64 bytes, the shortcut 32 - 14 - 18, the test above 5)
        if (!m.match(op, off, (uint32_t)M, ip)) return BAIL;
        op += (uint32_t)M;
        // the next token is inside the block: after a tested run ip + 8 <= end before the offset,
        // after a shortcut ip + 1 <= end, after a match extension ip + 4 < end
    }
}

// The raw block of a stream whose preamble parsed: skip the preamble, the special cases of
// lz4.c:1701-1707, then the walk.
template <class Mem>
__device__ __forceinline__ uint32_t lz4_block(Mem &m, uint32_t s0, uint32_t end, uint32_t N) {
    uint32_t p = s0;
    {
        uint64_t t = m.rd(p);   // (validated by the length kernel: at most 5 bytes)
        while (t & 0x80) { ++p; t >>= 8; }
        ++p;
    }
    if (N == 0) return end - p == 1 && (m.rd(p) & 0xFF) == 0 ? RR_LZ4_OK : end == p ? RR_LZ4_E_TRUNC : RR_LZ4_E_OVERFLOW;
    if (end == p) return RR_LZ4_E_TRUNC;
    return lz4_walk(m, p, end, N);
}

__global__ __launch_bounds__(WAVE) void lz4_dec_kernel(const uint8_t *__restrict__ in, uint64_t in_cap,
                                                       const uint64_t *__restrict__ in_offs, uint64_t n,
                                                       uint8_t *__restrict__ out, uint64_t out_cap,
                                                       const uint64_t *__restrict__ out_offs,
                                                       uint8_t *__restrict__ status, uint32_t wcap) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    lds_u8 *win = (lds_u8 *)smem;
    lds_u32 *win32 = (lds_u32 *)win;
    const uint32_t lane = lane_id();
    for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {
        if (status[b] != RR_LZ4_OK) continue;   // (the preamble did not parse)
        const uint64_t o0 = out_offs[b], o1 = out_offs[b + 1];
        if (o1 > out_cap) {
            if (lane == 0) status[b] = RR_LZ4_E_CAPACITY;
            continue;
        }
        const uint32_t N = (uint32_t)(o1 - o0);
        const uint64_t c0 = in_offs[b], clen = in_offs[b + 1] - c0;
        const uint32_t s0 = (uint32_t)(c0 & 3), end = s0 + (uint32_t)clen;
        const uint64_t base = c0 - s0;   // (whole dwords: the buffer's padding, not past it)
        const uint64_t span = (s0 + clen + 15) & ~15ull;
        uint8_t *gout = out + o0;
        const rsrc_t Ro = mk_rsrc_clamped(gout, N);
        uint32_t st = BAIL;
        if (N <= wcap && span <= wcap) {
            // stage: the block's 16-byte granules at the window's end (the allocation's last
            // 32 bytes: reads past the end), eight loads a lane in flight
            const rsrc_t R = mk_rsrc_clamped(in + base, span < in_cap - base ? span : in_cap - base);
            const uint32_t ng = (uint32_t)(span >> 4), D = wcap + 16 - 16 * ng;
            lds_u32x4 *d4 = (lds_u32x4 *)(win + D);
            for (uint32_t j0 = 0; j0 < ng; j0 += 8 * WAVE) {
                u32x4_t g[8];
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j)
                    g[j] = __builtin_amdgcn_raw_buffer_load_b128(R, (int)(16 * (j0 + lane + WAVE * j)), 0, 0);
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j)
                    if (j0 + lane + WAVE * j < ng) d4[j0 + lane + WAVE * j] = g[j];
            }
            LdsMem m{win, D};
            st = lz4_block(m, s0, end, N);
            if (st == RR_LZ4_OK) {   // LDS -> output: bytes to a 4-aligned address, dwords, bytes
                const uint32_t g0 = (uint32_t)((uintptr_t)gout & 3), hh = min((4u - g0) & 3, N);
                const uint32_t t0 = hh + ((N - hh) & ~3u);
                if (lane < hh) __builtin_amdgcn_raw_buffer_store_b8(win[lane], Ro, (int)lane, 0, 0);
                for (uint32_t j = hh + 4 * lane; j < t0; j += 4 * WAVE) {
                    const uint32_t a = j >> 2;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_amdgcn_alignbyte(win32[a + 1], win32[a], j & 3), Ro, (int)j, 0, 0);
                }
                if (t0 + lane < N) __builtin_amdgcn_raw_buffer_store_b8(win[t0 + lane], Ro, (int)(t0 + lane), 0, 0);
            }
        }
        if (st == BAIL) {
            GlobalMem m{mk_rsrc_clamped(in + base, in_cap - base), Ro};
            st = lz4_block(m, s0, end, N);
        }
        if (lane == 0) status[b] = (uint8_t)st;
    }
}

// ---- compression ----------------------------------------------------------------------------

// The block's bytes in place, through its buffer resource (position k at R[g + k]).
struct Src {
    rsrc_t R;
    uint32_t g;
    __device__ __forceinline__ uint32_t ld32(uint32_t k) const {   // 4 bytes at k, per lane
        const uint32_t q = g + k, a = q & ~3u;
        const uint32_t lo = __builtin_amdgcn_raw_buffer_load_b32(R, (int)a, 0, 0);
        const uint32_t hi = __builtin_amdgcn_raw_buffer_load_b32(R, (int)a + 4, 0, 0);
        return __builtin_amdgcn_alignbyte(hi, lo, q & 3);
    }
    __device__ __forceinline__ uint32_t byte(uint32_t k) const {
        return __builtin_amdgcn_raw_buffer_load_b8(R, (int)(g + k), 0, 0);
    }
};

// Output slot writer: uniform op, lanes store.
struct Out {
    rsrc_t R;
    uint32_t op;
    uint32_t mis;   // the slot's address mod 4
    __device__ __forceinline__ void put(uint32_t nbytes, uint64_t v) {   // up to 8 bytes
        const uint32_t l = lane_id();
        if (l < nbytes) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(v >> (8 * l)), R, (int)(op + l), 0, 0);
        op += nbytes;
    }
    // the extension bytes of a length whose part past 15 is v: v / 255 bytes of 255, then v % 255
    __device__ __forceinline__ void ext(uint32_t v) {
        const uint32_t l = lane_id(), nb = v / 255 + 1;
        for (uint32_t i = l; i < nb; i += WAVE)
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(i + 1 < nb ? 255u : v % 255), R, (int)(op + i), 0, 0);
        op += nb;
    }
    // literal bytes: up to 64 a byte a lane; longer: a head to the first 4-aligned destination
    // byte, aligned dwords four a lane a round, a tail of < 4 bytes
    __device__ __forceinline__ void bytes(const Src &F, uint32_t from, uint32_t len) {
        const uint32_t l = lane_id();
        if (len <= WAVE) {
            if (l < len) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)F.byte(from + l), R, (int)(op + l), 0, 0);
            op += len;
            return;
        }
        const uint32_t h = (4u - ((mis + op) & 3u)) & 3u;
        const uint32_t nd = (len - h) >> 2, s = from + h, d = op + h, t = h + 4 * nd;
        const uint32_t hb = l < h ? F.byte(from + l) : 0u, tb = l < len - t ? F.byte(from + t + l) : 0u;
        for (uint32_t i = 0; i < nd; i += 4 * WAVE) {
            uint32_t v[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t k = i + j * WAVE + l;
                v[j] = k < nd ? F.ld32(s + 4 * k) : 0u;
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t k = i + j * WAVE + l;
                if (k < nd) __builtin_amdgcn_raw_buffer_store_b32(v[j], R, (int)(d + 4 * k), 0, 0);
            }
        }
        if (l < h) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)hb, R, (int)(op + l), 0, 0);
        if (l < len - t) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)tb, R, (int)(op + t + l), 0, 0);
        op += len;
    }
    // one sequence: lit literals from `from`, then (ml != 0) a match of ml bytes at offset off
    __device__ __forceinline__ void sequence(const Src &F, uint32_t from, uint32_t lit, uint32_t off, uint32_t ml) {
        const uint32_t mc = ml ? ml - MINMATCH : 0u;
        put(1, ((lit < 15 ? lit : 15u) << 4) | (mc < 15 ? mc : 15u));
        if (lit >= 15) ext(lit - 15);
        if (lit) bytes(F, from, lit);
        if (ml) {
            put(2, off);
            if (mc >= 15) ext(mc - 15);
        }
    }
};

// bytes equal at a + i and b + i (a < b), for b + i < lim; 64 lanes a step
__device__ __forceinline__ uint32_t match_len(const Src &F, uint32_t a, uint32_t b, uint32_t lim) {
    const uint32_t l = lane_id();
    for (uint32_t m = 0;; m += WAVE) {
        const uint32_t k = m + l;
        const bool stop = b + k >= lim || F.byte(a + k) != F.byte(b + k);
        const uint64_t bal = __ballot(stop);
        if (bal) return m + (uint32_t)__builtin_ctzll(bal);
    }
}

__device__ __forceinline__ uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - HLOG); }

// table[h] = the largest of the positions the lanes with `ins` hold for h (all above what the
// table holds from earlier rounds).  Lanes with the same hash store to the same entry and one
// of them lands; whichever it is, the lanes that hold a larger position store again, so the
// result is the maximum and does not depend on which store the hardware lets win.  Each pass
// raises every contested entry: at most 64 passes.
__device__ __forceinline__ void insert(lds_u16 *tab, bool ins, uint32_t h, uint32_t pos) {
    for (;;) {
        const uint32_t cur = ins ? (uint32_t)tab[h] : 0u;
        ins = ins && cur < pos;
        if (!__ballot(ins)) return;
        if (ins) tab[h] = (uint16_t)pos;
    }
}

// first[h] = the smallest of the words (position << 16 | 16 hash bits) the lanes with `ins` hold
// for h, where the entry is still empty (0: the caller keeps the chunk's first position and every
// other one with its hash out of `ins`, so that entry stays 0 and stands for it).  Positions
// grow from round to round, so an entry is written in one round only; inside it the lanes that
// hold a smaller position than the one that landed store again: the result is the minimum
// whichever store the hardware lets win.  At most 64 passes.
__device__ __forceinline__ void insert_first(lds_u32 *first, bool ins, uint32_t h, uint32_t word, uint32_t round0) {
    for (;;) {
        const uint32_t cur = ins ? first[h] : 0u;
        ins = ins && (cur == 0 || ((cur >> 16) >= round0 && cur > word));   // (round0: this round's first position)
        if (!__ballot(ins)) return;
        if (ins) first[h] = word;
    }
}

__global__ __launch_bounds__(WAVE) void lz4_comp_kernel(const uint8_t *__restrict__ in, uint64_t in_cap,
                                                        const uint64_t *__restrict__ in_offs, uint64_t n,
                                                        uint8_t *__restrict__ slots,
                                                        const uint64_t *__restrict__ slot_offs,
                                                        uint64_t *__restrict__ sizes) {
    __shared__ uint16_t tab_mem[HSIZE];
    __shared__ uint32_t first_mem[FSIZE];
    lds_u16 *tab = (lds_u16 *)tab_mem;
    lds_u32 *first = (lds_u32 *)first_mem;
    const uint32_t lane = lane_id();
    for (uint64_t b = blockIdx.x; b < n; b += gridDim.x) {
        const uint64_t c0 = in_offs[b];
        const uint32_t len = (uint32_t)(in_offs[b + 1] - c0);
        const uint32_t s0 = (uint32_t)(c0 & 3);
        const uint64_t base = c0 - s0;
        const Src F{mk_rsrc_clamped(in + base, in_cap - base), s0};
        Out O;
        O.R = mk_rsrc_clamped(slots + slot_offs[b], slot_offs[b + 1] - slot_offs[b]);
        O.op = 0;
        O.mis = (uint32_t)((uintptr_t)(slots + slot_offs[b]) & 3u);
        {   // varint32 length
            uint32_t v = len, nb = 1;
            uint64_t enc = 0;
            for (uint32_t k = 0; k < 5; ++k) {
                const uint32_t more = v >= 128;
                enc |= (uint64_t)((v & 0x7F) | (more << 7)) << (8 * k);
                if (!more) { nb = k + 1; break; }
                v >>= 7;
            }
            O.put(nb, enc);
        }
        uint32_t anchor = 0;
        if (len > MFLIMIT) {
            // a match starts at or before mfl (12 bytes before the end) and ends at or before
            // mlim (the last 5 bytes are literals): lz4_Block_format.md, end of block restrictions
            const uint32_t mfl = len - MFLIMIT, mlim = len - LASTLITERALS;
            uint32_t ip = 0, cb = 0;   // cb: the chunk's first position (table entries are relative to it)
            uint32_t h0 = 0;           // first's hash at cb: first[h0] stays 0, which stands for cb
            bool fresh = true;
            while (ip <= mfl) {
                if (fresh || ip - cb >= CHUNK) {   // a new 64 KiB chunk: its own table; pending literals carry over
                    cb = ip;
                    for (uint32_t k = lane; k < HSIZE / 2; k += WAVE) ((lds_u32 *)tab)[k] = 0;
                    for (uint32_t k = lane; k < FSIZE; k += WAVE) first[k] = 0;
                    fresh = false;
                }
                const uint32_t P = ip + lane;
                const bool valid = P <= mfl && P - cb < CHUNK;
                const uint32_t x = F.ld32(valid ? P : 0u), h = hash4(x);
                // the latest position with this hash; where that is no match, the chunk's first one
                // (a repeat from far back, which later positions have pushed out of tab), read
                // only where the entry's 16 hash bits agree
                const uint32_t hv = x * 2654435761u, hf = hv >> (32 - FLOG), tag = (hv >> (16 - FLOG)) & 0xFFFFu;
                if (ip == cb) h0 = rl32(hf, 0);
                const uint32_t c1 = cb + (valid ? (uint32_t)tab[h] : 0u);   // (an empty entry reads as the chunk's first position)
                const uint32_t e = valid ? first[hf] : 0u, c2 = cb + (e >> 16);
                const bool hit1 = valid && c1 < P && F.ld32(c1) == x;
                const bool may2 = valid && !hit1 && c2 != c1 && c2 < P && (e ? (e & 0xFFFFu) == tag : hf == h0);
                const bool hit = hit1 || (may2 && F.ld32(c2) == x);
                const uint32_t c = hit1 ? c1 : c2;
                const uint64_t bal = __ballot(hit);
                const uint32_t sl = bal ? (uint32_t)__builtin_ctzll(bal) : WAVE;
                insert(tab, valid && lane <= sl, h, P - cb);
                if (ip - cb < 4 * FSIZE)   // (after four positions an entry the table is full but for 2 %)
                    insert_first(first, valid && lane <= sl && hf != h0, hf, ((P - cb) << 16) | tag, ip - cb);
                if (!bal) {
                    ip += WAVE;
                    continue;
                }
                const uint32_t ms = ip + sl, mc = rl32(c, sl);
                const uint32_t ml = MINMATCH + match_len(F, mc + MINMATCH, ms + MINMATCH, mlim);
                O.sequence(F, anchor, ms - anchor, ms - mc, ml);
                ip = ms + ml;
                anchor = ip;
            }
        }
        O.sequence(F, anchor, len - anchor, 0, 0);   // the last run (a block below 13 bytes: the only one)
        if (lane == 0) sizes[b] = O.op;
    }
}

// slot sizes (rr_lz4_max_compressed_length per block); zeroes both scans' look-back words and the
// two arrays' last entries
__global__ __launch_bounds__(256) void lz4_bound_kernel(const uint64_t *__restrict__ in_offs, uint64_t n,
                                                        uint64_t *__restrict__ slot_offs, uint64_t *__restrict__ sizes,
                                                        uint64_t *__restrict__ lb, uint32_t lbw2) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < lbw2) lb[i] = 0;
    if (i < n) {
        const uint64_t len = in_offs[i + 1] - in_offs[i];
        slot_offs[i] = 5 + len + len / 255 + 16;
    } else if (i == n) {
        slot_offs[n] = 0;
        sizes[n] = 0;
    }
}

uint32_t grid_for(uint64_t n, uint32_t cap) { return (uint32_t)(n < cap ? (n ? n : 1) : cap); }
constexpr uint32_t GRID_CAP = 1u << 16;   // workgroups a launch; the blocks past it by the grid-stride loops

// RR_LZ4_DEC_WINDOW (environment, read at each call; tests): the window bytes the decompressor
// uses, at most the compiled RR_LZ4_DEC_WIN; 0 sends every block down the global path
uint32_t dec_window() {
    const char *e = getenv("RR_LZ4_DEC_WINDOW");
    if (!e || !*e) return LZ4_DEC_WIN;
    const unsigned long v = strtoul(e, nullptr, 10) & ~15ul;
    return v < LZ4_DEC_WIN ? (uint32_t)v : LZ4_DEC_WIN;
}

}  // namespace

// scratch: two scans' look-back words, the error word, slot offsets, the slots
extern "C" uint64_t rr_lz4_scratch_words(uint64_t n, uint64_t slot_bytes) {
    return 2 * rr_scan_words(n) + 1 + (n + 1) + (slot_bytes + 7) / 8 + 2;
}

// decompression: 3 launches (length preambles, scan, blocks)
extern "C" hipError_t rr_launch_lz4_decompress(const uint8_t *in, uint64_t in_cap, const uint64_t *in_offs, uint64_t n, uint8_t *out,
                                               uint64_t out_cap, uint64_t *out_offs, uint8_t *status, uint64_t *scratch,
                                               hipStream_t stream) {
    const uint64_t lbw = rr_scan_words(n);
    uint64_t *lb = scratch, *err = scratch + 2 * lbw;
    hipError_t e = rr_launch_varint_lengths(in, in_offs, n, out_offs, status, lb, lbw, stream);
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(out_offs, n, lb, err, stream);
    if (e != hipSuccess || n == 0) return e != hipSuccess ? e : hipGetLastError();
    hipLaunchKernelGGL(lz4_dec_kernel, dim3(grid_for(n, GRID_CAP)), dim3(WAVE), LZ4_DEC_WIN + 48, stream, in, in_cap, in_offs, n, out,
                       out_cap, (const uint64_t *)out_offs, status, dec_window());
    return hipGetLastError();
}

// compression: bounds + scan -> per-block slots in scratch, blocks, scan of the sizes, pack
extern "C" hipError_t rr_launch_lz4_compress(const uint8_t *in, uint64_t in_cap, const uint64_t *in_offs, uint64_t n, uint8_t *out,
                                             uint64_t *out_offs, uint64_t *scratch, uint64_t slot_bytes, hipStream_t stream) {
    const uint64_t lbw = rr_scan_words(n);
    uint64_t *lb = scratch, *lb2 = scratch + lbw, *err = scratch + 2 * lbw, *slot_offs = err + 1;
    uint8_t *slots = reinterpret_cast<uint8_t *>(slot_offs + n + 1);
    (void)slot_bytes;
    const uint64_t m = (n + 1 > 2 * lbw ? n + 1 : 2 * lbw);
    hipLaunchKernelGGL(lz4_bound_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, stream, in_offs, n, slot_offs, out_offs, lb,
                       (uint32_t)(2 * lbw));
    hipError_t e = rr_launch_scan_u64(slot_offs, n, lb, err, stream);
    if (e != hipSuccess) return e;
    if (n) hipLaunchKernelGGL(lz4_comp_kernel, dim3(grid_for(n, GRID_CAP)), dim3(WAVE), 0, stream, in, in_cap, in_offs, n, slots,
                              (const uint64_t *)slot_offs, out_offs);
    e = rr_launch_scan_u64(out_offs, n, lb2, err, stream);
    if (e != hipSuccess || n == 0) return e != hipSuccess ? e : hipGetLastError();
    return rr_launch_slot_pack(slots, slot_offs, n, out, out_offs, stream);
}
