// rr_rdbfile.hip — gfx950 kernels of include/rr_rdbfile.h: the RDB stream framing around
// rr_rdbsave_batch's payloads (rdbSaveKeyValuePair, rdb.c:1017-1073; the EOF and checksum of
// rdbSaveRio :1249-1255), DUMP payloads and their verification (cluster.c:4817-4867), and the
// CRC-64 (crc64.c:1-12) all of them carry.
//
// The CRC.  init 0 and no final xor make it linear, so zero bytes in front of a run with state 0
// change nothing and every piece's value can be computed alone.  A stream of N bytes is cut into
// pieces of PIECE bytes counted from its END: piece q is [N - (q + 1) * PIECE, N - q * PIECE), and
// only the first one (the highest q) can be short; it is treated as a full piece with zero bytes in
// front.  Inside a piece lane l takes the RUN bytes [l * RUN, (l + 1) * RUN) (slice-by-8 over eight
// 256-entry u64 tables in LDS, which every workgroup generates from the polynomial when it starts),
// multiplies its value by the constant x^(8 * RUN * (63 - l)) mod P and the wave xors the lanes.
// The incoming checksum is the initial state of the lane that owns the stream's first byte, so no
// shift by a run-time length exists anywhere: every combine is a product with a constant, a 64-step
// shift / xor loop (gfx950 has no carry-less multiply).
//   crc_stream_kernel: wave w of W takes the pieces q = w, w + W, ... from the highest down,
//     acc = acc * x^(8 * PIECE * W) ^ piece, and leaves acc in part[w].
//   crc_finish_kernel (one wave): sum over w of part[w] * x^(8 * PIECE * w), by Horner over
//     MAX_WAVES / 64 words a lane and one constant a lane; writes the state and the EOF checksum.
//   wave_crc: the same for one value's bytes by one wave (rdbdump_emit_kernel, rdbdump_check_kernel).
//
// The section.  file_size_kernel (a record a lane: status, size), rr_launch_scan_u64 over
// head_bytes | sizes, file_emit_kernel (a record a lane for the header; the key and the payload are
// copy_bodies'), then the two CRC kernels over the assembled bytes.  A section that does not fit
// out_cap is not written at all.  The shape is rr_stage_device.h's, with loops of its own: a record
// a lane, y[] one word ahead of the records (head_bytes in front), and the calls report through
// rr_rdbfile_result, not rr_totals.  The leaves are the shared ones.
#include <hip/hip_runtime.h>

#include "rr_rdb_device.h"
#include "rr_stage_device.h"
#include "../../include/rr_rdbfile.h"

using namespace rr;

namespace {

constexpr uint32_t WPB = 4;                       // waves per workgroup
constexpr uint32_t RUN = RR_CRC64_RUN, PIECE = RR_CRC64_PIECE;
constexpr uint32_t MAX_WAVES = RR_CRC64_MAX_WAVES, PER_LANE = MAX_WAVES / RR_WAVE;
constexpr uint32_t DUMP_GRID = RR_RDBDUMP_MAX_WAVES / WPB;
constexpr uint32_t REC_GRID_CAP = 4096;           // workgroups of the section's size and emit kernels
constexpr uint64_t POLY = 0x95ac9329ac4bc9b5ull;  // 0xad93d23594c935a9 reflected
constexpr uint64_t ONE = 1ull << 63;              // x^0 in the reflected bit order
static_assert(PIECE == RR_WAVE * RUN && MAX_WAVES % RR_WAVE == 0 && RUN % 8 == 0, "a lane a run");

// ---- GF(2)[x] mod P, reflected: bit 63 - i is the coefficient of x^i --------------------------
__host__ __device__ constexpr uint64_t gf_mulx(uint64_t a) { return (a >> 1) ^ (POLY & (0ull - (a & 1))); }
__host__ __device__ constexpr uint64_t gf_mul(uint64_t a, uint64_t b) {
    uint64_t r = 0;
    for (int i = 0; i < 64; ++i) {
        r ^= a & (0ull - (b >> 63));
        b <<= 1;
        a = gf_mulx(a);
    }
    return r;
}
// x^(8 * nbytes) mod P by square-and-multiply (build time and the launchers only)
__host__ __device__ constexpr uint64_t gf_xpow8(uint64_t nbytes) {
    uint64_t r = ONE, sq = ONE;
    for (int i = 0; i < 8; ++i) sq = gf_mulx(sq);   // x^8
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1) r = gf_mul(r, sq);
        sq = gf_mul(sq, sq);
    }
    return r;
}
struct LaneK { uint64_t k[RR_WAVE]; };
constexpr LaneK make_run_k() {      // lane l: x^(8 * RUN * (63 - l))
    LaneK t{};
    const uint64_t xr = gf_xpow8(RUN);
    uint64_t v = ONE;
    for (int l = RR_WAVE - 1; l >= 0; --l) { t.k[l] = v; v = gf_mul(v, xr); }
    return t;
}
constexpr LaneK make_part_k() {     // lane l: x^(8 * PIECE * PER_LANE * l)
    LaneK t{};
    const uint64_t xs = gf_xpow8((uint64_t)PIECE * PER_LANE);
    uint64_t v = ONE;
    for (uint32_t l = 0; l < RR_WAVE; ++l) { t.k[l] = v; v = gf_mul(v, xs); }
    return t;
}
__device__ const LaneK RUN_K = make_run_k();
__device__ const LaneK PART_K = make_part_k();
constexpr uint64_t X_PIECE = gf_xpow8(PIECE);

__device__ __forceinline__ uint64_t wave_xor(uint64_t x) {
#pragma unroll
    for (int d = RR_WAVE / 2; d > 0; d >>= 1) x ^= __shfl_xor(x, d, RR_WAVE);
    return x;
}

// ---- the tables: T[k][b] = the state after byte b and k zero bytes, from state 0 ---------------
// Every thread of the workgroup (WPB * 64 = 256 threads: an entry of each table a thread).
__device__ __forceinline__ lds_u64 *crc_tables() {
    __shared__ uint64_t tab[8 * 256];
    lds_u64 *T = (lds_u64 *)tab;
    const uint32_t b = threadIdx.x;
    uint64_t c = b;
    for (int i = 0; i < 8; ++i) c = gf_mulx(c);
    T[b] = c;
    __syncthreads();
    for (uint32_t k = 1; k < 8; ++k) {
        c = T[c & 0xFF] ^ (c >> 8);
        T[k * 256 + b] = c;
    }
    __syncthreads();
    return T;
}
__device__ __forceinline__ uint64_t crc_byte(const lds_u64 *T, uint64_t c, uint32_t b) { return T[(uint32_t)(c ^ b) & 0xFF] ^ (c >> 8); }
__device__ __forceinline__ uint64_t crc_word(const lds_u64 *T, uint64_t c, uint64_t w) {
    c ^= w;
    const uint32_t lo = (uint32_t)c, hi = (uint32_t)(c >> 32);
    return T[7 * 256 + (lo & 0xFF)] ^ T[6 * 256 + ((lo >> 8) & 0xFF)] ^ T[5 * 256 + ((lo >> 16) & 0xFF)] ^ T[4 * 256 + (lo >> 24)] ^
           T[3 * 256 + (hi & 0xFF)] ^ T[2 * 256 + ((hi >> 8) & 0xFF)] ^ T[1 * 256 + ((hi >> 16) & 0xFF)] ^ T[hi >> 24];
}

// A lane's run: n <= RUN bytes at p, from state c.  Bytes up to an 8-byte boundary, words (four
// loads in flight), the tail bytes.  Reads [p, p + n) only.
__device__ __forceinline__ uint64_t crc_run(const lds_u64 *T, uint64_t c, const uint8_t *__restrict__ p, uint32_t n) {
    uint32_t h = (uint32_t)(0 - (uintptr_t)p) & 7;
    if (h > n) h = n;
    n -= h;
    for (; h; --h) c = crc_byte(T, c, *p++);
    const uint64_t *w = reinterpret_cast<const uint64_t *>(p);
    for (; n >= 32; n -= 32, w += 4) {
        const uint64_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
        c = crc_word(T, c, w0);
        c = crc_word(T, c, w1);
        c = crc_word(T, c, w2);
        c = crc_word(T, c, w3);
    }
    for (; n >= 8; n -= 8) c = crc_word(T, c, *w++);
    p = reinterpret_cast<const uint8_t *>(w);
    for (; n; --n) c = crc_byte(T, c, *p++);
    return c;
}

// One piece by the whole wave: the len <= PIECE bytes at p (wave-uniform), as the END of a full
// piece.  first: the piece starts the stream, and init is the state in front of its first byte.
// Returns crc(first ? init : 0, p[0, len)) in every lane.
__device__ __forceinline__ uint64_t crc_piece(const lds_u64 *T, const uint8_t *__restrict__ p, uint32_t len, bool first, uint64_t init) {
    const uint32_t lane = lane_id(), pad = PIECE - len;
    const uint32_t v0 = lane * RUN, v1 = v0 + RUN;     // the lane's bytes of the full piece
    uint64_t c = 0;
    if (v1 > pad) {
        const uint32_t s = v0 > pad ? v0 - pad : 0;    // its first real byte
        if (first && s == 0) c = init;
        c = crc_run(T, c, p + s, v1 - pad - s);
    }
    if (__ballot(c != 0 && lane != RR_WAVE - 1)) c = gf_mul(c, RUN_K.k[lane]);   // (lane 63's constant is 1)
    return wave_xor(c);
}

// crc(init, p[0, len)) by one wave, len > 0 (wave-uniform arguments)
__device__ __forceinline__ uint64_t wave_crc(const lds_u64 *T, const uint8_t *__restrict__ p, uint64_t len, uint64_t init) {
    const uint64_t np = (len + PIECE - 1) / PIECE;
    const uint32_t flen = (uint32_t)(len - (np - 1) * PIECE);   // the first piece
    uint64_t acc = crc_piece(T, p, flen, true, init);
    p += flen;
    for (uint64_t q = 1; q < np; ++q, p += PIECE) acc = gf_mul(acc, X_PIECE) ^ crc_piece(T, p, PIECE, false, 0);
    return acc;
}

// ---- the stream pass -----------------------------------------------------------------------------
// N = (n_ptr ? *n_ptr : 0) + n_add bytes at data; nothing is done when N + cap_add > cap (the section
// does not fit) or off (RR_RDBFILE_NO_CKSUM).  x_stride = x^(8 * PIECE * W), W the launch's waves.
__global__ __launch_bounds__(WPB * RR_WAVE) void crc_stream_kernel(const uint8_t *__restrict__ data, const uint64_t *n_ptr,
                                                                   uint64_t n_add, uint64_t cap_add, uint64_t cap,
                                                                   const uint64_t *__restrict__ state, uint64_t x_stride,
                                                                   uint64_t *__restrict__ part, int off) {
    const lds_u64 *T = crc_tables();
    const uint64_t W = (uint64_t)gridDim.x * WPB, w = (uint64_t)blockIdx.x * WPB + threadIdx.x / RR_WAVE;
    const uint64_t N = (n_ptr ? first64(*n_ptr) : 0) + n_add;
    uint64_t acc = 0;
    if (!off && N + cap_add <= cap && N) {
        const uint64_t np = (N + PIECE - 1) / PIECE;
        const uint64_t init = first64(state[0]);
        if (w < np) {
            uint64_t q = w + (np - 1 - w) / W * W;      // the wave's highest piece
            for (;; q -= W) {
                const bool first = q == np - 1;
                const uint64_t end = N - q * PIECE;     // the piece is [end - len, end)
                const uint32_t len = first ? (uint32_t)(N - (np - 1) * PIECE) : PIECE;
                const uint64_t c = crc_piece(T, data + end - len, len, first, init);
                acc = acc ? gf_mul(acc, x_stride) ^ c : c;
                if (q < W) break;
            }
        }
    }
    if (lane_id() == 0) part[w] = acc;
}

// One wave: the parts of the W waves into the new state; the EOF checksum.  eof_at: where the
// checksum's 8 bytes go, relative to the stream's end (RR_RDBFILE_EOF), when out != NULL.
__global__ __launch_bounds__(RR_WAVE) void crc_finish_kernel(const uint64_t *n_ptr, uint64_t n_add, uint64_t cap_add, uint64_t cap,
                                                             uint64_t *state, const uint64_t *__restrict__ part, uint32_t W, int off,
                                                             uint8_t *out, const uint64_t *err, rr_rdbfile_result *result) {
    const uint32_t lane = lane_id();
    const uint64_t N = (n_ptr ? first64(*n_ptr) : 0) + n_add, need = N + cap_add;
    const bool fits = need <= cap;
    uint64_t c = first64(state[0]);
    if (!off && fits && N) {
        uint64_t a = 0;                                  // Horner over the lane's words, highest first
        for (uint32_t j = PER_LANE; j-- > 0;) {
            const uint32_t w = lane * PER_LANE + j;
            const uint64_t x = w < W ? part[w] : 0;
            a = a ? gf_mul(a, X_PIECE) ^ x : x;
        }
        if (__ballot(a != 0 && lane != 0)) a = gf_mul(a, PART_K.k[lane]);
        c = wave_xor(a);
    }
    if (lane == 0) {
        if (fits) {
            state[0] = c;
            if (out)
                for (uint32_t k = 0; k < 8; ++k) out[N + k] = (uint8_t)(c >> (8 * k));
        }
        state[1] = need;
        if (result && err && *err) result->bytes = ~0ull;
    }
}

// ---- the section ---------------------------------------------------------------------------------
struct Sec {
    const uint8_t *pay;  const uint64_t *pay_offs;  uint64_t pay_cap;
    const uint8_t *key;  const uint64_t *key_offs;  uint64_t key_cap;
    const uint8_t *types, *status;
    const int64_t *expires;  const uint64_t *idle;  const uint8_t *freq;
    const uint8_t *head;  uint64_t head_bytes;
    uint64_t n;
    uint32_t flags;
};

// y[0] = head_bytes, y[1 + i] = record i's size, y[n + 1] = 0 (the scan's total); rec_status; and
// the stage's zeroing
__global__ __launch_bounds__(WPB * RR_WAVE) void file_size_kernel(Sec S, uint64_t *__restrict__ y, uint8_t *__restrict__ rec_status,
                                                                  uint64_t *__restrict__ zero, uint64_t nzero,
                                                                  rr_rdbfile_result *result) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    zero_stage_words(gtid, nthreads, zero, nzero, &y[S.n + 1], result);
    if (gtid == 0) y[0] = S.head_bytes;
    for (uint64_t i = gtid; i < S.n; i += nthreads) {
        uint32_t st = RR_OK;
        uint64_t size = 0;
        const uint64_t p0 = S.pay_offs[i], p1 = S.pay_offs[i + 1], k0 = S.key_offs[i], k1 = S.key_offs[i + 1];
        if (S.status[i] != 0 || !slice_ok(p0, p1, S.pay_cap)) st = RR_RDBFILE_E_VALUE;
        else if (!slice_ok(k0, k1, S.key_cap)) st = RR_RDBFILE_E_KEY;
        else {
            const uint32_t kl = (uint32_t)(k1 - k0);
            int64_t iv;
            size = 1 + (p1 - p0) + (raw_is_int(S.key + k0, kl, iv) ? rint_bytes(iv) : len_bytes(kl) + kl);
            if (S.expires && S.expires[i] != -1) size += 9;
            if (S.flags & RR_RDBFILE_IDLE) size += 1 + len_bytes(S.idle[i]);
            if (S.flags & RR_RDBFILE_FREQ) size += 2;
        }
        y[1 + i] = size;
        rec_status[i] = (uint8_t)st;
    }
}

// y scanned: y[1 + i] record i's start, y[n + 1] the end of the last one.
__global__ __launch_bounds__(WPB * RR_WAVE) void file_emit_kernel(Sec S, const uint64_t *__restrict__ y,
                                                                  const uint8_t *__restrict__ rec_status, uint8_t *out, uint64_t out_cap,
                                                                  uint64_t *__restrict__ rec_offsets, const uint64_t *err,
                                                                  rr_rdbfile_result *result) {
    const uint32_t lane = lane_id();
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = (uint64_t)gridDim.x * WPB, wave = first64(gtid / RR_WAVE);
    const uint64_t end = first64(y[S.n + 1]), need = end + ((S.flags & RR_RDBFILE_EOF) ? 9 : 0);
    const bool fits = need <= out_cap;
    if (gtid == 0) {
        result->bytes = *err ? ~0ull : need;
        result->status = fits ? RR_OK : RR_E_CAPACITY;
        rec_offsets[S.n] = end;
        if (fits && (S.flags & RR_RDBFILE_EOF)) out[end] = 0xFF;   // rdb.c:1249
    }
    if (wave == 0 && fits && S.head_bytes) {
        for (uint64_t k = 0; k < S.head_bytes; k += 1u << 30) {
            const uint64_t m = S.head_bytes - k;
            wave_copy(out + k, S.head + k, (uint32_t)(m < (1u << 30) ? m : 1u << 30));
        }
    }
    uint64_t n_bad = 0;
    for (uint64_t base = wave * RR_WAVE; base < S.n; base += nwaves * RR_WAVE) {
        const uint64_t i = base + lane;
        const bool live = i < S.n;
        const uint32_t st = live ? rec_status[i] : 1u;
        if (live) {
            rec_offsets[i] = y[1 + i];
            n_bad += st != 0;
        }
        if (!fits) continue;
        const bool mine = live && st == 0;
        uint8_t *d = out, *kd = out, *pd = out;
        const uint8_t *ks = S.key, *ps = S.pay;
        uint32_t kl = 0, pl = 0;
        if (mine) {
            d += y[1 + i];
            const int64_t ex = S.expires ? S.expires[i] : -1;
            if (ex != -1) {                                    // rdb.c:1030-1034, :115-119
                d[0] = 0xFC;
                put_le(d + 1, (uint64_t)ex, 8);
                d += 9;
            }
            if (S.flags & RR_RDBFILE_IDLE) {                   // :1037-1042
                d[0] = 0xF8;
                d += 1 + put_len(d + 1, S.idle[i]);
            }
            if (S.flags & RR_RDBFILE_FREQ) {                   // :1045-1054
                d[0] = 0xF9;
                d[1] = S.freq[i];
                d += 2;
            }
            *d++ = S.types[i];                                 // :1057
            const uint64_t k0 = S.key_offs[i], p0 = S.pay_offs[i];
            kl = (uint32_t)(S.key_offs[i + 1] - k0);
            pl = (uint32_t)(S.pay_offs[i + 1] - p0);
            ks += k0;
            ps += p0;
            int64_t iv;
            if (raw_is_int(ks, kl, iv)) {                      // rdbSaveRawString, :416-422
                const uint32_t nb = rint_bytes(iv) - 1;
                d[0] = (uint8_t)(0xC0 | (nb == 1 ? 0 : nb == 2 ? 1 : 2));
                put_le(d + 1, (uint64_t)iv, nb);
                d += 1 + nb;
                kl = 0;
            } else {
                d += put_len(d, kl);
            }
            kd = d;
            pd = d + kl;
        }
        copy_bodies(kd, ks, kl, mine);
        copy_bodies(pd, ps, pl, mine);
    }
    n_bad = wave_sum(n_bad);
    if (lane == 0 && n_bad) atomicAdd((unsigned long long *)&result->n_bad, (unsigned long long)n_bad);
}

// ---- DUMP payloads ------------------------------------------------------------------------------
__global__ __launch_bounds__(WPB * RR_WAVE) void dump_size_kernel(const uint64_t *__restrict__ in_offs, uint64_t in_cap,
                                                                  const uint8_t *__restrict__ status, uint64_t n,
                                                                  uint64_t *__restrict__ out_offs, uint8_t *__restrict__ out_status,
                                                                  uint64_t *__restrict__ zero, uint64_t nzero, rr_rdbfile_result *result) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    zero_stage_words(gtid, nthreads, zero, nzero, &out_offs[n], result);
    for (uint64_t i = gtid; i < n; i += nthreads) {
        const uint64_t o0 = in_offs[i], o1 = in_offs[i + 1];
        const bool ok = status[i] == 0 && slice_ok(o0, o1, in_cap);
        out_offs[i] = ok ? o1 - o0 + 11 : 0;
        out_status[i] = ok ? RR_OK : RR_RDBFILE_E_VALUE;
    }
}

// A wave a value: type | payload | 09 00 | crc.  The CRC is taken over the source bytes: the type
// byte is the state in front of the payload, the footer two byte steps behind it.
__global__ __launch_bounds__(WPB * RR_WAVE) void dump_emit_kernel(const uint8_t *__restrict__ data, const uint64_t *__restrict__ in_offs,
                                                                  const uint8_t *__restrict__ types, uint64_t n,
                                                                  const uint64_t *__restrict__ out_offs, uint8_t *out, uint64_t out_cap,
                                                                  uint8_t *out_status, const uint64_t *err, rr_rdbfile_result *result) {
    const lds_u64 *T = crc_tables();
    const uint32_t lane = lane_id();
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = (uint64_t)gridDim.x * WPB;
    if (gtid == 0) result->bytes = *err ? ~0ull : out_offs[n];
    uint64_t n_bad = 0;   // wave-uniform
    for (uint64_t v = first64(gtid / RR_WAVE); v < n; v += nwaves) {
        if (rfl(out_status[v])) { ++n_bad; continue; }
        const uint64_t b0 = first64(out_offs[v]), b1 = first64(out_offs[v + 1]);
        if (b1 > out_cap) {
            ++n_bad;
            if (lane == 0) out_status[v] = RR_E_CAPACITY;
            continue;
        }
        const uint64_t o0 = first64(in_offs[v]);
        const uint32_t len = (uint32_t)(b1 - b0 - 11), type = rfl(types[v]);
        uint64_t c = T[type];                                  // the state after the type byte
        if (len) {
            wave_copy(out + b0 + 1, data + o0, len);
            c = wave_crc(T, data + o0, len, c);
        }
        c = crc_byte(T, crc_byte(T, c, RR_RDB_VERSION & 0xFF), RR_RDB_VERSION >> 8);
        if (lane == 0) {
            uint8_t *d = out + b0;
            d[0] = (uint8_t)type;
            d[1 + len] = RR_RDB_VERSION & 0xFF;                // cluster.c:4831-4834
            d[2 + len] = RR_RDB_VERSION >> 8;
            put_le(d + 3 + len, c, 8);                         // :4837-4840
        }
    }
    if (lane == 0 && n_bad) atomicAdd((unsigned long long *)&result->n_bad, (unsigned long long)n_bad);
}

// verifyDumpPayload (cluster.c:4850-4867) a wave a value: status, the type byte, the payload's size
__global__ __launch_bounds__(WPB * RR_WAVE) void dump_check_kernel(const uint8_t *__restrict__ data, uint64_t in_cap,
                                                                   const uint64_t *__restrict__ in_offs, uint64_t n,
                                                                   uint64_t *__restrict__ out_offs, uint8_t *__restrict__ types,
                                                                   uint8_t *__restrict__ status, uint64_t *__restrict__ zero, uint64_t nzero,
                                                                   rr_rdbfile_result *result) {
    const lds_u64 *T = crc_tables();
    const uint32_t lane = lane_id();
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    zero_stage_words(gtid, nthreads, zero, nzero, &out_offs[n], result);
    const uint64_t nwaves = nthreads / RR_WAVE;
    for (uint64_t v = first64(gtid / RR_WAVE); v < n; v += nwaves) {
        const uint64_t o0 = first64(in_offs[v]), o1 = first64(in_offs[v + 1]);
        uint32_t st = RR_OK, type = 0;
        uint64_t size = 0;
        if (!slice_ok(o0, o1, in_cap)) st = RR_RDBDUMP_E_SHORT;
        else {
            const uint64_t L = o1 - o0;
            const uint8_t *p = data + o0;
            if (L) type = rfl(p[0]);
            if (L < 11) st = RR_RDBDUMP_E_SHORT;               // :4856 (10 there)
            else {
                const uint32_t f = lane < 10 ? (uint32_t)p[L - 10 + lane] : 0u;   // the footer, a byte a lane
                const uint32_t ver = rl32(f, 0) | (rl32(f, 1) << 8);
                uint64_t want = 0;
                for (uint32_t k = 0; k < 8; ++k) want |= (uint64_t)rl32(f, 2 + k) << (8 * k);
                if (ver > RR_RDB_VERSION) st = RR_RDBDUMP_E_VERSION;              // :4860-4861
                else if (wave_crc(T, p, L - 8, 0) != want) st = RR_RDBDUMP_E_CRC; // :4864-4866
                else size = L - 11;
            }
        }
        if (lane == 0) {
            out_offs[v] = size;
            types[v] = (uint8_t)type;
            status[v] = (uint8_t)st;
        }
    }
}

__global__ __launch_bounds__(WPB * RR_WAVE) void dump_unpack_kernel(const uint8_t *__restrict__ data, const uint64_t *__restrict__ in_offs,
                                                                    uint64_t n, const uint64_t *__restrict__ out_offs, uint8_t *out,
                                                                    uint64_t out_cap, uint8_t *status, const uint64_t *err,
                                                                    rr_rdbfile_result *result) {
    const uint32_t lane = lane_id();
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = (uint64_t)gridDim.x * WPB;
    if (gtid == 0) result->bytes = *err ? ~0ull : out_offs[n];
    uint64_t n_bad = 0;
    for (uint64_t v = first64(gtid / RR_WAVE); v < n; v += nwaves) {
        if (rfl(status[v])) { ++n_bad; continue; }
        const uint64_t b0 = first64(out_offs[v]), b1 = first64(out_offs[v + 1]);
        if (b1 > out_cap) {
            ++n_bad;
            if (lane == 0) status[v] = RR_E_CAPACITY;
            continue;
        }
        if (b1 > b0) wave_copy(out + b0, data + first64(in_offs[v]) + 1, (uint32_t)(b1 - b0));
    }
    if (lane == 0 && n_bad) atomicAdd((unsigned long long *)&result->n_bad, (unsigned long long)n_bad);
}

// the stream pass's workgroups for at most `bytes` bytes
uint32_t crc_grid(uint64_t bytes) { return capped_grid(bytes, (uint64_t)WPB * PIECE, MAX_WAVES / WPB); }

}  // namespace

// scratch of the section: y[n + 2] | the scan's look-back words | the error word | part[MAX_WAVES]
extern "C" uint64_t rr_rdbfile_scratch_words(uint64_t n) { return n + 2 + rr_scan_words(n + 1) + 1 + MAX_WAVES; }
// rr_crc64_device: part[MAX_WAVES]
extern "C" uint64_t rr_crc64_scratch_words(void) { return MAX_WAVES; }
// the DUMP calls: the scan's look-back words and the error word
extern "C" uint64_t rr_rdbdump_scratch_words(uint64_t n) { return rr_scan_words(n) + 1; }

extern "C" hipError_t rr_launch_crc64(const uint8_t *data, uint64_t bytes, uint64_t *state, uint64_t *scratch, hipStream_t stream) {
    const uint32_t g = crc_grid(bytes);
    hipLaunchKernelGGL(crc_stream_kernel, dim3(g), dim3(WPB * RR_WAVE), 0, stream, data, (const uint64_t *)nullptr, bytes, 0ull, ~0ull,
                       (const uint64_t *)state, gf_xpow8((uint64_t)PIECE * g * WPB), scratch, 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crc_finish_kernel, dim3(1), dim3(RR_WAVE), 0, stream, (const uint64_t *)nullptr, bytes, 0ull, ~0ull, state,
                       (const uint64_t *)scratch, g * WPB, 0, (uint8_t *)nullptr, (const uint64_t *)nullptr,
                       (rr_rdbfile_result *)nullptr);
    return hipGetLastError();
}

extern "C" hipError_t rr_launch_rdbfile(const rr_rdbfile_in *in, uint32_t flags, uint8_t *out, uint64_t out_cap, uint64_t *rec_offsets,
                                        uint8_t *rec_status, uint64_t *state, rr_rdbfile_result *result, uint64_t *scratch,
                                        hipStream_t stream) {
    const uint64_t n = in->payloads.n, lbw = rr_scan_words(n + 1);
    uint64_t *y = scratch, *lb = y + n + 2, *err = lb + lbw, *part = err + 1;
    const Sec S = {in->payloads.data, in->payloads.offsets, in->payloads.data_cap, in->keys.data, in->keys.offsets, in->keys.data_cap,
                   in->types, in->status, in->expires, in->idle, in->freq, in->head, in->head_bytes, n, flags};
    const uint32_t gs = capped_grid(n, WPB * RR_WAVE, REC_GRID_CAP);
    hipLaunchKernelGGL(file_size_kernel, dim3(gs), dim3(WPB * RR_WAVE), 0, stream, S, y, rec_status, lb, lbw + 1, result);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(y, n + 1, lb, err, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(file_emit_kernel, dim3(gs), dim3(WPB * RR_WAVE), 0, stream, S, (const uint64_t *)y, (const uint8_t *)rec_status,
                       out, out_cap, rec_offsets, (const uint64_t *)err, result);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int eof = (flags & RR_RDBFILE_EOF) != 0, off = (flags & RR_RDBFILE_NO_CKSUM) != 0;
    // the checksum covers the 0xFF; the capacity test also counts the checksum's own 8 bytes
    const uint32_t g = crc_grid(out_cap);
    hipLaunchKernelGGL(crc_stream_kernel, dim3(g), dim3(WPB * RR_WAVE), 0, stream, (const uint8_t *)out, (const uint64_t *)(y + n + 1),
                       (uint64_t)eof, eof ? 8ull : 0ull, out_cap, (const uint64_t *)state, gf_xpow8((uint64_t)PIECE * g * WPB), part, off);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crc_finish_kernel, dim3(1), dim3(RR_WAVE), 0, stream, (const uint64_t *)(y + n + 1), (uint64_t)eof,
                       eof ? 8ull : 0ull, out_cap, state, (const uint64_t *)part, g * WPB, off, eof ? out : (uint8_t *)nullptr,
                       (const uint64_t *)err, result);
    return hipGetLastError();
}

extern "C" hipError_t rr_launch_rdbdump(const uint8_t *data, uint64_t in_cap, const uint64_t *in_offs, const uint8_t *types,
                                        const uint8_t *status, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_offs,
                                        uint8_t *out_status, uint64_t *scratch, rr_rdbfile_result *result, hipStream_t stream) {
    const uint64_t lbw = rr_scan_words(n);
    uint64_t *lb = scratch, *err = scratch + lbw;
    hipLaunchKernelGGL(dump_size_kernel, dim3(capped_grid(n, WPB * RR_WAVE, REC_GRID_CAP)), dim3(WPB * RR_WAVE), 0, stream, in_offs, in_cap,
                       status, n, out_offs, out_status, lb, lbw + 1, result);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(out_offs, n, lb, err, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dump_emit_kernel, dim3(capped_grid(n, WPB, DUMP_GRID)), dim3(WPB * RR_WAVE), 0, stream, data, in_offs, types, n,
                       (const uint64_t *)out_offs, out, out_cap, out_status, (const uint64_t *)err, result);
    return hipGetLastError();
}

extern "C" hipError_t rr_launch_rdbdump_verify(const uint8_t *data, uint64_t in_cap, const uint64_t *in_offs, uint64_t n, uint8_t *out,
                                               uint64_t out_cap, uint64_t *out_offs, uint8_t *types, uint8_t *status, uint64_t *scratch,
                                               rr_rdbfile_result *result, hipStream_t stream) {
    const uint64_t lbw = rr_scan_words(n);
    uint64_t *lb = scratch, *err = scratch + lbw;
    hipLaunchKernelGGL(dump_check_kernel, dim3(capped_grid(n, WPB, DUMP_GRID)), dim3(WPB * RR_WAVE), 0, stream, data, in_cap, in_offs, n,
                       out_offs, types, status, lb, lbw + 1, result);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(out_offs, n, lb, err, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dump_unpack_kernel, dim3(capped_grid(n, WPB, DUMP_GRID)), dim3(WPB * RR_WAVE), 0, stream, data, in_offs, n,
                       (const uint64_t *)out_offs, out, out_cap, status, (const uint64_t *)err, result);
    return hipGetLastError();
}
