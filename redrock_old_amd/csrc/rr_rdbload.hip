// rr_rdbload.hip — gfx950 kernels of include/rr_rdbload.h: RDB value payloads -> rock blobs (the
// blob desObject turns into the object rdbLoadObject builds, rdb.c:1450-1700).  The stage is
// rr_stage_device.h's (size, scan, emit): rdbload_size_kernel takes every decision (status, CONVERT,
// an LZF stream's validity and exact output length), rdbload_emit_kernel writes the bytes.
//
// A value is a chain of dependent length
// prefixes, so the walk is wave-uniform: every lane takes the same path, the state lives in scalar
// registers, and the lanes are used where bytes are independent.  A header is read by one 64-byte
// load, a byte a lane, and picked apart with readlane (one memory round trip per string, per
// ziplist entry, per ~20 LZF sequences); bodies are copied by the whole wave, 16 bytes a lane; an
// LZF sequence is copied by the wave, a byte a lane.  Every load of payload bytes in the size pass
// goes through a buffer resource that covers exactly the value's slice, so a corrupt length reads
// zeros, never a neighbour.  The emit pass runs the same walk over values the size pass accepted.
//
// Content the walk has to look at but that is not in the payload as it is — the decimal text of an
// integer-form string, an LZF string — is first put into the wave's LDS window (RR_RDBLOAD_LZF_NODE_MAX
// bytes): a List node in the LZF form is decompressed there and walked there; of an intset blob or a
// ziplist only the header is needed, of a Set member or a String at most 20 bytes.  An LZF string
// that is only copied is decompressed by the emit pass straight into its place in the blob.
#include <hip/hip_runtime.h>

#include "rr_rdbload_device.h"
#include "rr_kernels.h"

using namespace rr;

namespace {

constexpr uint32_t WPB = 4;             // waves (values in flight) per workgroup
constexpr uint32_t GRID_CAP = 16384;    // workgroups
static_assert(WPB * WIN <= 65536 && WIN >= 64, "the windows are static LDS");

// ---- a List node: the strict ziplist walk (ziplist.c:300-447, parse_ziplist of rr_kernels.hip) ---
// The node's L bytes are at c.  EMIT: every entry as u32 len | bytes at out + pos.
template <bool EMIT>
__device__ __forceinline__ bool walk_node(const Rd &r, const Src &c, uint64_t L, const lds_u8 *win, uint8_t *out, uint64_t &pos,
                                          uint64_t &pay, uint64_t &nel) {
    const uint32_t lane = lane_id();
    if (L < 11) return false;
    uint32_t v = src_peek(r, c, 0, win);
    if (le_lanes(v, 0, 4) != L) return false;
    const uint32_t zltail = (uint32_t)le_lanes(v, 4, 4), zllen = (uint32_t)le_lanes(v, 8, 2);
    uint64_t p = 10, prev_raw = 0, last = 10, cnt = 0, base = 0;
    for (;;) {
        if (p >= L) return false;
        if (p - base + 14 > RR_WAVE) {
            base = p;
            v = src_peek(r, c, (uint32_t)base, win);
        }
        const uint32_t i = (uint32_t)(p - base);
        const uint32_t b0 = rl32(v, i);
        if (b0 == 0xFF) break;
        uint64_t pl;
        uint32_t pls;
        if (b0 < 254) { pl = b0; pls = 1; }
        else {
            if (p + 5 > L - 1) return false;
            pl = le_lanes(v, i + 1, 4);
            pls = 5;
        }
        if (pl != prev_raw) return false;
        const uint64_t q = p + pls;
        if (q >= L - 1) return false;
        const uint32_t enc = rl32(v, i + pls);
        uint64_t end;
        if (enc < 0xC0) {
            const uint32_t cls = enc & 0xC0;
            uint64_t ls, sl;
            if (cls == 0x00) { ls = 1; sl = enc & 0x3F; }
            else if (cls == 0x40) {
                if (q + 2 > L - 1) return false;
                ls = 2;
                sl = ((uint64_t)(enc & 0x3F) << 8) | rl32(v, i + pls + 1);
            } else {
                if (q + 5 > L - 1) return false;
                ls = 5;
                sl = be_lanes(v, i + pls + 1, 4);
            }
            const uint64_t d = q + ls;
            end = d + sl;
            if (end > L - 1) return false;
            if (EMIT) {
                uint8_t *dst = out + pos;
                if (lane == 0) put_le(dst, sl, 4);
                if (c.lds) {
                    for (uint32_t k = lane; k < (uint32_t)sl; k += RR_WAVE) dst[4 + k] = win[(uint32_t)d + k];
                } else {
                    wave_copy(dst + 4, r.base + c.off + d, (uint32_t)sl);
                }
                pay += sl;
            }
            pos += 4 + sl;
        } else {
            uint32_t isz;
            switch (enc) {
                case 0xFE: isz = 1; break;
                case 0xC0: isz = 2; break;
                case 0xF0: isz = 3; break;
                case 0xD0: isz = 4; break;
                case 0xE0: isz = 8; break;
                default:
                    if (enc >= 0xF1 && enc <= 0xFD) isz = 0;
                    else return false;
            }
            end = q + 1 + isz;
            if (end > L - 1) return false;
            const uint64_t x = le_lanes(v, i + pls + 1, isz);
            int64_t iv;
            if (isz == 0) iv = (int64_t)(enc & 0x0F) - 1;
            else if (isz == 8) iv = (int64_t)x;
            else iv = (int64_t)(x << (64 - 8 * isz)) >> (64 - 8 * isz);   // sign-extend isz bytes
            const uint32_t dl = dec_len(iv);
            if (EMIT) {
                if (lane == 0) {
                    put_le(out + pos, dl, 4);
                    dec_write(out + pos + 4, iv);   // sdsll2str
                }
                pay += dl;
            }
            pos += 4 + dl;
        }
        ++cnt;
        prev_raw = end - p;
        last = p;
        p = end;
    }
    if (p != L - 1) return false;
    if (zllen != 0xFFFF && zllen != cnt) return false;
    if (zltail != last) return false;
    nel += cnt;
    return true;
}

// ---- one value -----------------------------------------------------------------------------------
// Returns the blob's size and the status (size pass), or writes the blob at out (EMIT, a value the
// size pass accepted).  pay / nel: rr_totals.payload and n_elems of this value, added.
template <bool EMIT>
__device__ uint64_t load_value(Rd &r, uint32_t type, const Opt &O, lds_u8 *win, uint8_t *out, uint32_t &status, uint64_t &pay,
                               uint64_t &nel) {
    const uint32_t lane = lane_id();
    uint64_t pos = 5;
    bool conv = false;
    uint32_t st = RR_OK;
    Str s;
    if (EMIT && lane == 0) {
        out[0] = (uint8_t)type;
        put_le(out + 1, O.lru, 4);
    }
    if (type == RR_TYPE_STRING) {
        if ((st = rd_string<!EMIT>(r, s))) { status = st; return 0; }
        ++nel;
        bool isint = s.kind == S_INT;
        int64_t iv = s.iv;
        if (!isint && s.len >= 1 && s.len <= 20) {         // tryObjectEncoding, object.c:458
            const Src c = materialize(r, s, 20, win);
            isint = str_is_ll(r, c, s.len, win, iv);
        }
        if (isint) {
            if (EMIT && lane == 0) {
                out[5] = RR_ENC_INT;
                put_le(out + 6, (uint64_t)iv, 8);
            }
            pos = 14;
        } else {
            if (EMIT) {
                if (lane == 0) out[5] = s.len <= RR_EMBSTR_SIZE_LIMIT ? RR_ENC_EMBSTR : RR_ENC_RAW;
                emit_string(r, s, out + 6);
                pay += s.len;
            }
            pos = 6 + (uint64_t)s.len;
        }
    } else if (type == RR_TYPE_SET_HT || type == RR_TYPE_HASH_HT || type == RR_TYPE_ZSET_SKIPLIST) {
        if (r.p >= r.n) { status = RR_RDBLOAD_E_TRUNC; return 0; }
        const uint32_t hv = ld8(r.R, r.p + lane);
        bool ie;
        uint64_t n;
        uint32_t used;
        if ((st = parse_len(hv, 0, r.n - r.p, ie, n, used))) { status = st; return 0; }   // a count site
        r.p += used;
        if (EMIT && lane == 0) put_le(out + 5, n, 8);
        pos = 13;
        const uint32_t per = type == RR_TYPE_HASH_HT ? 2 : 1;
        bool all_int = type == RR_TYPE_SET_HT && n <= O.set_ie;
        uint64_t maxlen = 0;
        for (uint64_t k = 0; k < n; ++k) {
            for (uint32_t j = 0; j < per; ++j) {
                if ((st = rd_string<!EMIT>(r, s))) { status = st; return 0; }
                ++nel;
                if (!EMIT && all_int && s.kind != S_INT) {   // isSdsRepresentableAsLongLong, rdb.c:1501
                    int64_t t;
                    all_int = s.len >= 1 && s.len <= 20 && str_is_ll(r, materialize(r, s, 20, win), s.len, win, t);
                }
                if (s.len > maxlen) maxlen = s.len;
                if (EMIT) {
                    if (lane == 0) put_le(out + pos, s.len, 8);
                    emit_string(r, s, out + pos + 8);
                    pay += s.len;
                }
                pos += 8 + (uint64_t)s.len;
            }
            if (type == RR_TYPE_ZSET_SKIPLIST) {           // rdbLoadBinaryDoubleValue
                if (r.n - r.p < 8) { status = RR_RDBLOAD_E_TRUNC; return 0; }
                if (EMIT && lane < 8) out[pos + lane] = (uint8_t)ld8(r.R, r.p + lane);
                r.p += 8;
                pos += 8;
            }
        }
        if (type == RR_TYPE_SET_HT) conv = all_int;                                        // rdb.c:1481-1506
        else if (type == RR_TYPE_HASH_HT) conv = n <= O.hash_e && maxlen <= O.hash_v;      // :1567-1596
        else conv = n <= O.zset_e && maxlen <= O.zset_v;                                   // :1553-1555
    } else if (type == RR_TYPE_LIST_QUICKLIST) {
        if (r.p >= r.n) { status = RR_RDBLOAD_E_TRUNC; return 0; }
        const uint32_t hv = ld8(r.R, r.p + lane);
        bool ie;
        uint64_t n;
        uint32_t used;
        if ((st = parse_len(hv, 0, r.n - r.p, ie, n, used))) { status = st; return 0; }
        r.p += used;
        for (uint64_t k = 0; k < n; ++k) {
            if ((st = rd_string<!EMIT>(r, s))) { status = st; return 0; }
            ++nel;
            if (s.kind == S_LZF && s.len > WIN) { conv = true; continue; }   // the CPU path's (rr_rdbload.h)
            const Src c = materialize(r, s, WIN, win);
            if (!walk_node<EMIT>(r, c, s.len, win, out, pos, pay, nel)) { status = RR_RDBLOAD_E_ZIPLIST; return 0; }
        }
    } else if (type == RR_TYPE_SET_INTSET) {
        if ((st = rd_string<!EMIT>(r, s))) { status = st; return 0; }
        ++nel;
        if (!EMIT) {
            if (s.len < 8) { status = RR_RDBLOAD_E_ZIPLIST; return 0; }
            const Src c = materialize(r, s, 8, win);
            const uint32_t hv = src_peek(r, c, 0, win);
            const uint64_t enc = le_lanes(hv, 0, 4), cnt = le_lanes(hv, 4, 4);
            if ((enc != 2 && enc != 4 && enc != 8) || (uint64_t)s.len != 8 + enc * cnt) { status = RR_RDBLOAD_E_ZIPLIST; return 0; }
            conv = cnt > O.set_ie;                                                         // rdb.c:1686
        } else {
            emit_string(r, s, out + 5);
            pay += s.len;
        }
        pos = 5 + (uint64_t)s.len;
    } else {   // HASH_ZIPLIST, ZSET_ZIPLIST
        if ((st = rd_string<!EMIT>(r, s))) { status = st; return 0; }
        ++nel;
        if (!EMIT) {
            if (s.len < 11) { status = RR_RDBLOAD_E_ZIPLIST; return 0; }
            const Src c = materialize(r, s, 10, win);
            const uint32_t zllen = (uint32_t)le_lanes(src_peek(r, c, 0, win), 8, 2);
            conv = zllen == 0xFFFF || zllen / 2 > (type == RR_TYPE_HASH_ZIPLIST ? O.hash_e : O.zset_e);   // rdb.c:1692, :1698
        } else {
            if (lane == 0) put_le(out + 5, s.len, 8);
            emit_string(r, s, out + 13);
            pay += s.len;
        }
        pos = 13 + (uint64_t)s.len;
    }
    if (r.p != r.n) { status = RR_RDBLOAD_E_EXTRA; return 0; }
    if (conv) { status = RR_RDBLOAD_E_CONVERT; return 0; }
    status = RR_OK;
    return pos;
}

__device__ __forceinline__ bool known_type(uint32_t t) {
    return t == RR_TYPE_STRING || t == RR_TYPE_SET_HT || t == RR_TYPE_HASH_HT || t == RR_TYPE_ZSET_SKIPLIST ||
           t == RR_TYPE_SET_INTSET || t == RR_TYPE_ZSET_ZIPLIST || t == RR_TYPE_HASH_ZIPLIST || t == RR_TYPE_LIST_QUICKLIST;
}

__device__ __forceinline__ lds_u8 *wave_window() {
    __shared__ uint8_t windows[WPB * WIN];
    return (lds_u8 *)windows + (threadIdx.x / RR_WAVE) * WIN;
}

// blob sizes into out_offs[0, n), out_offs[n] = 0; status; and the stage's zeroing
__global__ __launch_bounds__(WPB * RR_WAVE) void rdbload_size_kernel(const uint8_t *__restrict__ data, uint64_t in_cap,
                                                                     const uint64_t *__restrict__ in_offs,
                                                                     const uint8_t *__restrict__ types, uint64_t n, Opt O,
                                                                     uint64_t *__restrict__ out_offs, uint8_t *__restrict__ status,
                                                                     uint64_t *__restrict__ zero, uint64_t nzero, rr_totals *totals) {
    lds_u8 *win = wave_window();
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    zero_stage_words(gtid, nthreads, zero, nzero, &out_offs[n], totals);
    const uint64_t nwaves = nthreads / RR_WAVE;
    for (uint64_t v = first64(gtid / RR_WAVE); v < n; v += nwaves) {
        const uint32_t type = rfl(types[v]);
        const uint64_t o0 = first64(in_offs[v]), o1 = first64(in_offs[v + 1]);
        uint32_t st = RR_OK;
        uint64_t size = 0, pay = 0, nel = 0;
        if (!known_type(type)) st = RR_RDBLOAD_E_TYPE;
        else if (o0 > o1 || o1 > in_cap) st = RR_RDBLOAD_E_TRUNC;
        else if (o1 - o0 >= MAX_SLICE) st = RR_RDBLOAD_E_LEN;
        else {
            Rd r = rd_of(data, o0, o1);
            size = load_value<false>(r, type, O, win, nullptr, st, pay, nel);
        }
        if (lane_id() == 0) {
            out_offs[v] = st ? 0 : size;
            status[v] = (uint8_t)st;
        }
    }
}

// out_offs scanned.  Writes the blobs of the values that are valid and fit out_cap; RR_E_CAPACITY for
// the valid ones that do not; the totals.
__global__ __launch_bounds__(WPB * RR_WAVE) void rdbload_emit_kernel(const uint8_t *__restrict__ data,
                                                                     const uint64_t *__restrict__ in_offs,
                                                                     const uint8_t *__restrict__ types, uint64_t n, Opt O,
                                                                     const uint64_t *__restrict__ out_offs, uint8_t *out, uint64_t out_cap,
                                                                     uint8_t *status, const uint64_t *err, rr_totals *totals) {
    lds_u8 *win = wave_window();
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nwaves = nthreads / RR_WAVE;
    if (gtid == 0) totals->bytes = *err ? ~0ull : out_offs[n];
    uint64_t pay = 0, nel = 0, n_bad = 0;   // wave-uniform
    for (uint64_t v = first64(gtid / RR_WAVE); v < n; v += nwaves) {
        const uint32_t type = rfl(types[v]);
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
        load_value<true>(r, type, O, win, out + b0, st, pay, nel);
    }
    add_totals(totals, pay, nel, n_bad);
}

}  // namespace

// scratch: the scan's look-back words and the error word
extern "C" uint64_t rr_rdbload_scratch_words(uint64_t n) { return rr_scan_words(n) + 1; }

extern "C" hipError_t rr_launch_rdbload(const uint8_t *data, uint64_t in_cap, const uint64_t *in_offs, const uint8_t *types,
                                        uint64_t n, const uint32_t *opt6, uint8_t *out, uint64_t out_cap, uint64_t *out_offs,
                                        uint8_t *status, uint64_t *scratch, rr_totals *totals, hipStream_t stream) {
    const uint64_t lbw = rr_scan_words(n);
    uint64_t *lb = scratch, *err = scratch + lbw;
    const Opt O = opt_of(opt6);
    const uint32_t grid = capped_grid(n, WPB, GRID_CAP);
    hipLaunchKernelGGL(rdbload_size_kernel, dim3(grid), dim3(WPB * RR_WAVE), 0, stream, data, in_cap, in_offs, types, n, O,
                       out_offs, status, lb, lbw + 1, totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rr_launch_scan_u64(out_offs, n, lb, err, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rdbload_emit_kernel, dim3(grid), dim3(WPB * RR_WAVE), 0, stream, data, in_offs, types, n, O,
                       (const uint64_t *)out_offs, out, out_cap, status, (const uint64_t *)err, totals);
    return hipGetLastError();
}
