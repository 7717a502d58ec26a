"""What rr_d2string and rr_rdbzset_batch must produce, restated in plain Python (include/rr_d2string.h and
include/rr_rdbzset.h state the same rule).

  d2string(bits)                      the reference's d2string (util.c:517-552) of the double with these bits
  libc_g17(v)                         the C library's snprintf("%.17g"): what Python's '%.17g' is held to
  zset_blob(payload, opts)            (status, blob or None, payload bytes, members) of an attempted value
  zset_batch(types, data, offsets, convert_status, opts, data_cap)
                                      (out data, offsets, status, totals, blobs)

Built on rdbconvert_reference (ziplist_of, _zsl_before: the ziplist and the skiplist's order) and
rdbload_reference.Rd (the reader)."""
import ctypes
import functools
import math
import struct

import numpy as np

import rdbconvert_reference as cv
import rdbload_reference as ld

OK, E_CAPACITY, E_CONVERT, SKIP = 0, 11, ld.E_CONVERT, 55
ZSET_2, ZSET_ZIPLIST = 5, 12
D2STRING_MAX = 24

_libc = ctypes.CDLL(None)
_libc.snprintf.restype = ctypes.c_int
_buf = ctypes.create_string_buffer(64)


def libc_g17(v):
    n = _libc.snprintf(_buf, ctypes.c_size_t(64), b"%.17g", ctypes.c_double(v))
    return _buf.raw[:n]


def to_double(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def to_bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def d2string(bits):
    v = to_double(bits)
    if v != v:                                           # :518
        return b"nan"
    if math.isinf(v):                                    # :520-524
        return b"-inf" if v < 0 else b"inf"
    if v == 0:                                           # :525-530
        return b"-0" if bits >> 63 else b"0"
    if -4503599627370495.0 < v < 4503599627370496.0 and v == float(int(v)):   # :542-545
        return str(int(v)).encode()                      # ll2string
    return ("%.17g" % v).encode()                        # :548


def _convert(payload, o):
    r = ld.Rd(payload)
    n = r.count()
    if n > o["zset_max_ziplist_entries"] or n > cv.MAX_N:    # rdb.c:1553; the sort arrays [deviation]
        raise cv.Stay
    items = []
    for _ in range(n):
        if ld.is_lzf_at(payload, r.p):                   # [deviation]: the sort compares member bytes in place
            raise cv.Stay
        m = r.string()
        if len(m) > o["zset_max_ziplist_value"]:         # :1554
            raise cv.Stay
        bits = struct.unpack("<Q", r.take(8))[0]         # rdbLoadBinaryDoubleValue :1540
        if to_double(bits) != to_double(bits):           # NaN: the reference asserts (t_zset.c:137) [deviation]
            raise cv.Stay
        items.append((m, bits))
    if r.p != len(payload):
        raise cv.Stay
    items.sort(key=functools.cmp_to_key(cv._zsl_before))
    strs = []
    for m, bits in items:                                # zsetConvert t_zset.c:1221-1230, zzlInsertAt :1035-1038
        strs += [m, d2string(bits)]
    z = cv.ziplist_of(strs)
    if len(z) >= cv.MAX_SLICE:
        raise cv.Stay
    return struct.pack("<Q", len(z)) + z, len(z), n


def zset_blob(payload, opts=None):
    o = opts or ld.DEFAULTS
    if len(payload) >= cv.MAX_SLICE:
        return E_CONVERT, None, 0, 0
    try:
        body, pay, nel = _convert(bytes(payload), o)
    except (cv.Stay, ld.Bad):
        return E_CONVERT, None, 0, 0
    return OK, bytes([ZSET_ZIPLIST]) + struct.pack("<I", o["lru"] & 0xFFFFFF) + body, pay, nel


def zset_batch(types, data, offsets, convert_status, opts=None, data_cap=None):
    """out data has min(data_cap, offsets[n]) bytes, unwritten ones zero."""
    n = len(offsets) - 1
    db = bytes(data)
    res = []
    for i in range(n):
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        if int(convert_status[i]) != E_CONVERT or int(types[i]) != ZSET_2:
            res.append((SKIP, None, 0, 0))
        elif o0 > o1 or o1 > len(db):
            res.append((E_CONVERT, None, 0, 0))
        else:
            res.append(zset_blob(db[o0:o1], opts))
    out_offs = np.zeros(n + 1, np.uint64)
    at = 0
    for i, x in enumerate(res):
        out_offs[i] = at
        at += len(x[1]) if x[0] == OK else 0
    out_offs[n] = at
    if data_cap is None:
        data_cap = at
    out = bytearray(min(data_cap, at))
    status = np.zeros(n, np.uint8)
    n_bad = pay = nel = 0
    for i, (st, blob, p, e) in enumerate(res):
        o = int(out_offs[i])
        if st == OK and o + len(blob) > data_cap:
            st = E_CAPACITY
        status[i] = st
        if st == SKIP:
            continue
        if st != OK:
            n_bad += 1
            continue
        out[o:o + len(blob)] = blob
        pay += p
        nel += e
    totals = {"n_elems": nel, "bytes": at, "n_bad": n_bad, "payload": pay}
    return np.frombuffer(bytes(out), np.uint8), out_offs, status, totals, [x[1] if x[0] == OK else None for x in res]


# ---- the scores the printer is held to (shared by the CPU and the GPU test) --------------------------------
EXAMPLES = [(0.1, b"0.10000000000000001"), (1e-5, b"1.0000000000000001e-05"), (0.0001, b"0.0001"), (1e16, b"10000000000000000"),
            (1e17, b"1e+17"), (1e23, b"9.9999999999999992e+22"), (2.0**52, b"4503599627370496"),
            (5e-324, b"4.9406564584124654e-324"), (1.7976931348623157e308, b"1.7976931348623157e+308")]


def tie_scores(seed=18, per=200):
    """Doubles with exactly 18 significant digits, the last a 5: a d-digit integer part plus an odd
    multiple of 2^-(18 - d) (its fraction has 18 - d digits, ending in 5)."""
    rng = np.random.default_rng(seed)
    out = []
    for d in range(1, 16):
        f = 18 - d
        for _ in range(per):
            ip = int(rng.integers(10 ** (d - 1), 10 ** d))
            odd = 2 * int(rng.integers(0, 1 << (f - 1))) + 1
            v = ip + odd * 2.0 ** -f                     # exact: ip < 2^50 and d + f = 18 digits need < 2^53 * 2^-f
            assert float(ip) + odd * 2.0 ** -f == v and (int(v * 2 ** f) == ip * 2 ** f + odd)
            out.append(v)
    return out


def edge_scores():
    """The edge list of the issue, both signs of each, as bits."""
    vs = [v for v, _ in EXAMPLES]
    vs += [math.ldexp(1.0, k) for k in range(-1074, 1024)]
    for k in range(-323, 309):
        v = float("1e%d" % k)
        vs += [math.nextafter(v, 0.0), v, math.nextafter(v, math.inf)]
    vs += [2.0**52 - 1, 2.0**52, 2.0**52 - 0.5, 2.0**53, 2.0**52 - 2]
    vs += [9.9999999999999991e-05, 0.0001, 99999999999999984.0, 1e17, 1.5, 17.0, 0.0, math.inf]
    vs += tie_scores()
    bits = [to_bits(v) for v in vs] + [to_bits(-v) for v in vs]
    bits += [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF]   # NaNs
    return np.array(bits, np.uint64)
