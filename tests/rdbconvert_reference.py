"""What rr_rdbconvert_batch must produce, restated in plain Python from the reference's source text
(include/rr_rdbconvert.h states the same rule): for an RDB value payload that rr_rdbload_batch left with
RR_RDBLOAD_E_CONVERT, the rock blob of the object rdbLoadObject (rdb.c:1476-1600) ends up with.

  convert_blob(typ, payload, opts)   (status, new type, blob or None, payload bytes, strings read)
  convert_batch(types, data, offsets, load_status, opts, data_cap)
                                     (out data, offsets, out_types, status, totals, blobs)

Built on rdbload_reference.Rd (the reader) and rdb_reference.zip_entry / zip_try_encoding /
canonical_int (ziplist entries, string2ll)."""
import functools
import struct

import numpy as np

import redrock_old_amd as rr

import rdbload_reference as ld
from rdb_reference import canonical_int, zip_entry

OK, E_CAPACITY, E_CONVERT, SKIP = 0, 11, ld.E_CONVERT, 45
MAX_N = 512                   # RR_RDBCONVERT_MAX_N
MAX_WAVES = 16384             # RR_RDBCONVERT_MAX_WAVES
MAX_SLICE = ld.MAX_SLICE


class Stay(Exception):
    """The value stays RR_RDBLOAD_E_CONVERT."""


def d2string(bits):
    """d2string, util.c:517-552, of the double with these bits; None where the reference asserts (NaN,
    t_zset.c:137) or prints with %.17g (:548) [deviation]."""
    v = struct.unpack("<d", struct.pack("<Q", bits))[0]
    if v != v:                                           # :518
        return None
    if v in (float("inf"), float("-inf")):               # :520-524
        return b"-inf" if v < 0 else b"inf"
    if v == 0:                                           # :525-530
        return b"-0" if bits >> 63 else b"0"
    if -4503599627370495.0 < v < 4503599627370496.0 and v == float(int(v)):   # :542-545
        return str(int(v)).encode()                      # ll2string
    return None


def intset_blob(values):
    """What intsetAdd (intset.c:204-231) leaves after the values in this order, from intsetNew
    (:97-102): followed add by add, so the statement does not rest on "sorted and unique"."""
    enc, arr = 2, []
    for v in values:
        need = 8 if not -(1 << 31) <= v < 1 << 31 else 4 if not -(1 << 15) <= v < 1 << 15 else 2   # :45-52
        if need > enc:                                   # :211 intsetUpgradeAndAdd :157-180: at either end
            enc = need
            arr = [v] + arr if v < 0 else arr + [v]
            continue
        lo, hi = 0, len(arr)                             # intsetSearch :115-154
        while lo < hi:
            mid = (lo + hi) // 2
            if arr[mid] < v:
                lo = mid + 1
            else:
                hi = mid
        if lo < len(arr) and arr[lo] == v:               # :219-221 already there
            continue
        arr.insert(lo, v)                                # :224-227
    return struct.pack("<II", enc, len(arr)) + b"".join(v.to_bytes(enc, "little", signed=True) for v in arr)


def ziplist_of(strings):
    """ziplistPush(.., ZIPLIST_TAIL) of each string on ziplistNew (ziplist.c:578-586, :956-960)."""
    body, prev, tail = b"", 0, 10
    for s in strings:
        e = zip_entry(prev, s)                           # prevlen :408-419, zipTryEncoding :480-504
        tail = 10 + len(body)
        body += e
        prev = len(e)
    return struct.pack("<IIH", 11 + len(body), tail, len(strings)) + body + b"\xFF"


def sdscmp(a, b):
    """sds.c:792-802."""
    m = min(len(a), len(b))
    if a[:m] != b[:m]:
        return -1 if a[:m] < b[:m] else 1
    return (len(a) > len(b)) - (len(a) < len(b))


def _zsl_before(x, y):
    """zslInsert's walk (t_zset.c:142-145): x stays in front of y.  Doubles compare, so -0 == 0."""
    sx, sy = struct.unpack("<d", struct.pack("<Q", x[1]))[0], struct.unpack("<d", struct.pack("<Q", y[1]))[0]
    if sx != sy:
        return -1 if sx < sy else 1
    return sdscmp(x[0], y[0])


def _convert(typ, payload, o):
    """(new type, body, payload bytes, strings read); raises Stay or rdbload_reference.Bad."""
    r = ld.Rd(payload)
    if typ == rr.T_SET_HT:                               # rdb.c:1476-1516
        n = r.count()
        if n > o["set_max_intset_entries"] or n > MAX_N:   # :1481; the sort arrays [deviation]
            raise Stay
        vals = []
        for _ in range(n):
            v = canonical_int(r.string())                # isSdsRepresentableAsLongLong :1501
            if v is None:
                raise Stay
            vals.append(v)
        body = intset_blob(vals)
        out = rr.T_SET_INTSET, body, len(body), n
    elif typ == rr.T_HASH_HT:                            # :1556-1596
        n = r.count()
        if n > o["hash_max_ziplist_entries"]:            # :1567
            raise Stay
        strs = []
        for _ in range(2 * n):
            s = r.string()
            if len(s) > o["hash_max_ziplist_value"]:     # :1586
                raise Stay
            strs.append(s)
        z = ziplist_of(strs)                             # :1580-1583
        out = rr.T_HASH_ZIPLIST, struct.pack("<Q", len(z)) + z, len(z), 2 * n
    elif typ == rr.T_ZSET_SKIPLIST:                      # :1517-1555
        n = r.count()
        if n > o["zset_max_ziplist_entries"] or n > MAX_N:   # :1553; the sort arrays [deviation]
            raise Stay
        items = []
        for _ in range(n):
            if ld.is_lzf_at(payload, r.p):               # [deviation]: the sort compares member bytes in place
                raise Stay
            m = r.string()
            if len(m) > o["zset_max_ziplist_value"]:     # :1554
                raise Stay
            bits = struct.unpack("<Q", r.take(8))[0]     # rdbLoadBinaryDoubleValue :1540
            if d2string(bits) is None:                   # NaN, %.17g [deviation]
                raise Stay
            items.append((m, bits))
        items.sort(key=functools.cmp_to_key(_zsl_before))   # the skiplist's order; equal pairs are the same bytes
        strs = []
        for m, bits in items:                            # zsetConvert t_zset.c:1221-1230, zzlInsertAt :1035-1038
            strs += [m, d2string(bits)]
        z = ziplist_of(strs)
        out = rr.T_ZSET_ZIPLIST, struct.pack("<Q", len(z)) + z, len(z), n
    else:                                                # the reverse conversions, Lists, anything else
        raise Stay
    if r.p != len(payload):
        raise Stay
    if out[2] >= MAX_SLICE:
        raise Stay
    return out


def convert_blob(typ, payload, opts=None):
    """(status, new type, blob or None, payload bytes, strings read) of an attempted value."""
    o = opts or ld.DEFAULTS
    if len(payload) >= MAX_SLICE:
        return E_CONVERT, 0, None, 0, 0
    try:
        t, body, pay, nel = _convert(typ, bytes(payload), o)
    except (Stay, ld.Bad):
        return E_CONVERT, 0, None, 0, 0
    return OK, t, bytes([t]) + struct.pack("<I", o["lru"] & 0xFFFFFF) + body, pay, nel


def convert_batch(types, data, offsets, load_status, opts=None, data_cap=None):
    """(out data, offsets, out_types, status, totals, blobs): out data has min(data_cap, offsets[n])
    bytes, unwritten ones zero."""
    n = len(offsets) - 1
    db = bytes(data)
    res = []
    for i in range(n):
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        if int(load_status[i]) != E_CONVERT:
            res.append((SKIP, 0, None, 0, 0))
        elif o0 > o1 or o1 > len(db):
            res.append((E_CONVERT, 0, None, 0, 0))
        else:
            res.append(convert_blob(int(types[i]), db[o0:o1], opts))
    out_offs = np.zeros(n + 1, np.uint64)
    at = 0
    for i, x in enumerate(res):
        out_offs[i] = at
        at += len(x[2]) if x[0] == OK else 0
    out_offs[n] = at
    if data_cap is None:
        data_cap = at
    out = bytearray(min(data_cap, at))
    status, out_types = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    n_bad = pay = nel = 0
    for i, (st, t, blob, p, e) in enumerate(res):
        o = int(out_offs[i])
        if st == OK and o + len(blob) > data_cap:
            st = E_CAPACITY
        status[i], out_types[i] = st, t
        if st == SKIP:
            continue
        if st != OK:
            n_bad += 1
            continue
        out[o:o + len(blob)] = blob
        pay += p
        nel += e
    totals = {"n_elems": nel, "bytes": at, "n_bad": n_bad, "payload": pay}
    return (np.frombuffer(bytes(out), np.uint8), out_offs, out_types, status, totals,
            [x[2] if x[0] == OK else None for x in res])
