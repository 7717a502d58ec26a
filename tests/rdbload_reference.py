"""What rr_rdbload_batch must produce, restated in plain Python from the reference's source text
(include/rr_rdbload.h states the same rule): RDB value payload -> the rock blob desObject turns into
the object rdbLoadObject (rdb.c:1450-1700) builds.

  load_blob(typ, payload, opts)   (status, blob or None, payload bytes, elems walked)
  load_batch(types, data, offsets, opts, data_cap)
                                  (out data, offsets, status, totals, blobs)

tests/rdb_reference.py (the save direction and a loader back to a plain model) and
tests/lzf_reference.py (lzf_decompress) are the statements this one is checked against."""
import struct

import numpy as np

import redrock_old_amd as rr

import lzf_reference as lzf
from rdb_reference import canonical_int

OK, E_CAPACITY = 0, 11
E_TYPE, E_LEN, E_TRUNC, E_LZF, E_EXTRA, E_ZIPLIST, E_CONVERT = 32, 33, 34, 35, 36, 37, 38
LZF_NODE_MAX = 10240          # RR_RDBLOAD_LZF_NODE_MAX
MAX_SLICE = 0x7FFFFFF0
TYPES = (rr.T_STRING, rr.T_SET_HT, rr.T_HASH_HT, rr.T_ZSET_SKIPLIST, rr.T_SET_INTSET, rr.T_ZSET_ZIPLIST,
         rr.T_HASH_ZIPLIST, rr.T_LIST_QUICKLIST)
DEFAULTS = dict(lru=0, set_max_intset_entries=512, hash_max_ziplist_entries=512, hash_max_ziplist_value=64,
                zset_max_ziplist_entries=128, zset_max_ziplist_value=64)   # config.c:2261-2267


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def c_opts(o):
    return rr.RdbLoadOpts(**o)


class Bad(Exception):
    def __init__(self, status):
        self.status = status


class Rd:
    def __init__(self, b):
        self.b, self.p = bytes(b), 0

    def take(self, n):
        if n > len(self.b) - self.p:                     # rioRead fails
            raise Bad(E_TRUNC)
        out = self.b[self.p:self.p + n]
        self.p += n
        return out

    def length(self):
        """rdbLoadLenByRef, rdb.c:190-224: (is encoded, value)."""
        c = self.take(1)[0]
        t = (c & 0xC0) >> 6                              # :196
        if t == 3:                                       # :197 RDB_ENCVAL
            return True, c & 0x3F
        if t == 0:                                       # :201 RDB_6BITLEN
            return False, c & 0x3F
        if t == 1:                                       # :204 RDB_14BITLEN
            return False, ((c & 0x3F) << 8) | self.take(1)[0]
        if c == 0x80:                                    # :208 RDB_32BITLEN, ntohl
            return False, struct.unpack(">I", self.take(4))[0]
        if c == 0x81:                                    # :213 RDB_64BITLEN, ntohu64
            return False, struct.unpack(">Q", self.take(8))[0]
        raise Bad(E_LEN)                                 # :219 unknown length encoding

    def count(self):
        """rdbLoadLen(rdb, NULL), :230-235: isencoded is not looked at, so the 0xC0 form is its low
        six bits (:200)."""
        return self.length()[1]

    def string(self):
        """rdbGenericLoadStringObject, rdb.c:487-540: the loaded bytes."""
        enc, n = self.length()                           # :497
        if not enc:
            return self.take(n)                          # :519-539
        if n in (0, 1, 2):                               # :500-503 rdbLoadIntegerObject :266-302
            v = struct.unpack(("<b", "<h", "<i")[n], self.take((1, 2, 4)[n]))[0]
            return str(v).encode()                       # ll2string
        if n == 3:                                       # :504-505 rdbLoadLzfStringObject :369-407
            clen, ulen = self.count(), self.count()      # :376-377
            stream = self.take(clen)                     # :389
            if ulen >= MAX_SLICE:                        # [stricter]
                raise Bad(E_LZF)
            s = lzf.decompress(stream, ulen)             # :390
            if s is None or len(s) != ulen:              # 0: the reference exits; short: [stricter]
                raise Bad(E_LZF)
            return s
        raise Bad(E_LEN)                                 # :512 unknown string encoding


def walk_node(z):
    """The decoder's strict ziplist rule (RR_E_ZL_CORRUPT; ziplist.c:300-447; oracle/pyoracle.py
    parse_ziplist states it too): the entries as ziplistGet gives them, integers as sdsll2str
    renders them, or None."""
    L = len(z)
    if L < 11 or struct.unpack_from("<I", z, 0)[0] != L:
        return None
    zltail, zllen = struct.unpack_from("<I", z, 4)[0], struct.unpack_from("<H", z, 8)[0]
    p, prev_raw, last, out = 10, 0, 10, []
    while True:
        if p >= L:
            return None
        if z[p] == 0xFF:
            break
        if z[p] < 254:                                   # ziplist.c:408-419
            pl, pls = z[p], 1
        else:
            if p + 5 > L - 1:
                return None
            pl, pls = struct.unpack_from("<I", z, p + 1)[0], 5
        if pl != prev_raw:
            return None
        q = p + pls
        if q >= L - 1:
            return None
        enc = z[q]
        if enc < 0xC0:                                   # strings, :332-364
            if enc >> 6 == 0:
                ls, sl = 1, enc & 0x3F
            elif enc >> 6 == 1:
                if q + 2 > L - 1:
                    return None
                ls, sl = 2, ((enc & 0x3F) << 8) | z[q + 1]
            else:
                if q + 5 > L - 1:
                    return None
                ls, sl = 5, struct.unpack_from(">I", z, q + 1)[0]
            d = q + ls
            end = d + sl
            if end > L - 1:
                return None
            out.append(z[d:end])
        else:                                            # integers, :507-534
            if 0xF1 <= enc <= 0xFD:
                isz = 0
            elif enc in (0xFE, 0xC0, 0xF0, 0xD0, 0xE0):
                isz = {0xFE: 1, 0xC0: 2, 0xF0: 3, 0xD0: 4, 0xE0: 8}[enc]
            else:
                return None
            end = q + 1 + isz
            if end > L - 1:
                return None
            v = (enc & 0x0F) - 1 if isz == 0 else int.from_bytes(z[q + 1:end], "little", signed=True)
            out.append(str(v).encode())
        prev_raw, last, p = end - p, p, end
    if p != L - 1 or (zllen != 0xFFFF and zllen != len(out)) or zltail != last:
        return None
    return out


def is_lzf_at(b, p):
    return p < len(b) and b[p] == 0xC3


def _load(typ, payload, o):
    """(blob body, CONVERT?, payload bytes, elems walked); raises Bad."""
    r = Rd(payload)
    pay = nel = 0
    conv = False
    if typ == rr.T_STRING:                               # rdb.c:1455-1458
        p0 = r.p
        s = r.string()
        nel += 1
        intform = payload[p0] in (0xC0, 0xC1, 0xC2)
        v = int(s) if intform else (canonical_int(s) if len(s) <= 20 else None)   # object.c:458 string2l
        if v is not None:
            body = b"\x01" + struct.pack("<q", v)        # OBJ_ENCODING_INT
        else:
            body = (b"\x08" if len(s) <= 44 else b"\x00") + s   # object.c:489 EMBSTR, else RAW
            pay += len(s)
    elif typ in (rr.T_SET_HT, rr.T_HASH_HT, rr.T_ZSET_SKIPLIST):
        n = r.count()                                    # :1478, :1523, :1561
        body = struct.pack("<Q", n)
        all_int, maxlen = True, 0
        for _ in range(n):
            for _ in range(2 if typ == rr.T_HASH_HT else 1):
                s = r.string()
                nel += 1
                pay += len(s)
                all_int = all_int and canonical_int(s) is not None   # isSdsRepresentableAsLongLong :1501
                maxlen = max(maxlen, len(s))
                body += struct.pack("<Q", len(s)) + s
            if typ == rr.T_ZSET_SKIPLIST:
                body += r.take(8)                        # rdbLoadBinaryDoubleValue :1540
        if typ == rr.T_SET_HT:                           # :1481-1506
            conv = n <= o["set_max_intset_entries"] and all_int
        elif typ == rr.T_HASH_HT:                        # :1567-1596
            conv = n <= o["hash_max_ziplist_entries"] and maxlen <= o["hash_max_ziplist_value"]
        else:                                            # :1553-1555
            conv = n <= o["zset_max_ziplist_entries"] and maxlen <= o["zset_max_ziplist_value"]
    elif typ == rr.T_LIST_QUICKLIST:                     # :1619-1630
        body = b""
        for _ in range(r.count()):
            lz = is_lzf_at(payload, r.p)
            z = r.string()
            nel += 1
            if lz and len(z) > LZF_NODE_MAX:             # the deviation of rr_rdbload.h: the CPU path's
                conv = True
                continue
            ents = walk_node(z)
            if ents is None:
                raise Bad(E_ZIPLIST)
            nel += len(ents)
            for e in ents:
                pay += len(e)
                body += struct.pack("<I", len(e)) + e
    elif typ == rr.T_SET_INTSET:                         # :1633-1640, :1683-1688
        b = r.string()
        nel += 1
        if len(b) < 8:
            raise Bad(E_ZIPLIST)
        enc, n = struct.unpack_from("<II", b, 0)
        if enc not in (2, 4, 8) or len(b) != 8 + enc * n:
            raise Bad(E_ZIPLIST)
        conv = n > o["set_max_intset_entries"]
        body = b
        pay += len(b)
    else:                                                # the two ziplists, :1689-1700
        z = r.string()
        nel += 1
        if len(z) < 11:
            raise Bad(E_ZIPLIST)
        zllen = struct.unpack_from("<H", z, 8)[0]
        thr = o["hash_max_ziplist_entries"] if typ == rr.T_HASH_ZIPLIST else o["zset_max_ziplist_entries"]
        conv = zllen == 0xFFFF or zllen // 2 > thr
        body = struct.pack("<Q", len(z)) + z
        pay += len(z)
    if r.p != len(payload):
        raise Bad(E_EXTRA)
    return body, conv, pay, nel


def load_blob(typ, payload, opts=None):
    """(status, blob or None, payload bytes, elems walked)."""
    o = opts or DEFAULTS
    if typ not in TYPES:
        return E_TYPE, None, 0, 0
    if len(payload) >= MAX_SLICE:
        return E_LEN, None, 0, 0
    try:
        body, conv, pay, nel = _load(typ, bytes(payload), o)
    except Bad as e:
        return e.status, None, 0, 0
    if conv:
        return E_CONVERT, None, 0, 0
    return OK, bytes([typ]) + struct.pack("<I", o["lru"] & 0xFFFFFF) + body, pay, nel


def load_batch(types, data, offsets, opts=None, data_cap=None):
    """(out data, offsets, status, totals, blobs): out data has min(data_cap, offsets[n]) bytes,
    unwritten ones zero."""
    n = len(offsets) - 1
    db = bytes(data)
    res = []
    for i in range(n):
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        if int(types[i]) not in TYPES:
            res.append((E_TYPE, None, 0, 0))
        elif o0 > o1 or o1 > len(db):
            res.append((E_TRUNC, None, 0, 0))
        else:
            res.append(load_blob(int(types[i]), db[o0:o1], opts))
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
        if st != OK:
            n_bad += 1
            continue
        out[o:o + len(blob)] = blob
        pay += p
        nel += e
    totals = {"n_elems": nel, "bytes": at, "n_bad": n_bad, "payload": pay}
    return np.frombuffer(bytes(out), np.uint8), out_offs, status, totals, [x[1] if x[0] == OK else None for x in res]


def pack(payloads):
    """Payload list -> (data, offsets)."""
    offs = np.zeros(len(payloads) + 1, np.uint64)
    np.cumsum([len(p) for p in payloads], out=offs[1:])
    raw = b"".join(payloads)
    return np.frombuffer(raw, np.uint8).copy() if raw else np.zeros(0, np.uint8), offs
