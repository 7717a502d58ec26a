"""What rr_rdbsave_batch must produce, restated in plain Python from the reference's source text
(include/rr_rdbsave.h states the same rule), and the loader's side of it for round trips.

  save(val, descs, arena, list_fill)   the bytes rdbSaveObject (rdb.c:761-900) writes, with
                                       `rdbcompression no`, for the object desObject builds from
                                       the value; SET_HT / HASH_HT in the flat order
  load(type, payload)                  rdbLoadObject (rdb.c:1450-1700) for the eight types, back
                                       to the plain model that model() gives for a flat value
  save_batch(...)                      the whole call: types, data, offsets, status, totals

Which values are saveable is rr_encode_batch's rule, tests/encode_expect.py.  Python integers
throughout; the two places where the reference's arithmetic is 32-bit are marked.
"""
import struct

import numpy as np

import redrock_old_amd as rr
from encode_expect import accepted_value  # noqa: F401 (re-exported)

_ZL = (rr.T_HASH_ZIPLIST, rr.T_ZSET_ZIPLIST)
I32 = (-(1 << 31), (1 << 31) - 1)
OPT_LEVEL = (4096, 8192, 16384, 32768, 65536)   # quicklist.c:47
SAFETY = 8192                                   # quicklist.c:51


def _signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


# ---- primitives --------------------------------------------------------------------------------
def save_len(n):
    """rdbSaveLen, rdb.c:147-178."""
    if n < 1 << 6:                                   # :151
        return bytes([n])
    if n < 1 << 14:                                  # :156
        return bytes([0x40 | (n >> 8), n & 0xFF])
    if n <= 0xFFFFFFFF:                              # :162
        return b"\x80" + struct.pack(">I", n)
    return b"\x81" + struct.pack(">Q", n)            # :169


def encode_integer(v):
    """rdbEncodeInteger, rdb.c:241-261: None when v is outside int32."""
    if -(1 << 7) <= v <= (1 << 7) - 1:               # :242
        return b"\xC0" + struct.pack("<b", v)
    if -(1 << 15) <= v <= (1 << 15) - 1:             # :246
        return b"\xC1" + struct.pack("<h", v)
    if I32[0] <= v <= I32[1]:                        # :251
        return b"\xC2" + struct.pack("<i", v)
    return None


def canonical_int(s):
    """The value when s is exactly what ll2string prints for it (rdbTryIntegerEncoding's strtoll +
    ll2string + memcmp, rdb.c:307-321; the same strings string2ll accepts, util.c:360-424), else
    None.  No sign '+', no space, no leading zero, no "-0", no empty string, int64 range."""
    if not s or len(s) > 20:
        return None
    body = s[1:] if s[:1] == b"-" else s
    if not body or not all(0x30 <= c <= 0x39 for c in body):
        return None
    if body[:1] == b"0" and (len(body) > 1 or s[:1] == b"-"):
        return None
    v = int(s)
    return v if -(1 << 63) <= v < 1 << 63 else None


def save_raw_string(s):
    """rdbSaveRawString, rdb.c:411-441, without the LZF branch (:426)."""
    if len(s) <= 11:                                 # :416
        v = canonical_int(s)
        if v is not None:
            enc = encode_integer(v)                  # :320
            if enc is not None:
                return enc
    return save_len(len(s)) + s                      # :434-438


def save_longlong(v):
    """rdbSaveLongLongAsStringObject, rdb.c:444-460."""
    enc = encode_integer(v)
    if enc is not None:
        return enc
    txt = str(v).encode()
    return save_len(len(txt)) + txt


# ---- ziplist entries (ziplist.c) -----------------------------------------------------------------
def zip_try_encoding(s):
    """zipTryEncoding, ziplist.c:480-504: (encoding byte, body) or None."""
    if len(s) >= 32 or len(s) == 0:                  # :483
        return None
    v = canonical_int(s)                             # string2ll :484
    if v is None:
        return None
    if 0 <= v <= 12:                                 # :487
        return 0xF1 + v, b""
    if -128 <= v <= 127:                             # :489
        return 0xFE, struct.pack("<b", v)
    if -32768 <= v <= 32767:                         # :491
        return 0xC0, struct.pack("<h", v)
    if -(1 << 23) <= v <= (1 << 23) - 1:             # :493, zipSaveInteger :517-520
        return 0xF0, struct.pack("<i", v)[:3]
    if I32[0] <= v <= I32[1]:                        # :495
        return 0xD0, struct.pack("<i", v)
    return 0xE0, struct.pack("<q", v)                # :498


def zip_entry(prevlen, s):
    """One entry as __ziplistInsert writes it, ziplist.c:829-836."""
    out = bytes([prevlen]) if prevlen < 254 else b"\xFE" + struct.pack("<I", prevlen & 0xFFFFFFFF)   # :408-419
    ie = zip_try_encoding(s)
    if ie is not None:
        return out + bytes([ie[0]]) + ie[1]
    n = len(s)
    if n <= 0x3F:                                    # :338
        hdr = bytes([n])
    elif n <= 0x3FFF:                                # :341
        hdr = bytes([0x40 | (n >> 8), n & 0xFF])
    else:                                            # :346
        hdr = b"\x80" + struct.pack(">I", n)
    return out + hdr + s


def allow_insert(node_sz, count, fill, sz):
    """_quicklistNodeAllowInsert, quicklist.c:420-450, for an existing node."""
    overhead = (1 if sz < 254 else 5) + (1 if sz < 64 else 2 if sz < 16384 else 5)   # :427-438
    new_sz = (node_sz + sz + overhead) & 0xFFFFFFFF  # unsigned int, :441
    if fill < 0 and -fill - 1 < len(OPT_LEVEL) and new_sz <= OPT_LEVEL[-fill - 1]:   # :401-416, :442
        return True
    if new_sz > SAFETY:                              # :444
        return False
    return count < fill                              # :446


def clamp_fill(fill):
    """quicklistSetFill (quicklist.c:117-124) into `int fill : 16` (quicklist.h:78)."""
    return max(-5, min(32767, fill))


def list_nodes(strings, fill):
    """The node ziplists desList's quicklistPushTail loop builds (quicklist.c:503-520)."""
    fill = clamp_fill(fill)
    nodes, cur, prev = [], None, 0
    for s in strings:
        if cur is None or not allow_insert(11 + len(cur["body"]), cur["count"], fill, len(s)):
            cur = {"body": b"", "count": 0, "tail": 10}
            nodes.append(cur)
            prev = 0
        ent = zip_entry(prev, s)
        cur["tail"] = 10 + len(cur["body"])
        cur["body"] += ent
        cur["count"] += 1
        prev = len(ent) & 0xFFFFFFFF                 # zipRawEntryLength, unsigned int, :471-476
    return [struct.pack("<IIH", (11 + len(n["body"])) & 0xFFFFFFFF, n["tail"], n["count"]) + n["body"] + b"\xFF"
            for n in nodes]


# ---- save ----------------------------------------------------------------------------------------
def save(val, descs, arena, list_fill=-2):
    """val: dict(type, enc); descs: (kind, data, len) with unsigned data; arena: bytes.  The value
    must be saveable (accepted_value)."""
    t = val["type"]

    def s(d):
        return arena[d[1]:d[1] + d[2]]

    if t == rr.T_STRING:                             # rdbSaveStringObject, rdb.c:463-480
        if val["enc"] == 1:
            return save_longlong(_signed(descs[0][1]))
        return save_raw_string(s(descs[0]))
    if t == rr.T_SET_INTSET:                         # rdb.c:816-820
        w = val["enc"]
        blob = struct.pack("<II", w, len(descs) & 0xFFFFFFFF)
        blob += b"".join((d[1] & ((1 << (8 * w)) - 1)).to_bytes(w, "little") for d in descs)
        return save_raw_string(blob)
    if t in _ZL:                                     # rdb.c:826-830, :862-866
        return save_raw_string(s(descs[0]))
    if t == rr.T_SET_HT:                             # rdb.c:794-815
        return save_len(len(descs)) + b"".join(save_raw_string(s(d)) for d in descs)
    if t == rr.T_HASH_HT:                            # rdb.c:868-897
        return save_len(len(descs) // 2) + b"".join(save_raw_string(s(d)) for d in descs)
    if t == rr.T_ZSET_SKIPLIST:                      # rdb.c:831-856
        out = save_len(len(descs) // 2)
        for j, d in enumerate(descs):
            out += save_raw_string(s(d)) if j % 2 == 0 else struct.pack("<Q", d[1])   # :605-608
        return out
    if t == rr.T_LIST_QUICKLIST:                     # rdb.c:770-788
        strings = [str(_signed(d[1])).encode() if d[0] == rr.K_INT else s(d) for d in descs]
        nodes = list_nodes(strings, list_fill)
        return save_len(len(nodes)) + b"".join(save_raw_string(z) for z in nodes)
    raise ValueError(t)


def model(val, descs, arena):
    """The plain model of a saveable flat value, what load() gives back."""
    t = val["type"]

    def s(d):
        return arena[d[1]:d[1] + d[2]]

    if t == rr.T_STRING:
        return ("string", str(_signed(descs[0][1])).encode() if val["enc"] == 1 else s(descs[0]))
    if t == rr.T_SET_INTSET:
        return ("intset", val["enc"], [_signed(d[1]) for d in descs])
    if t in _ZL:
        return ("ziplist", s(descs[0]))
    if t == rr.T_SET_HT:
        return ("set", [s(d) for d in descs])
    if t == rr.T_HASH_HT:
        return ("hash", [s(d) for d in descs])
    if t == rr.T_ZSET_SKIPLIST:
        return ("zset", [s(d) if j % 2 == 0 else d[1] for j, d in enumerate(descs)])
    return ("list", [str(_signed(d[1])).encode() if d[0] == rr.K_INT else s(d) for d in descs])


# ---- load ----------------------------------------------------------------------------------------
class _Rd:
    def __init__(self, b):
        self.b, self.p = b, 0

    def take(self, n):
        assert self.p + n <= len(self.b), "payload truncated"
        out = self.b[self.p:self.p + n]
        self.p += n
        return out

    def length(self):
        """rdbLoadLenByRef, rdb.c:190-224: (is encoded, value)."""
        c = self.take(1)[0]
        k = c >> 6
        if k == 3:
            return True, c & 0x3F
        if k == 0:
            return False, c & 0x3F
        if k == 1:
            return False, ((c & 0x3F) << 8) | self.take(1)[0]
        if c == 0x80:
            return False, struct.unpack(">I", self.take(4))[0]
        assert c == 0x81, "unknown length encoding"
        return False, struct.unpack(">Q", self.take(8))[0]

    def string(self):
        """rdbGenericLoadStringObject, rdb.c:483-540, and rdbLoadIntegerObject :266-302."""
        enc, n = self.length()
        if not enc:
            return self.take(n)
        assert n in (0, 1, 2), "LZF or unknown string encoding"
        return str(struct.unpack(("<b", "<h", "<i")[n], self.take((1, 2, 4)[n]))[0]).encode()


def walk_ziplist(z):
    """The entries of a ziplist as the strings ziplistGet gives (ziplist.c:1034-1052), its header
    checked against the walk."""
    zlbytes, zltail, zllen = struct.unpack("<IIH", z[:10])
    assert zlbytes == len(z) and z[-1] == 0xFF
    p, out, prev, last = 10, [], 0, 10
    while z[p] != 0xFF:
        last = p
        if z[p] < 254:
            pl, p = z[p], p + 1
        else:
            pl, p = struct.unpack("<I", z[p + 1:p + 5])[0], p + 5
        assert pl == prev, "prevlen chain"
        e = z[p]
        if e < 0xC0:
            if e >> 6 == 0:
                n, p = e & 0x3F, p + 1
            elif e >> 6 == 1:
                n, p = ((e & 0x3F) << 8) | z[p + 1], p + 2
            else:
                n, p = struct.unpack(">I", z[p + 1:p + 5])[0], p + 5
            out.append(z[p:p + n])
            p += n
        else:
            p += 1
            if 0xF1 <= e <= 0xFD:
                v = e - 0xF1
            else:
                w = {0xFE: 1, 0xC0: 2, 0xF0: 3, 0xD0: 4, 0xE0: 8}[e]
                v = int.from_bytes(z[p:p + w], "little", signed=True)
                p += w
            out.append(str(v).encode())
        prev = p - last
    assert p == len(z) - 1 and zllen == len(out) and zltail == last
    return out


def load(typ, payload):
    """rdbLoadObject (rdb.c:1450-1700) for the eight types the engine writes."""
    r = _Rd(payload)
    if typ == rr.T_STRING:                           # :1452-1456
        out = ("string", r.string())
    elif typ == rr.T_LIST_QUICKLIST:                 # :1619-1633: each node a ziplist, appended
        items = []
        for _ in range(r.length()[1]):
            items += walk_ziplist(r.string())
        out = ("list", items)
    elif typ == rr.T_SET_HT:                         # :1485-1527
        out = ("set", [r.string() for _ in range(r.length()[1])])
    elif typ == rr.T_ZSET_SKIPLIST:                  # :1528-1567, RDB_TYPE_ZSET_2: binary doubles
        items = []
        for _ in range(r.length()[1]):
            items.append(r.string())
            items.append(struct.unpack("<Q", r.take(8))[0])
        out = ("zset", items)
    elif typ == rr.T_HASH_HT:                        # :1568-1618
        out = ("hash", [r.string() for _ in range(2 * r.length()[1])])
    elif typ == rr.T_SET_INTSET:                     # :1634-1700: the blob kept as it is
        b = r.string()
        w, n = struct.unpack("<II", b[:8])
        assert len(b) == 8 + w * n
        out = ("intset", w, [int.from_bytes(b[8 + w * k:8 + w * (k + 1)], "little", signed=True) for k in range(n)])
    elif typ in _ZL:
        out = ("ziplist", r.string())
    else:
        raise ValueError(typ)
    assert r.p == len(payload), "bytes left over"
    return out


# ---- the batch -----------------------------------------------------------------------------------
def flat_values(values, elems, arena):
    """Per value: (val dict, descs or None when its range passes elem_cap)."""
    ecap = len(elems)
    kinds, datas, lens = elems["kind"].tolist(), elems["data"].tolist(), elems["len"].tolist()
    for r in values:
        val = {"type": int(r["type"]), "enc": int(r["enc"]), "status": int(r["status"])}
        b, c = int(r["elem_base"]), int(r["n_elems"])
        descs = [(kinds[k], datas[k], lens[k]) for k in range(b, b + c)] if b + c <= ecap else None
        yield val, descs


def save_batch(values, elems, arena, list_fill=-2, data_cap=None):
    """(types, data, offsets, status, totals, payloads): data has min(data_cap, offsets[n]) bytes,
    unwritten ones zero; payloads[i] is None for an unsaveable value."""
    ab = arena.tobytes()
    n = len(values)
    pays, payloads, n_elems = [], [], 0
    for (val, descs), r in zip(flat_values(values, elems, arena), values):
        n_elems += int(r["n_elems"])
        if not accepted_value(val, descs, len(arena)):
            payloads.append(None)
            pays.append(0)
            continue
        used = descs[:1] if val["type"] in _ZL else descs
        payloads.append(save(val, used, ab, list_fill))
        pays.append(sum(d[2] for d in used if d[0] in (rr.K_STR, rr.K_ZLRAW)))
    offsets = np.zeros(n + 1, np.uint64)
    at = 0
    for i, p in enumerate(payloads):
        offsets[i] = at
        at += len(p) if p is not None else 0
    offsets[n] = at
    if data_cap is None:
        data_cap = at
    out = bytearray(min(data_cap, at))
    status = np.zeros(n, np.uint8)
    n_bad = payload = 0
    for i, p in enumerate(payloads):
        o = int(offsets[i])
        if p is None:
            status[i] = rr.E_ENCODE
        elif o + len(p) > data_cap:
            status[i] = rr.E_CAPACITY
        else:
            out[o:o + len(p)] = p
            payload += pays[i]
            continue
        n_bad += 1
    totals = {"n_elems": n_elems, "bytes": at, "n_bad": n_bad, "payload": payload}
    return values["type"].astype(np.uint8), np.frombuffer(bytes(out), np.uint8), offsets, status, totals, payloads
