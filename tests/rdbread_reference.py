"""Restatement in Python of include/rr_rdbread.h, beside rdbfile_reference.py (whose parse() states
rdbLoadRio's framing for the streams rr_rdbfile_section writes): the record index with record starts
and ends, the legacy types and the 0xFD opcode (rdb.c:2072-2242, extents by lengths alone), and the
split's per-record rule: prefix opcodes, type, key (rdbload_reference.Rd.string: plain, integer as
ll2string text, LZF through lzf_reference) and the payload as it is.

  walk(stream)                  dict(version, records [(start, end, db)], items [(opcode, at, end)], eof_at,
                                has_cksum, cksum), or raises Stop(code, at, partial dict)
  split_record(rec)             (status, type, key, payload, expire, idle, freq)
  split(data, starts, ends, ..) rr_rdbread_split's outputs
  builders                      lzf_literal, lzf_string, int_string, old_double, value payloads"""
import struct

import numpy as np

import redrock_old_amd as rr

import rdb_reference as ref
import rdbload_reference as ld

MAX_SLICE = 0x7FFFFFF0
DONE, MORE, FULL = 0, 1, 2
E_CAPACITY = 11
E_SLICE, E_TRUNC, E_OPCODE, E_KEY, NO_CKSUM = 46, 47, 48, 49, 50
E_MAGIC, E_VERSION, E_UNSUPPORTED, E_LEN = 51, 52, 53, 54
E_CRC = 44
PREFIX_OPS = (0xFD, 0xFC, 0xF8, 0xF9)
NOT_A_TYPE = (0xF7, 0xFA, 0xFB, 0xFE, 0xFF)
ONE_STRING = (0, 9, 10, 11, 12, 13)
INDEXED = (0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14)


class Stop(Exception):
    def __init__(self, code, at, partial):
        self.code, self.at, self.partial = code, at, partial


# ---- builders ----------------------------------------------------------------------------------------
def lzf_literal(s):
    """An LZF stream of literal runs alone."""
    return b"".join(bytes([len(s[i:i + 32]) - 1]) + s[i:i + 32] for i in range(0, len(s), 32))


def lzf_string(stream, ulen):
    """The 0xC3 string form around an LZF stream that claims ulen bytes."""
    return b"\xC3" + ref.save_len(len(stream)) + ref.save_len(ulen) + stream


def lzf_backref(ln, dist):
    """One back reference of ln >= 3 bytes at distance dist >= 1 (lzf_d.c:106-181)."""
    off, l = dist - 1, ln - 2
    if l < 7:
        return bytes([(l << 5) | (off >> 8), off & 0xFF])
    return bytes([(7 << 5) | (off >> 8), l - 7, off & 0xFF])


def int_string(v):
    """The shortest integer form of v (rdbEncodeInteger, rdb.c:241-261)."""
    if -128 <= v <= 127:
        return b"\xC0" + struct.pack("<b", v)
    if -32768 <= v <= 32767:
        return b"\xC1" + struct.pack("<h", v)
    return b"\xC2" + struct.pack("<i", v)


def old_double(x):
    """rdbSaveDoubleValue's form as rdbLoadDoubleValue reads it (rdb.c:583-598)."""
    if x != x:
        return b"\xFD"
    if x in (float("inf"), float("-inf")):
        return b"\xFE" if x > 0 else b"\xFF"
    t = repr(x).encode()
    return bytes([len(t)]) + t


def counted(strings):
    return ref.save_len(len(strings)) + b"".join(strings)


def raw(s):
    """A string in the plain form whatever its bytes are."""
    return ref.save_len(len(s)) + s


# ---- the index ---------------------------------------------------------------------------------------
def _skip_string(r):
    enc, n = r.length()
    if not enc:
        r.take(n)
    elif n in (0, 1, 2):
        r.take((1, 2, 4)[n])
    elif n == 3:
        clen, _ = r.count(), r.count()
        r.take(clen)
    else:
        raise ld.Bad(ld.E_LEN)


def _skip_value(r, typ):
    if typ in ONE_STRING:
        _skip_string(r)
        return
    n = r.count()
    k = 0
    while k < n:                                         # (a count near 2^64 ends at the buffer's end)
        _skip_string(r)
        if typ == 4:
            _skip_string(r)
        elif typ == 5:
            r.take(8)
        elif typ == 3:
            l = r.take(1)[0]
            r.take(0 if l >= 253 else l)
        k += 1


def walk(stream):
    b = bytes(stream)
    out = {"version": 0, "records": [], "items": [], "eof_at": None, "has_cksum": False, "cksum": 0}
    if len(b) < 9:
        raise Stop(MORE, 0, out)
    if b[:5] != b"REDIS":
        raise Stop(E_MAGIC, 0, out)
    if not b[5:9].isdigit() or not 1 <= int(b[5:9]) <= 9:
        raise Stop(E_VERSION, 0, out)
    out["version"] = int(b[5:9])
    r = ld.Rd(b)
    r.p = 9
    db = 0
    while True:
        at = r.p
        try:
            op = r.take(1)[0]
            if op == 0xFF:
                if out["version"] >= 5:
                    out["cksum"] = struct.unpack("<Q", r.take(8))[0]
                    out["has_cksum"] = True
                out["eof_at"] = at
                out["end"] = r.p
                return out
            if op == 0xFA:
                _skip_string(r)
                _skip_string(r)
            elif op == 0xFE:
                db = r.count()
            elif op == 0xFB:
                r.count()
                r.count()
            if op in (0xFA, 0xFE, 0xFB):
                out["items"].append((op, at, r.p))
                continue
            while op in PREFIX_OPS:
                if op == 0xF8:
                    r.count()
                else:
                    r.take({0xFD: 4, 0xFC: 8, 0xF9: 1}[op])
                op = r.take(1)[0]
            if op not in INDEXED:
                raise Stop(E_UNSUPPORTED, at, out)
            _skip_string(r)
            _skip_value(r, op)
            out["records"].append((at, r.p, db))
        except ld.Bad as e:
            raise Stop(MORE if e.status == ld.E_TRUNC else E_LEN, at, out) from None


# ---- the split -----------------------------------------------------------------------------------------
def split_record(rec):
    """(status, type, key, payload, expire, idle, freq) of one record's bytes; on a nonzero status the
    rest is (0, b"", b"", -1, None, None)."""
    bad = lambda st: (st, 0, b"", b"", -1, None, None)
    r = ld.Rd(rec)
    expire, idle, freq = -1, None, None
    try:
        while True:
            op = r.take(1)[0]
            if op == 0xFD:
                expire = struct.unpack("<i", r.take(4))[0] * 1000      # rdb.c:2079-2086
            elif op == 0xFC:
                expire = struct.unpack("<q", r.take(8))[0]
            elif op == 0xF9:
                freq = r.take(1)[0]
            elif op == 0xF8:
                try:
                    idle = r.count()
                except ld.Bad as e:
                    return bad(E_TRUNC if e.status == ld.E_TRUNC else E_OPCODE)
            elif op in NOT_A_TYPE:
                return bad(E_OPCODE)
            else:
                break
        key = r.string()
    except ld.Bad as e:
        return bad(E_TRUNC if e.status == ld.E_TRUNC else E_KEY)
    return 0, op, key, rec[r.p:], expire, idle, freq


def split(data, rec_start, rec_end, data_cap=None, key_cap=None, pay_cap=None):
    """dict(keys, pays (lists; None where nothing is written), key_offsets, pay_offsets, types, expires, idle,
    freq, status, bytes, n_bad, result_status)."""
    b = bytes(data)
    data_cap = len(b) if data_cap is None else data_cap
    n = len(rec_start)
    keys, pays = [], []
    ko, po = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    ty, st = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    ex, idl, fq = np.full(n, -1, np.int64), np.full(n, (1 << 64) - 1, np.uint64), np.full(n, -1, np.int16)
    ka = pa = 0
    for i in range(n):
        s, e = int(rec_start[i]), int(rec_end[i])
        ko[i], po[i] = ka, pa
        if not (s <= e <= data_cap and e - s < MAX_SLICE):
            st[i] = E_SLICE
            keys.append(None)
            pays.append(None)
            continue
        status, typ, key, pay, expire, idle, freq = split_record(b[s:e])
        st[i] = status
        if status:
            keys.append(None)
            pays.append(None)
            continue
        ty[i], ex[i] = typ, expire
        idl[i] = (1 << 64) - 1 if idle is None else idle
        fq[i] = -1 if freq is None else freq
        ka += len(key)
        pa += len(pay)
        if (key_cap is not None and ka > key_cap) or (pay_cap is not None and pa > pay_cap):
            st[i] = E_CAPACITY
            key = pay = None
        keys.append(key)
        pays.append(pay)
    ko[n], po[n] = ka, pa
    over = (key_cap is not None and ka > key_cap) or (pay_cap is not None and pa > pay_cap)
    return dict(keys=keys, pays=pays, key_offsets=ko, pay_offsets=po, types=ty, expires=ex, idle=idl, freq=fq, status=st,
                bytes=pa, n_bad=int((st != 0).sum()), result_status=E_CAPACITY if over else 0)


assert (rr.RDBREAD_E_SLICE, rr.RDBREAD_E_TRUNC, rr.RDBREAD_E_OPCODE, rr.RDBREAD_E_KEY, rr.RDBREAD_NO_CKSUM) == \
    (E_SLICE, E_TRUNC, E_OPCODE, E_KEY, NO_CKSUM)
