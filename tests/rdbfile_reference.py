"""Restatement in Python of include/rr_rdbfile.h: the CRC-64 of crc64.c:1-12 with its table generated
from the polynomial, the shift that combines checksums, the writer of a stream section
(rdbSaveKeyValuePair, rdb.c:1017-1073; the EOF of rdbSaveRio :1249-1255), the head
(rdbSaveInfoAuxFields :1101-1122) and SELECTDB / RESIZEDB (:1193-1205), the DUMP writer and verifier
(cluster.c:4817-4867), and a parser of the framing that finds each payload's end by the walk of
rdbload_reference.py and checks the trailing checksum the way rdbLoadRio does (rdb.c:2229-2246)."""
import struct

import numpy as np

import rdb_reference as ref
import rdbload_reference as ld
import redrock_old_amd as rr

POLY_R = 0x95AC9329AC4BC9B5          # 0xad93d23594c935a9, bits reversed
M64 = (1 << 64) - 1
ONE = 1 << 63                        # x^0: bit 63 - i is the coefficient of x^i
RDB_VERSION = 9
MAX_SLICE = 0x7FFFFFF0
IDLE, FREQ, EOF, NO_CKSUM = rr.RDBFILE_IDLE, rr.RDBFILE_FREQ, rr.RDBFILE_EOF, rr.RDBFILE_NO_CKSUM
E_VALUE, E_KEY, E_SHORT, E_VERSION, E_CRC, E_CAPACITY = 40, 41, 42, 43, 44, 11


def _mulx(a):
    return (a >> 1) ^ (POLY_R if a & 1 else 0)


def _table():
    t = []
    for b in range(256):
        c = b
        for _ in range(8):
            c = _mulx(c)
        t.append(c)
    return t


TABLE = _table()
_NP_TABLE = np.array(TABLE, np.uint64)


def crc64_simple(crc, data):
    """crc64.c:173-186, a byte at a time."""
    for b in bytes(data):
        crc = TABLE[(crc ^ b) & 0xFF] ^ (crc >> 8)
    return crc


def gf_mul(a, b):
    r = 0
    for i in range(64):
        if (b >> (63 - i)) & 1:
            r ^= a
        a = _mulx(a)
    return r


def xpow8(n):
    """x^(8n) mod P."""
    r, sq = ONE, ONE
    for _ in range(8):
        sq = _mulx(sq)
    while n:
        if n & 1:
            r = gf_mul(r, sq)
        sq = gf_mul(sq, sq)
        n >>= 1
    return r


def shift(c, n):
    """c * x^(8n) mod P = crc64(c, n zero bytes)."""
    return gf_mul(c, xpow8(n)) if c else 0


def crc64(crc, data):
    """crc64(crc, data).  Long inputs use the linearity the header states: zero bytes in front change
    nothing, equal chunks are stepped together in numpy and combined by shifts (the CPU tests check
    this path against crc64_simple)."""
    data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    n = data.size
    if n < 1 << 14:
        return crc64_simple(crc, data.tobytes())
    m = 2048
    k = (n + m - 1) // m
    buf = np.zeros(k * m, np.uint8)
    buf[k * m - n:] = data
    cols = np.ascontiguousarray(buf.reshape(k, m).T)
    st = np.zeros(k, np.uint64)
    for j in range(m):
        st = _NP_TABLE[((st & np.uint64(0xFF)).astype(np.uint8) ^ cols[j]).astype(np.intp)] ^ (st >> np.uint64(8))
    xm = xpow8(m)
    acc = 0
    for c in st.tolist():
        acc = (gf_mul(acc, xm) if acc else 0) ^ c
    return acc ^ shift(crc, n)


# ---- writers -------------------------------------------------------------------------------------
def aux(key, val):
    return b"\xFA" + ref.save_raw_string(key) + ref.save_raw_string(val)


def head(ver, ctime, used_mem, repl=None, aof_preamble=False):
    out = b"REDIS%04d" % RDB_VERSION
    out += aux(b"redis-ver", ver.encode()) + aux(b"redis-bits", b"64") + aux(b"ctime", str(ctime).encode())
    out += aux(b"used-mem", str(used_mem).encode())
    if repl is not None:
        out += aux(b"repl-stream-db", str(repl[0]).encode()) + aux(b"repl-id", repl[1].encode())
        out += aux(b"repl-offset", str(repl[2]).encode())
    return out + aux(b"aof-preamble", b"1" if aof_preamble else b"0")


def selectdb(dbid, db_size, expires_size):
    return b"\xFE" + ref.save_len(dbid) + b"\xFB" + ref.save_len(min(db_size, 0xFFFFFFFF)) + ref.save_len(min(expires_size, 0xFFFFFFFF))


def _slice_ok(o0, o1, cap):
    return o0 <= o1 <= cap and o1 - o0 < MAX_SLICE


def record(typ, key, payload, expire=-1, idle=None, freq=None):
    out = b""
    if expire != -1:
        out += b"\xFC" + struct.pack("<q", expire)
    if idle is not None:
        out += b"\xF8" + ref.save_len(idle)
    if freq is not None:
        out += b"\xF9" + bytes([freq])
    return out + bytes([typ]) + ref.save_raw_string(key) + payload


def section(pay_data, pay_offs, types, status, key_data, key_offs, expires=None, idle=None, freq=None, head=b"", flags=0,
            crc_in=0, pay_cap=None, key_cap=None, out_cap=None):
    """dict(data, rec_offsets, rec_status, n_bad, bytes, status, crc): rr_rdbfile_section's outputs.  data is
    None when the section does not fit out_cap (status E_CAPACITY, crc == crc_in)."""
    n = len(pay_offs) - 1
    pb, kb = bytes(pay_data), bytes(key_data)
    pay_cap = len(pb) if pay_cap is None else pay_cap
    key_cap = len(kb) if key_cap is None else key_cap
    parts, offs, st = [bytes(head)], np.zeros(n + 1, np.uint64), np.zeros(n, np.uint8)
    at = len(head)
    for i in range(n):
        offs[i] = at
        p0, p1, k0, k1 = int(pay_offs[i]), int(pay_offs[i + 1]), int(key_offs[i]), int(key_offs[i + 1])
        if status[i] != 0 or not _slice_ok(p0, p1, pay_cap):
            st[i] = E_VALUE
        elif not _slice_ok(k0, k1, key_cap):
            st[i] = E_KEY
        else:
            r = record(int(types[i]), kb[k0:k1], pb[p0:p1], -1 if expires is None else int(expires[i]),
                       int(idle[i]) if flags & IDLE else None, int(freq[i]) if flags & FREQ else None)
            parts.append(r)
            at += len(r)
    offs[n] = at
    body = b"".join(parts)
    need = at + (9 if flags & EOF else 0)
    res = {"rec_offsets": offs, "rec_status": st, "n_bad": int((st != 0).sum()), "bytes": need}
    if out_cap is not None and need > out_cap:
        res.update(data=None, status=E_CAPACITY, crc=crc_in)
        return res
    if flags & EOF:
        body += b"\xFF"
    crc = crc_in if flags & NO_CKSUM else crc64(crc_in, body)
    if flags & EOF:
        body += struct.pack("<Q", crc)
    res.update(data=body, status=0, crc=crc)
    return res


def dump(typ, payload):
    """createDumpPayload, cluster.c:4817-4844."""
    b = bytes([typ]) + bytes(payload) + struct.pack("<H", RDB_VERSION)
    return b + struct.pack("<Q", crc64(0, b))


def dump_batch(data, offsets, types, status, data_cap=None, out_cap=None):
    """(values or None, offsets, status, n_bad): rr_rdbdump_batch's outputs."""
    n = len(offsets) - 1
    db = bytes(data)
    cap = len(db) if data_cap is None else data_cap
    vals, offs, st = [], np.zeros(n + 1, np.uint64), np.zeros(n, np.uint8)
    at = 0
    for i in range(n):
        offs[i] = at
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        if status[i] != 0 or not _slice_ok(o0, o1, cap):
            st[i] = E_VALUE
            vals.append(None)
            continue
        v = dump(int(types[i]), db[o0:o1])
        at += len(v)
        if out_cap is not None and at > out_cap:
            st[i] = E_CAPACITY
            v = None
        vals.append(v)
    offs[n] = at
    return vals, offs, st, int((st != 0).sum())


def dump_verify(b):
    """verifyDumpPayload, cluster.c:4850-4867 (11 bytes at least, rr_rdbfile.h): (status, type, payload)."""
    b = bytes(b)
    typ = b[0] if b else 0
    if len(b) < 11:
        return E_SHORT, typ, None
    if struct.unpack_from("<H", b, len(b) - 10)[0] > RDB_VERSION:
        return E_VERSION, typ, None
    if crc64(0, b[:-8]) != struct.unpack_from("<Q", b, len(b) - 8)[0]:
        return E_CRC, typ, None
    return 0, typ, b[1:-10]


# ---- the parser ------------------------------------------------------------------------------------
def skip_value(r, typ):
    """Moves ld.Rd r behind one value of RDB type typ: the walk of rdbload_reference._load."""
    if typ in (rr.T_STRING, rr.T_SET_INTSET, rr.T_HASH_ZIPLIST, rr.T_ZSET_ZIPLIST):
        r.string()
    elif typ in (rr.T_SET_HT, rr.T_HASH_HT, rr.T_ZSET_SKIPLIST):
        for _ in range(r.count()):
            r.string()
            if typ == rr.T_HASH_HT:
                r.string()
            if typ == rr.T_ZSET_SKIPLIST:
                r.take(8)
    elif typ == rr.T_LIST_QUICKLIST:
        for _ in range(r.count()):
            r.string()
    else:
        raise ValueError(f"type {typ}")


def parse(stream, checksum=True):
    """rdbLoadRio's framing (rdb.c:2040-2250): dict(version, aux, dbs, records, cksum_ok); a record is
    (dbid, key, expire or -1, idle or None, freq or None, type, payload)."""
    b = bytes(stream)
    assert b[:5] == b"REDIS"
    out = {"version": int(b[5:9]), "aux": [], "dbs": [], "records": []}
    r = ld.Rd(b)
    r.p = 9
    db, expire, idle, freq = 0, -1, None, None
    while True:
        op = r.take(1)[0]
        if op == 0xFC:
            expire = struct.unpack("<q", r.take(8))[0]
        elif op == 0xF8:
            idle = r.count()
        elif op == 0xF9:
            freq = r.take(1)[0]
        elif op == 0xFA:
            out["aux"].append((r.string(), r.string()))
        elif op == 0xFE:
            db = r.count()
        elif op == 0xFB:
            out["dbs"].append((db, r.count(), r.count()))
        elif op == 0xFF:
            break
        else:
            key = r.string()
            p0 = r.p
            skip_value(r, op)
            out["records"].append((db, key, expire, idle, freq, op, b[p0:r.p]))
            expire, idle, freq = -1, None, None
    want = struct.unpack("<Q", r.take(8))[0]
    assert r.p == len(b)
    out["cksum"] = want
    out["cksum_ok"] = want == 0 if not checksum else want == crc64(0, b[:-8])   # :2229-2246 (0: not checked)
    return out
