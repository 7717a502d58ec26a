"""CPU tests of the conversion rule (include/rr_rdbconvert.h) as tests/rdbconvert_reference.py states it:
literals written out by hand from ziplist.c / intset.c, the same cases through the oracle's decoder
against rdb_reference.load, every RR_RDBLOAD_E_CONVERT value of the corpora the load tests use, the
bound and the argument checks.  The GPU tests hold rr_rdbconvert_batch to this same statement
(tests/test_gpu_rdbconvert.py)."""
import collections
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np

import redrock_old_amd as rr
from oracle import pyoracle

import lzf_reference as lzf
import rdb_reference as ref
import rdbconvert_reference as cv
import rdbload_mutants as mut
import rdbload_reference as ld
import test_rdbload as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = lambda t, lru=0: bytes([t]) + struct.pack("<I", lru)
S, L, SET, HASH, ZSET = rr.T_STRING, rr.T_LIST_QUICKLIST, rr.T_SET_HT, rr.T_HASH_HT, rr.T_ZSET_SKIPLIST
ISET, HZL, ZZL = rr.T_SET_INTSET, rr.T_HASH_ZIPLIST, rr.T_ZSET_ZIPLIST
raw = lambda b: ref.save_len(len(b)) + b
dbl = lambda x: struct.pack("<d", x)
ZL = lambda zlbytes, zltail, zllen, body: struct.pack("<Q", zlbytes) + struct.pack("<IIH", zlbytes, zltail, zllen) + body + b"\xFF"
BIG = float(2**52 - 1)


def literal_cases():
    """(type, payload, options, expected status, expected blob or None): shared with the GPU test."""
    c = []
    add = lambda t, p, st, blob=None, o=None: c.append((t, p, o, st, blob))
    # --- the empty values: intsetNew (intset.c:97-102), ziplistNew (ziplist.c:578-586)
    add(SET, b"\x00", 0, HDR(ISET) + b"\x02\x00\x00\x00" b"\x00\x00\x00\x00")
    empty = b"\x0B\x00\x00\x00" b"\x0A\x00\x00\x00" b"\x00\x00" b"\xFF"
    add(HASH, b"\x00", 0, HDR(HZL) + struct.pack("<Q", 11) + empty)
    add(ZSET, b"\x00", 0, HDR(ZZL, 0x123456) + struct.pack("<Q", 11) + empty, ld.options(lru=0xFF123456))
    # --- intsets: ascending, a value already there dropped, the narrowest width for all (intset.c:45-52)
    add(SET, b"\x04" + raw(b"3") + raw(b"1") + raw(b"3") + raw(b"-129"), 0,
        HDR(ISET) + b"\x02\x00\x00\x00" b"\x03\x00\x00\x00" b"\x7F\xFF" b"\x01\x00" b"\x03\x00")
    add(SET, b"\x01" + raw(b"32768"), 0, HDR(ISET) + b"\x04\x00\x00\x00" b"\x01\x00\x00\x00" b"\x00\x80\x00\x00")
    add(SET, b"\x01" + raw(b"2147483648"), 0,
        HDR(ISET) + b"\x08\x00\x00\x00" b"\x01\x00\x00\x00" b"\x00\x00\x00\x80\x00\x00\x00\x00")
    add(SET, b"\x03\xC0\xFB" + raw(b"70000") + b"\xC1\x00\x80", 0,         # the integer forms: -5, 70000, -32768 -> enc 4
        HDR(ISET) + b"\x04\x00\x00\x00" b"\x03\x00\x00\x00" + struct.pack("<iii", -32768, -5, 70000))
    # --- a Hash pair: prevlen 0 | ZIP_STR_06B 1 | 'a', then prevlen 3 | 0xF1 + 12
    add(HASH, b"\x01" + raw(b"a") + raw(b"12"), 0, HDR(HZL) + ZL(16, 13, 2, b"\x00\x01a" b"\x03\xFD"))
    # --- the six integer encodings at their borders (ziplist.c:487-498), one entry behind the other
    ints = [b"12", b"13", b"127", b"128", b"32767", b"32768", b"8388607", b"8388608", b"2147483647", b"2147483648"]
    body = (b"\x00\xFD"                                    # 12: 0xF1 + 12
            b"\x02\xFE\x0D"                                # 13: int8
            b"\x03\xFE\x7F"                                # 127
            b"\x03\xC0\x80\x00"                            # 128: int16
            b"\x04\xC0\xFF\x7F"                            # 32767
            b"\x04\xF0\x00\x80\x00"                        # 32768: int24
            b"\x05\xF0\xFF\xFF\x7F"                        # 2^23 - 1
            b"\x05\xD0\x00\x00\x80\x00"                    # 2^23: int32
            b"\x06\xD0\xFF\xFF\xFF\x7F"                    # 2^31 - 1
            b"\x06\xE0\x00\x00\x00\x80\x00\x00\x00\x00")   # 2^31: int64
    assert len(body) == 48
    add(HASH, b"\x05" + b"".join(raw(x) for x in ints), 0, HDR(HZL) + ZL(59, 48, 10, body))
    # --- 31 digits: zipTryEncoding looks (len < 32) and string2ll refuses; a string entry
    d31 = b"1" * 31
    add(HASH, b"\x01" + raw(b"f") + raw(d31), 0, HDR(HZL) + ZL(47, 13, 2, b"\x00\x01f" b"\x03\x1F" + d31))
    add(HASH, b"\x01" + raw(b"-0") + raw(b"007"), 0, HDR(HZL) + ZL(20, 14, 2, b"\x00\x02-0" b"\x04\x03007"))
    # --- a ZSet: zslInsert's order, d2string's text.  -inf | -0 == 0, "n" < "p" | 5: "ab" < "abc" < "b" | 7 (the
    # member "p" a second time) | 2^52 - 1 | inf
    pay = b"\x09" + b"".join(raw(m) + dbl(s) for m, s in (
        (b"b", 5.0), (b"z", float("inf")), (b"abc", 5.0), (b"p", 0.0), (b"ab", 5.0), (b"n", -0.0), (b"m", float("-inf")),
        (b"big", BIG), (b"p", 7.0)))
    body = (b"\x00\x01m" b"\x03\x04-inf"
            b"\x06\x01n" b"\x03\x02-0"
            b"\x04\x01p" b"\x03\xF1"
            b"\x02\x02ab" b"\x04\xF6"
            b"\x02\x03abc" b"\x05\xF6"
            b"\x02\x01b" b"\x03\xF6"
            b"\x02\x01p" b"\x03\xF8"
            b"\x02\x03big" b"\x05\xE0\xFF\xFF\xFF\xFF\xFF\xFF\x0F\x00"
            b"\x0A\x01z" b"\x03\x03inf")
    assert len(body) == 67
    add(ZSET, pay, 0, HDR(ZZL) + ZL(78, 72, 18, body))
    add(ZSET, b"\x02" + b"\xC0\x11" + dbl(17.0) + raw(b"x") + dbl(-3.0), 0,    # an integer-form member, "17" an integer entry
        HDR(ZZL) + ZL(23, 19, 4, b"\x00\x01x" b"\x03\xFE\xFD" b"\x03\xFE\x11" b"\x03\xFE\x11"))
    # --- what stays RR_RDBLOAD_E_CONVERT (the deviations of rr_rdbconvert.h)
    for sc in (1.5, float(2**52), -BIG, 1e300, 5e-324):
        add(ZSET, b"\x01" + raw(b"m") + dbl(sc), cv.E_CONVERT)               # d2string would print %.17g
    add(ZSET, b"\x01" + raw(b"m") + dbl(float("nan")), cv.E_CONVERT)         # t_zset.c:137
    add(ZSET, b"\x01" + mut.lz(b"ab" * 18) + dbl(1.0), cv.E_CONVERT)         # an LZF member
    i3 = tl.intset_of(2, [1, 2, 3])
    two = ld.options(set_max_intset_entries=2, hash_max_ziplist_entries=2, zset_max_ziplist_entries=2)
    add(ISET, raw(i3), cv.E_CONVERT, None, two)                              # the reverse conversions
    add(HZL, raw(tl.zl_of(6)), cv.E_CONVERT, None, two)
    add(ZZL, raw(tl.zl_of(2, zllen=0xFFFF)), cv.E_CONVERT)
    return c


def over_max_n():
    """A Set and a ZSet of RR_RDBCONVERT_MAX_N + 1 members under thresholds raised above it."""
    o = ld.options(set_max_intset_entries=1000, zset_max_ziplist_entries=1000)
    n = cv.MAX_N + 1
    return o, [(SET, ref.save_len(n) + b"".join(raw(str(k).encode()) for k in range(n))),
               (ZSET, ref.save_len(n) + b"".join(raw(str(k).encode()) + dbl(float(k)) for k in range(n)))]


def test_literals():
    seen = collections.Counter()
    for t, p, o, st, blob in literal_cases():
        assert ld.load_blob(t, p, o)[0] == ld.E_CONVERT, (t, p)      # each is a value the second stage is handed
        got = cv.convert_blob(t, p, o)
        assert got[0] == st, (t, p, got[0], st)
        assert got[2] == blob, (t, p, got[2], blob)
        if st == 0:
            assert got[1] == blob[0]
            seen[blob[0]] += 1
    assert set(seen) == {ISET, HZL, ZZL}
    o, vals = over_max_n()
    for t, p in vals:
        assert ld.load_blob(t, p, o)[0] == ld.E_CONVERT and cv.convert_blob(t, p, o)[0] == cv.E_CONVERT
    at_max = [(SET, ref.save_len(cv.MAX_N) + b"".join(raw(str(k).encode()) for k in range(cv.MAX_N))),
              (ZSET, ref.save_len(cv.MAX_N) + b"".join(raw(str(k).encode()) + dbl(float(k)) for k in range(cv.MAX_N)))]
    for t, p in at_max:
        assert cv.convert_blob(t, p, o)[0] == 0


def test_d2string():
    bits = lambda x: struct.unpack("<Q", struct.pack("<d", x))[0]
    assert cv.d2string(bits(0.0)) == b"0" and cv.d2string(bits(-0.0)) == b"-0"          # util.c:525-530
    assert cv.d2string(bits(float("inf"))) == b"inf" and cv.d2string(bits(float("-inf"))) == b"-inf"
    assert cv.d2string(bits(BIG)) == b"4503599627370495" and cv.d2string(bits(float(2**52))) is None   # value < max
    assert cv.d2string(bits(-float(2**52 - 2))) == b"-4503599627370494" and cv.d2string(bits(-BIG)) is None   # value > min
    assert cv.d2string(bits(17.0)) == b"17" and cv.d2string(bits(1.5)) is None and cv.d2string(bits(float("nan"))) is None


def members_of(blob):
    """The converted blob through the oracle's decoder: its members / pairs / (member, score) as a multiset."""
    val, elems = pyoracle.decode_one(blob, 0)
    assert val["status"] == 0, val
    text = lambda e: blob[e[1]:e[1] + e[2]] if e[0] == rr.K_STR else str(e[1]).encode()
    if blob[0] == ISET:
        return collections.Counter(text(e) for e in elems)
    ents = [text(e) for e in elems[1:]]                               # elems[0] is the whole ziplist
    if blob[0] == HZL:
        return collections.Counter(zip(ents[0::2], ents[1::2]))
    return collections.Counter((m, struct.pack("<d", float(s))) for m, s in zip(ents[0::2], ents[1::2]))


def loaded_members(typ, payload):
    kind, items = ref.load(typ, payload)
    if typ == SET:
        return collections.Counter(set(items))                        # intsetAdd drops a value already there
    if typ == HASH:
        return collections.Counter(zip(items[0::2], items[1::2]))
    return collections.Counter((m, struct.pack("<Q", b)) for m, b in zip(items[0::2], items[1::2]))


def test_literals_decode_to_what_the_loader_reads():
    n = 0
    for t, p, o, st, blob in literal_cases():
        if st == 0:
            assert members_of(cv.convert_blob(t, p, o)[2]) == loaded_members(t, p), (t, p)
            n += 1
    assert n >= 12


def documented_stay(typ, payload):
    """Is this RR_RDBLOAD_E_CONVERT value one the header leaves to the CPU path?  Told from the payload
    alone, not through convert_blob."""
    if typ in (ISET, HZL, ZZL, L):                                     # the reverse conversions; oversize LZF nodes
        return True
    if typ == HASH:
        return False
    r = ld.Rd(payload)
    n = r.count()
    if n > cv.MAX_N:
        return True
    if typ == ZSET:
        for _ in range(n):
            if ld.is_lzf_at(payload, r.p):
                return True
            r.string()
            v = struct.unpack("<d", r.take(8))[0]
            if v != v or not (v in (float("inf"), float("-inf")) or (v == int(v) and -BIG < v < 2.0**52)):
                return True
    return False


def convert_seeds():
    """Every RR_RDBLOAD_E_CONVERT value of the load tests' corpora: (type, payload, options)."""
    types, pays, _ = mut.corpus()
    out = [(t, p, mut.OPTS) for t, p in zip(types, pays) if ld.load_blob(t, p, mut.OPTS)[0] == ld.E_CONVERT]
    out += [(t, p, o) for t, p, o, st, _ in tl.literal_cases() if st == ld.E_CONVERT]
    return out


def test_every_convert_value_of_the_load_corpora():
    seeds = convert_seeds()
    stays = conv = 0
    kinds = set()
    for t, p, o in seeds:
        st, nt, blob, _, _ = cv.convert_blob(t, p, o)
        assert st in (0, cv.E_CONVERT)                                 # RR_E_CAPACITY is the batch's
        assert (st == cv.E_CONVERT) == documented_stay(t, p), (t, p, st)
        if st == 0:
            assert members_of(blob) == loaded_members(t, lzf.expand(t, p)[0]), (t, p)   # (rdb_reference.load reads no LZF)
            conv += 1
            kinds.add(nt)
        else:
            stays += 1
    assert len(seeds) > 100 and stays and kinds == {ISET, HZL, ZZL}, (len(seeds), stays, conv, kinds)


def test_bound_holds():
    assert rr.lib().rr_rdbconvert_bound(3, 100) == (24 * 3 + 4 * 100 + 15) & ~15
    for t, p, o, st, blob in literal_cases():
        if st == 0 and b"\xC3" not in p:
            assert len(blob) <= rr.rdbconvert_bound(1, len(p)), (t, p)
    worst = [(SET, b"\x02\xC0\x01" + raw(b"-9223372036854775808")),            # 2 payload bytes -> 8
             (HASH, b"\x20" + b"\x00" * 64),                                    # empty strings: 1 -> 2
             (HASH, b"\x01" + raw(b"x" * 250) + raw(b"")),                      # a 5-byte prevlen behind 254 bytes
             (ZSET, b"\x01\x00" + dbl(-BIG + 1))]                               # 8 score bytes -> 10
    for t, p in worst:
        st, _, blob, _, _ = cv.convert_blob(t, p, ld.options(hash_max_ziplist_value=1000))
        assert st == 0 and len(blob) <= rr.rdbconvert_bound(1, len(p)), (t, len(blob))


def test_argument_checks():
    """Bad options give RR_API_EINVAL from both calls before anything else is looked at; a NULL context
    after that."""
    lib = rr.lib()
    offs = np.zeros(1, np.uint64)
    t = rr.Totals()
    ib, ob = rr.BlobBatch(), rr.BlobBatch()

    def host(o):
        rc = lib.rr_rdbconvert_batch_host(None, None, rr._ptr(offs), None, None, 0, o, None, 0, rr._ptr(offs), None, None,
                                          C.byref(t))
        return rc, lib.rr_last_error().decode()

    def dev(o):
        rc = lib.rr_rdbconvert_batch(None, C.byref(ib), None, None, C.byref(ob), None, None, None, o, None)
        return rc, lib.rr_last_error().decode()

    for call in (host, dev):
        rc, msg = call(C.byref(rr.RdbLoadOpts(flags=1)))
        assert rc == rr.API_EINVAL and "flags" in msg
        for field in ("set_max_intset_entries", "hash_max_ziplist_entries", "zset_max_ziplist_entries"):
            rc, msg = call(C.byref(rr.RdbLoadOpts(**{field: 32768})))
            assert rc == rr.API_EINVAL and "32767" in msg
        for o in (None, C.byref(rr.RdbLoadOpts(hash_max_ziplist_value=1 << 31))):
            rc, msg = call(o)
            assert rc == rr.API_EINVAL and "NULL" in msg               # the options pass; the missing context is next


def test_library_exports_every_rdbconvert_symbol():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rr_rdbconvert.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(rr_[a-z_0-9]+)\s*\(", txt)))
    assert len(syms) == 3 and all(s.startswith("rr_rdbconvert_") for s in syms)
    lib = rr.lib()
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/rr_rdbconvert.h but not exported"
        assert getattr(lib, s).argtypes, f"{s} not bound"
    assert sorted(rr.RDBCONVERT_EXPORTS) == syms
    for name, py in (("RR_RDBCONVERT_SKIP", rr.RDBCONVERT_SKIP), ("RR_RDBCONVERT_MAX_N", rr.RDBCONVERT_MAX_N),
                     ("RR_RDBCONVERT_MAX_WAVES", rr.RDBCONVERT_MAX_WAVES)):
        assert int(re.search(rf"#define {name}\s+(\d+)", txt).group(1)) == py
    assert (rr.RDBCONVERT_SKIP, rr.RDBCONVERT_MAX_N, rr.RDBCONVERT_MAX_WAVES) == (cv.SKIP, cv.MAX_N, cv.MAX_WAVES)
    assert rr.RDBCONVERT_MAX_N >= 512


def test_rdbconvert_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rr_rdbconvert.h"\n'
                   'int main(void){ rr_rdbload_opts o = {0, 512, 512, 64, 128, 64, 0};\n'
                   '  return (RR_RDBCONVERT_SKIP == 45 && RR_RDBCONVERT_SKIP > RR_RDBLOAD_E_CONVERT && RR_RDBCONVERT_MAX_N >= 512\n'
                   '          && RR_RDBCONVERT_MAX_WAVES % 4 == 0 && o.flags == 0) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0
