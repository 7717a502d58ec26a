"""CPU tests of the RDB load rule (include/rr_rdbload.h) as tests/rdbload_reference.py states it:
literals derived by hand next to the reference line that decides each, cross-checks against the
statements already in the tree (rdb_reference's loader, the oracle's decoder, lzf_reference), the
bound (a host function of the library) and the argument checks.  The GPU tests hold
rr_rdbload_batch to this same statement (tests/test_gpu_rdbload.py)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np

import redrock_old_amd as rr
from oracle import cpu as oracle

import lzf_reference as lzf
import rdb_reference as ref
import rdbload_reference as ld
from helpers import batch_from_blobs, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = ld.options(set_max_intset_entries=0, hash_max_ziplist_entries=0, hash_max_ziplist_value=0,
                  zset_max_ziplist_entries=0, zset_max_ziplist_value=0)
HDR = lambda t, lru=0: bytes([t]) + struct.pack("<I", lru)
S, L, SET, HASH, ZSET = rr.T_STRING, rr.T_LIST_QUICKLIST, rr.T_SET_HT, rr.T_HASH_HT, rr.T_ZSET_SKIPLIST
ISET, HZL, ZZL = rr.T_SET_INTSET, rr.T_HASH_ZIPLIST, rr.T_ZSET_ZIPLIST

NODE = (b"\x16\x00\x00\x00" b"\x11\x00\x00\x00" b"\x02\x00"   # zlbytes 22, zltail 17, zllen 2
        b"\x00\x05hello"                                         # prevlen 0 | ZIP_STR_06B 5 | bytes
        b"\x07\xC0\x00\x04"                                      # prevlen 7 | ZIP_INT_16B | 1024 LE
        b"\xFF")


def zl_of(n_entries, zllen=None):
    """A ziplist of n one-byte string entries 'a' (3 bytes each: prevlen, 0x01, 'a')."""
    body = b"".join(bytes([0 if k == 0 else 3, 1]) + b"a" for k in range(n_entries))
    tail = 10 + 3 * (n_entries - 1) if n_entries else 10
    return struct.pack("<IIH", 11 + len(body), tail, n_entries if zllen is None else zllen) + body + b"\xFF"


def intset_of(enc, vals):
    return struct.pack("<II", enc, len(vals)) + b"".join(int(v).to_bytes(enc, "little", signed=True) for v in vals)


def literal_cases():
    """(type, payload, options, expected status, expected blob or None): shared with the GPU test."""
    c = []
    add = lambda t, p, st, blob=None, o=None: c.append((t, p, o, st, blob))
    # --- rdbLoadLen, rdb.c:190-224, at a count site of a Set (thresholds 0: nothing converts)
    mem = lambda k: b"".join(b"\x01" + bytes([97 + i % 26]) for i in range(k))
    blob = lambda k: HDR(SET) + struct.pack("<Q", k) + b"".join(struct.pack("<Q", 1) + bytes([97 + i % 26]) for i in range(k))
    add(SET, b"\x05" + mem(5), 0, blob(5), ZERO)                       # :201 6 bits
    add(SET, b"\x40\x42" + mem(66), 0, blob(66), ZERO)                 # :204 14 bits: (0x40 & 0x3F) << 8 | 0x42
    add(SET, b"\x80\x00\x00\x00\x03" + mem(3), 0, blob(3), ZERO)       # :208 0x80 then u32 big-endian
    add(SET, b"\x81" + b"\x00" * 7 + b"\x02" + mem(2), 0, blob(2), ZERO)   # :213 0x81 then u64 big-endian
    add(SET, b"\xC5" + mem(5), 0, blob(5), ZERO)                       # :197-200 with isencoded NULL: 0xC5 counts 5
    add(SET, b"\x82" + mem(2), ld.E_LEN)                               # :219 unknown length encoding
    # --- the integer forms, rdb.c:266-302, as a String (enc INT + i64) and as a Set member (the text)
    add(S, b"\xC0\xFF", 0, HDR(S) + b"\x01" + struct.pack("<q", -1))                 # :273 (signed char)
    add(S, b"\xC1\x00\x80", 0, HDR(S) + b"\x01" + struct.pack("<q", -32768))         # :276 enc[0] | enc[1] << 8, int16
    add(S, b"\xC2\x00\x00\x00\x80", 0, HDR(S) + b"\x01" + struct.pack("<q", -2**31))  # :281 int32
    add(SET, b"\x02\xC0\x80\x01x", 0, HDR(SET) + struct.pack("<Q", 2) + struct.pack("<Q", 4) + b"-128" +
        struct.pack("<Q", 1) + b"x", ZERO)
    add(S, b"\xC4\x00", ld.E_LEN)                                      # :512 unknown string encoding
    # --- tryObjectEncoding, object.c:431-508
    s20, s21 = b"-9223372036854775808", b"-92233720368547758080"
    add(S, bytes([20]) + s20, 0, HDR(S) + b"\x01" + struct.pack("<q", -2**63))       # :458 len <= 20 and string2l
    add(S, bytes([21]) + s21, 0, HDR(S) + b"\x08" + s21)                             # 21 bytes: not tried; EMBSTR
    add(S, b"\x02-0", 0, HDR(S) + b"\x08-0")                                         # string2ll refuses "-0"
    add(S, b"\x03007", 0, HDR(S) + b"\x08007")                                       # and a leading zero
    add(S, b"\x0212", 0, HDR(S, 0x123456) + b"\x01" + struct.pack("<q", 12), ld.options(lru=0xFF123456))   # lru & 0xFFFFFF
    add(S, bytes([44]) + b"e" * 44, 0, HDR(S) + b"\x08" + b"e" * 44)                 # :489 len <= 44: EMBSTR
    add(S, bytes([45]) + b"r" * 45, 0, HDR(S) + b"\x00" + b"r" * 45)                 # else RAW
    add(S, b"\x00", 0, HDR(S) + b"\x08")                                             # the empty string
    # --- one two-entry List node, byte by byte: rdbLoadLen(1 node) | string(node) -> {u32 len, bytes}*
    add(L, b"\x01\x16" + NODE, 0, HDR(L) + b"\x05\x00\x00\x00hello" + b"\x04\x00\x00\x001024")
    add(L, b"\x00", 0, HDR(L))                                                       # no node: an empty body
    add(L, b"\x01\x0B" + zl_of(0), 0, HDR(L))                                        # an empty node contributes nothing
    # --- Hash and ZSet bodies
    add(HASH, b"\x01\x01f\x02vv", 0, HDR(HASH) + struct.pack("<Q", 1) + struct.pack("<Q", 1) + b"f" + struct.pack("<Q", 2) + b"vv", ZERO)
    add(ZSET, b"\x01\x01m" + struct.pack("<d", 1.5), 0, HDR(ZSET) + struct.pack("<Q", 1) + struct.pack("<Q", 1) + b"m" +
        struct.pack("<d", 1.5), ZERO)
    # --- intset and ziplists
    i3 = intset_of(2, [1, 2, 3])
    add(ISET, bytes([len(i3)]) + i3, 0, HDR(ISET) + i3)
    z2 = zl_of(2)
    add(HZL, bytes([len(z2)]) + z2, 0, HDR(HZL) + struct.pack("<Q", len(z2)) + z2)
    add(ZZL, bytes([len(z2)]) + z2, 0, HDR(ZZL) + struct.pack("<Q", len(z2)) + z2)
    # --- LZF: 0xC3 | clen | len | stream.  "aaaaaaaaaa": literal run of 1 ('a'), then a match of 9 at distance 1
    stream = b"\x00a" + bytes([(7 << 5) | 0, 0, 0])                                  # l = 7 + 0, ml = 9, off = 1
    add(S, b"\xC3\x05\x0A" + stream, 0, HDR(S) + b"\x08" + b"a" * 10)
    # --- every status once
    add(1, b"\x00", ld.E_TYPE)                                         # RDB_TYPE_LIST
    add(3, b"\x00", ld.E_TYPE); add(9, b"\x00", ld.E_TYPE); add(10, b"\x00", ld.E_TYPE); add(15, b"\x00", ld.E_TYPE)
    add(S, b"\x05abc", ld.E_TRUNC)
    add(S, b"", ld.E_TRUNC)
    add(ZSET, b"\x01\x01m\x00\x00", ld.E_TRUNC, None, ZERO)            # the score runs past the slice
    add(S, b"\xC3\x05\x0B" + stream, ld.E_LZF)                         # a declared len one more than the stream yields
    add(S, b"\x01ab", ld.E_EXTRA)
    add(L, b"\x01\x0A" + zl_of(0)[:10], ld.E_ZIPLIST)                  # a node shorter than 11 bytes
    add(ISET, b"\x07" + i3[:7], ld.E_ZIPLIST)
    add(ISET, bytes([len(i3)]) + b"\x03" + i3[1:], ld.E_ZIPLIST)       # enc 3
    add(ISET, bytes([len(i3) - 1]) + i3[:-1], ld.E_ZIPLIST)            # length != 8 + enc * n
    add(HZL, b"\x0A" + z2[:10], ld.E_ZIPLIST)
    # --- CONVERT at its threshold and one past it
    two = ld.options(set_max_intset_entries=2, hash_max_ziplist_entries=2, hash_max_ziplist_value=3,
                     zset_max_ziplist_entries=2, zset_max_ziplist_value=3)
    add(SET, b"\x02\x011\x0212", ld.E_CONVERT, None, two)              # n <= 2 and every member an integer (rdb.c:1481, :1501)
    add(SET, b"\x03\x011\x0212\x013", 0, HDR(SET) + struct.pack("<Q", 3) + b"".join(struct.pack("<Q", len(m)) + m for m in (b"1", b"12", b"3")), two)
    add(SET, b"\x02\x011\x01x", 0, HDR(SET) + struct.pack("<Q", 2) + struct.pack("<Q", 1) + b"1" + struct.pack("<Q", 1) + b"x", two)
    add(SET, b"\x00", ld.E_CONVERT, None, ZERO)                        # n == 0 stays an intset
    add(HASH, b"\x02\x01a\x03bbb\x01c\x01d", ld.E_CONVERT, None, two)  # n <= 2, lengths <= 3 (rdb.c:1567, :1586)
    h = lambda pairs: HDR(HASH) + struct.pack("<Q", len(pairs) // 2) + b"".join(struct.pack("<Q", len(m)) + m for m in pairs)
    add(HASH, b"\x02\x01a\x04bbbb\x01c\x01d", 0, h([b"a", b"bbbb", b"c", b"d"]), two)
    add(HASH, b"\x03" + b"\x01a\x01b" * 3, 0, h([b"a", b"b"] * 3), two)
    add(HASH, b"\x00", ld.E_CONVERT, None, ZERO)
    sc = struct.pack("<d", 2.0)
    z = lambda ms: HDR(ZSET) + struct.pack("<Q", len(ms)) + b"".join(struct.pack("<Q", len(m)) + m + sc for m in ms)
    add(ZSET, b"\x02\x03abc" + sc + b"\x01d" + sc, ld.E_CONVERT, None, two)   # rdb.c:1553-1554
    add(ZSET, b"\x02\x04abcd" + sc + b"\x01d" + sc, 0, z([b"abcd", b"d"]), two)
    add(ZSET, b"\x03\x01a" + sc + b"\x01b" + sc + b"\x01c" + sc, 0, z([b"a", b"b", b"c"]), two)
    add(ISET, bytes([14]) + intset_of(2, [1, 2, 3]), ld.E_CONVERT, None, two)   # header n 3 > 2 (rdb.c:1686)
    i2 = intset_of(2, [1, 2])
    add(ISET, bytes([12]) + i2, 0, HDR(ISET) + i2, two)
    z4, z6 = zl_of(4), zl_of(6)
    for t in (HZL, ZZL):
        add(t, bytes([len(z4)]) + z4, 0, HDR(t) + struct.pack("<Q", len(z4)) + z4, two)   # zllen / 2 == 2
        add(t, bytes([len(z6)]) + z6, ld.E_CONVERT, None, two)                          # 3 > 2 (rdb.c:1692, :1698)
        zf = zl_of(2, zllen=0xFFFF)
        add(t, bytes([len(zf)]) + zf, ld.E_CONVERT)                                     # zllen 0xFFFF: always
    return c


def test_length_forms():
    assert ld.Rd(b"\x3F").length() == (False, 63)                      # rdb.c:201-203
    assert ld.Rd(b"\x7F\xFF").length() == (False, 16383)               # :204-207
    assert ld.Rd(b"\x80\x00\x00\x40\x00").length() == (False, 16384)   # :208-212
    assert ld.Rd(b"\x81\x00\x00\x00\x01\x00\x00\x00\x00").length() == (False, 1 << 32)   # :213-217
    assert ld.Rd(b"\xC5").length() == (True, 5) and ld.Rd(b"\xC5").count() == 5         # :197-200, :230-235


def test_literals():
    seen = set()
    for t, p, o, st, blob in literal_cases():
        got = ld.load_blob(t, p, o)
        assert got[0] == st, (t, p, got[0], st)
        assert got[1] == blob, (t, p, got[1], blob)
        seen.add(st)
    assert seen == {0, ld.E_TYPE, ld.E_LEN, ld.E_TRUNC, ld.E_LZF, ld.E_EXTRA, ld.E_ZIPLIST, ld.E_CONVERT}


def test_lzf_node_above_the_window_is_left_to_the_cpu_path():
    ents = [bytes([97 + k % 26]) * 60 for k in range(200)]
    node = ref.list_nodes(ents, -5)[0]
    assert len(node) > ld.LZF_NODE_MAX
    comp = lzf.compress(node, len(node) - 4)
    lz = b"\xC3" + ref.save_len(len(comp)) + ref.save_len(len(node)) + comp
    assert ld.load_blob(L, b"\x01" + lz)[0] == ld.E_CONVERT
    st, blob, pay, nel = ld.load_blob(L, b"\x01" + ref.save_len(len(node)) + node)
    assert st == 0 and pay == 200 * 60 and nel == 201


def saveable(values, elems, arena):
    ab = arena.tobytes()
    for (val, descs), _ in zip(ref.flat_values(values, elems, arena), values):
        if ref.accepted_value(val, descs, len(arena)):
            yield val, (descs[:1] if val["type"] in (HZL, ZZL) else descs), ab


def opts_for(val, descs):
    """Thresholds under which the reference keeps the value's encoding: 0 for the hash-table kinds,
    the largest allowed for the compact ones."""
    if val["type"] in (SET, HASH, ZSET):
        return ZERO
    return ld.options(set_max_intset_entries=32767, hash_max_ziplist_entries=32767, zset_max_ziplist_entries=32767)


def lzf_string(s, raw):
    """lzf_reference.save_lzf_string (rdb.c:411-441 with `rdbcompression yes`), the raw form by `raw`."""
    comp = lzf.compress(s, len(s) - 4) if len(s) > 20 else None
    if comp is None:
        return raw(s)
    assert lzf.save_lzf_string(s) == b"\xC3" + ref.save_len(len(comp)) + ref.save_len(len(s)) + comp
    return lzf.save_lzf_string(s)


def crosscheck(values, elems, arena, with_lzf):
    """model(oracle decode(load_blob(save(x)))) == rdb_reference.load(type, save(x)); with_lzf: the
    same payload with its strings through lzf_reference.save_lzf_string loads to the same blob."""
    blobs, want, types = [], [], set()
    n_lzf = 0
    for val, descs, ab in saveable(values, elems, arena):
        t = val["type"]
        pay = ref.save(val, descs, ab)
        o = opts_for(val, descs)
        st, blob, _, _ = ld.load_blob(t, pay, o)
        if t in (SET, HASH) and len(descs) == 0:
            assert st == ld.E_CONVERT
            continue
        assert st == 0, (t, st)
        blobs.append(blob)
        want.append(ref.load(t, pay))
        types.add(t)
        if with_lzf:
            keep = ref.save_raw_string                 # lzf_reference.save_lzf_string's rule at every string site
            ref.save_raw_string = lambda x: lzf_string(x, keep)
            try:
                lp = ref.save(val, descs, ab)
            finally:
                ref.save_raw_string = keep
            plain, met = lzf.expand(t, lp)
            n_lzf += len(met)
            big = t == L and any(u > ld.LZF_NODE_MAX for _, u, _, _ in met)
            assert ld.load_blob(t, lp, o)[:2] == ((ld.E_CONVERT, None) if big else ld.load_blob(t, plain, o)[:2])
            assert ld.load_blob(t, plain, o)[1] == blob
    data, offs = batch_from_blobs(blobs)
    v2, e2, a2, _ = oracle.decode(data, offs)
    assert (v2["status"] == 0).all()
    ab2 = a2.tobytes()
    for (val, descs), w in zip(ref.flat_values(v2, e2, a2), want):
        used = descs[:1] if val["type"] in (HZL, ZZL) else descs
        assert ref.model(val, used, ab2) == w
    return types, n_lzf


def payload_corpus():
    g = golden()
    blobs = [bytes.fromhex(fx["blob"]) for key in ("kats", "edges", "shapes") for fx in g[key]]
    data, offs = batch_from_blobs(blobs)
    yield rr.host_decode_ex(data, offs, 0)[:3]
    data, offs = rr.gen_batch(4, 1500)
    yield rr.host_decode(data, offs)[:3]


def test_crosscheck_golden_fixtures():
    flat = next(payload_corpus())
    types, n_lzf = crosscheck(*flat, with_lzf=True)
    assert len(types) == 8


def test_crosscheck_generated_batch():
    data, offs = rr.gen_batch(4, 1500)
    types, n_lzf = crosscheck(*rr.host_decode(data, offs)[:3], with_lzf=True)
    assert len(types) >= 6 and n_lzf > 0


def test_bound_holds():
    """rr_rdbload_bound (absent from the library before this header existed) over every payload above
    and over the adversarial minimal ones."""
    lib = rr.lib()
    assert lib.rr_rdbload_bound(3, 100) == (5 * 3 + 8 * 100 + 15) & ~15
    for flat in payload_corpus():
        n = tot_p = tot_b = 0
        for val, descs, ab in saveable(*flat):
            pay = ref.save(val, descs, ab)
            st, blob, _, _ = ld.load_blob(val["type"], pay, opts_for(val, descs))
            if st == 0:
                assert len(blob) <= rr.rdbload_bound(1, len(pay))
                n, tot_p, tot_b = n + 1, tot_p + len(pay), tot_b + len(blob)
        assert n and tot_b <= rr.rdbload_bound(n, tot_p)
    for t, p, o, st, blob in literal_cases():
        if st == 0 and p[:1] != b"\xC3":
            assert len(blob) <= rr.rdbload_bound(1, len(p)), (t, p)
    ints = b"".join(bytes([0 if k == 0 else 2, 0xF1 + k]) for k in range(13))   # entries 0..12, two bytes each
    node = struct.pack("<IIH", 11 + len(ints), 10 + len(ints) - 2, 13) + ints + b"\xFF"
    for t, p in ((SET, b"\x40\xC8" + b"\x00" * 200),                             # a Set of empty strings
                 (SET, b"\x32" + b"\xC2\x00\x00\x00\x80" * 50),                  # 0xC2 members: 5 -> 8 + 11
                 (L, b"\x01" + bytes([len(node)]) + node)):                      # List nodes of integers 0..12
        st, blob, _, _ = ld.load_blob(t, p, ZERO)
        assert st == 0 and len(blob) <= rr.rdbload_bound(1, len(p))
    assert len(ld.load_blob(SET, b"\x40\xC8" + b"\x00" * 200, ZERO)[1]) == 5 + 8 * 202 - 8   # 8 per payload byte but the count's second


def test_argument_checks():
    """An unknown flag bit and an *_entries of 32768 give RR_API_EINVAL from both calls, before
    anything else is looked at (no context is needed to see it)."""
    lib = rr.lib()
    offs = np.zeros(1, np.uint64)
    t = rr.Totals()
    ib, ob = rr.BlobBatch(), rr.BlobBatch()

    def host(o):
        rc = lib.rr_rdbload_batch_host(None, None, rr._ptr(offs), None, 0, C.byref(o), None, 0, rr._ptr(offs), None, C.byref(t))
        return rc, lib.rr_last_error().decode()

    def dev(o):
        rc = lib.rr_rdbload_batch(None, C.byref(ib), None, C.byref(ob), None, None, C.byref(o), None)
        return rc, lib.rr_last_error().decode()

    for call in (host, dev):
        rc, msg = call(rr.RdbLoadOpts(flags=1))
        assert rc == rr.API_EINVAL and "flags" in msg
        for field in ("set_max_intset_entries", "hash_max_ziplist_entries", "zset_max_ziplist_entries"):
            rc, msg = call(rr.RdbLoadOpts(**{field: 32768}))
            assert rc == rr.API_EINVAL and "32767" in msg
        rc, msg = call(rr.RdbLoadOpts(**{"set_max_intset_entries": 32767, "hash_max_ziplist_value": 1 << 31}))
        assert rc == rr.API_EINVAL and "NULL" in msg           # the options pass; the missing context is next


def test_library_exports_every_rdbload_symbol():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rr_rdbload.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(rr_[a-z_0-9]+)\s*\(", txt)))
    assert len(syms) == 3 and all(s.startswith("rr_rdbload_") for s in syms)
    lib = rr.lib()
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/rr_rdbload.h but not exported"
    assert sorted(rr.RDBLOAD_EXPORTS) == syms
    assert C.sizeof(rr.RdbLoadOpts) == 28
    d = rr.RdbLoadOpts()
    assert {k: getattr(d, k) for k in ld.DEFAULTS} == ld.DEFAULTS and d.flags == 0


def test_rdbload_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rr_rdbload.h"\n'
                   'int main(void){ rr_rdbload_opts o = {0, 512, 512, 64, 128, 64, 0};\n'
                   '  return (RR_RDBLOAD_E_TYPE == 32 && RR_RDBLOAD_E_CONVERT == 38 && RR_RDBLOAD_E_TYPE > RR_N_STATUS\n'
                   '          && sizeof o == 28 && o.flags == 0) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0
