"""CPU tests of the third stage's rule (include/rr_rdbzset.h) as tests/rdbzset_reference.py states it:
blobs written out by hand, every reference blob through the oracle's decoder against what
rdb_reference.load reads, integer-only values against rdbconvert_reference, the bound and the argument
checks.  The GPU tests hold rr_rdbzset_batch to this same statement (tests/test_gpu_rdbzset.py)."""
import collections
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np

import redrock_old_amd as rr
from oracle import pyoracle

import rdb_reference as ref
import rdbconvert_reference as cv
import rdbload_reference as ld
import rdbzset_reference as zr
from rdbload_mutants import lz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZSET, ZZL = rr.T_ZSET_SKIPLIST, rr.T_ZSET_ZIPLIST
HDR = lambda t, lru=0: bytes([t]) + struct.pack("<I", lru)
raw = lambda b: ref.save_len(len(b)) + b
dbl = lambda x: struct.pack("<d", x)
ZL = lambda zlbytes, zltail, zllen, body: struct.pack("<Q", zlbytes) + struct.pack("<IIH", zlbytes, zltail, zllen) + body + b"\xFF"


def zset(pairs):
    return ref.save_len(len(pairs)) + b"".join(raw(m) + dbl(s) for m, s in pairs)


def literal_cases():
    """(payload, options, expected status, expected blob or None): shared with the GPU test."""
    c = []
    add = lambda p, st, blob=None, o=None: c.append((p, o, st, blob))
    add(zset([(b"a", 1.5)]), 0, HDR(ZZL) + ZL(19, 13, 2, b"\x00\x01a" b"\x03\x031.5"))
    # 2^52 prints as an integer and passes string2ll: an 0xE0 entry; 1e17 prints as "1e+17" and stays a string
    body = (b"\x00\x01a" b"\x03\xE0" + struct.pack("<q", 1 << 52) +
            b"\x0A\x01b" b"\x03\x051e+17")
    assert len(body) == 23
    add(zset([(b"b", 1e17), (b"a", 2.0**52)]), 0, HDR(ZZL, 0x345678) + ZL(34, 26, 4, body), ld.options(lru=0x12345678))
    # -0.1 | -0 == 0, "c" < "d" | 0.1
    body = (b"\x00\x01b" b"\x03\x14-0.10000000000000001"
            b"\x16\x01c" b"\x03\x02-0"
            b"\x04\x01d" b"\x03\xF1"
            b"\x02\x01a" b"\x03\x130.10000000000000001")
    assert len(body) == 61
    add(zset([(b"a", 0.1), (b"b", -0.1), (b"c", -0.0), (b"d", 0.0)]), 0, HDR(ZZL) + ZL(72, 50, 8, body))
    add(b"\x00", 0, HDR(ZZL) + struct.pack("<Q", 11) + b"\x0B\x00\x00\x00" b"\x0A\x00\x00\x00" b"\x00\x00" b"\xFF")
    # --- what stays RR_RDBLOAD_E_CONVERT
    add(zset([(b"a", 1.5), (b"m", float("nan"))]), zr.E_CONVERT)                 # t_zset.c:137
    add(b"\x01" + lz(b"ab" * 18) + dbl(1.5), zr.E_CONVERT)                       # an LZF member
    add(zset([(b"a", 1.5), (b"b", 2.5), (b"c", 3.5)]), zr.E_CONVERT, None, ld.options(zset_max_ziplist_entries=2))
    add(zset([(b"abcd", 1.5)]), zr.E_CONVERT, None, ld.options(zset_max_ziplist_value=3))
    add(zset([(b"a", 1.5)])[:-3], zr.E_CONVERT)                                  # truncated inside the score
    add(zset([(b"a", 1.5)]) + b"\x00", zr.E_CONVERT)                             # a byte left over
    return c


def test_literals():
    for p, o, st, blob in literal_cases():
        got = zr.zset_blob(p, o)
        assert got[0] == st and got[1] == blob, (p, got[:2], blob)
    blob = zr.zset_blob(literal_cases()[1][0])[1]
    assert blob[13 + 10 + 3 + 1] == 0xE0                                         # the 2^52 score
    for v, text in ((2.0**53, b"9007199254740992"), (1e16, b"10000000000000000")):
        b = zr.zset_blob(zset([(b"a", v)]))[1]
        assert zr.d2string(zr.to_bits(v)) == text and b[13 + 10 + 3 + 1] == 0xE0 and struct.unpack("<q", b[28:36])[0] == int(v)
    over = zset([(b"%d" % k, k + 0.5) for k in range(cv.MAX_N + 1)])
    o = ld.options(zset_max_ziplist_entries=1000)
    assert zr.zset_blob(over, o)[0] == zr.E_CONVERT
    assert zr.zset_blob(zset([(b"%d" % k, k + 0.5) for k in range(cv.MAX_N)]), o)[0] == 0


def decoded(blob):
    """The blob through the oracle's faithful desObject port: (member, score text) as a multiset."""
    val, elems = pyoracle.decode_one(blob, 0)
    assert val["status"] == 0 and blob[0] == ZZL, val
    text = lambda e: blob[e[1]:e[1] + e[2]] if e[0] == rr.K_STR else str(e[1]).encode()
    ents = [text(e) for e in elems[1:]]                               # elems[0] is the whole ziplist
    return collections.Counter(zip(ents[0::2], ents[1::2]))


def loaded(payload):
    kind, items = ref.load(ZSET, payload)
    return collections.Counter((m, zr.d2string(b)) for m, b in zip(items[0::2], items[1::2]))


def random_zsets(seed=9, n=60):
    rng = np.random.default_rng(seed)
    edge = zr.edge_scores()
    edge = edge[(edge & np.uint64(0x7FFFFFFFFFFFFFFF)) <= np.uint64(0x7FF0000000000000)]   # no NaN
    out = []
    for k in range(n):
        cnt = int(rng.integers(1, 40))
        pairs = []
        for j in range(cnt):
            s = zr.to_double(int(edge[int(rng.integers(0, len(edge)))])) if rng.integers(0, 3) else float(rng.integers(-5, 5)) / 4
            m = (b"%d" % rng.integers(-300, 300)) if rng.integers(0, 4) == 0 else bytes(rng.integers(97, 100, int(rng.integers(0, 6)), dtype=np.uint8))
            pairs.append((m, s))
        out.append(zset(pairs))
    return out


def test_reference_blobs_decode_to_what_the_loader_reads():
    n = 0
    for p in [c[0] for c in literal_cases() if c[2] == 0 and c[1] is None] + random_zsets():
        st, blob, pay, nel = zr.zset_blob(p)
        assert st == 0 and decoded(blob) == loaded(p), p
        n += 1
    assert n > 60


def test_integer_scores_give_rdbconvert_bytes():
    rng = np.random.default_rng(3)
    specials = [float("inf"), float("-inf"), 0.0, -0.0, float(2**52 - 1), -float(2**52 - 2), 12.0, 13.0, -129.0, 70000.0]
    for k in range(40):
        pairs = [(b"m%d" % j, specials[int(rng.integers(0, len(specials)))] if rng.integers(0, 2) else float(rng.integers(-2**40, 2**40)))
                 for j in range(int(rng.integers(1, 30)))]
        p = zset(pairs)
        st, t, blob, pay, nel = cv.convert_blob(ZSET, p)
        assert st == 0 and zr.zset_blob(p) == (0, blob, pay, nel)


def test_bound_holds():
    assert rr.lib().rr_rdbzset_bound(3, 100) == (24 * 3 + 4 * 100 + 15) & ~15
    o = ld.options(zset_max_ziplist_value=1000)
    worst = [zset([(b"", -5e-324)] * 100),                                       # 1 + 8 -> 2 + 26
             zset([(b"", -5e-324)]),
             zset([(b"x" * 250, -5e-324), (b"x" * 251, -1e-310)]),               # a 5-byte prevlen in front of a printed score
             zset([(b"\xFF" * 64, -2.2250738585072014e-308)])]
    for p in worst:
        st, blob, _, _ = zr.zset_blob(p, o)
        assert st == 0 and len(blob) <= rr.rdbzset_bound(1, len(p)), (len(blob), len(p))
    for p, o, st, blob in literal_cases():
        if st == 0:
            assert len(blob) <= rr.rdbzset_bound(1, len(p))
    assert len(zr.zset_blob(worst[1], o)[1]) == 24 + 28                          # the worst-case line of the header


def test_argument_checks():
    """Bad options give RR_API_EINVAL from both calls before anything else is looked at; a NULL context
    after that.  The error texts are rr_rdbload_batch's."""
    lib = rr.lib()
    offs = np.zeros(1, np.uint64)
    t = rr.Totals()
    ib, ob = rr.BlobBatch(), rr.BlobBatch()

    def host(o):
        rc = lib.rr_rdbzset_batch_host(None, None, rr._ptr(offs), None, None, 0, o, None, 0, rr._ptr(offs), None, C.byref(t))
        return rc, lib.rr_last_error().decode()

    def dev(o):
        rc = lib.rr_rdbzset_batch(None, C.byref(ib), None, None, C.byref(ob), None, None, o, None)
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
    one = np.zeros(1, np.uint64)
    assert lib.rr_d2string_batch_host(None, rr._ptr(one), 1, rr._ptr(one), rr._ptr(one)) == rr.API_EINVAL
    assert lib.rr_d2string_batch(None, None, 0, None, None, None) == rr.API_EINVAL


def test_library_exports_every_rdbzset_symbol():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rr_rdbzset.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(rr_[a-z_0-9]+)\s*\(", txt)))
    assert len(syms) == 3 and all(s.startswith("rr_rdbzset_") for s in syms)
    lib = rr.lib()
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/rr_rdbzset.h but not exported"
        assert getattr(lib, s).argtypes, f"{s} not bound"
    assert sorted(rr.RDBZSET_EXPORTS) == syms
    assert int(re.search(r"#define RR_RDBZSET_SKIP\s+(\d+)", txt).group(1)) == rr.RDBZSET_SKIP == zr.SKIP == 55


def test_rdbzset_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rr_rdbzset.h"\n#include "rr_d2string.h"\n'
                   'int main(void){ rr_rdbload_opts o = {0, 512, 512, 64, 128, 64, 0};\n'
                   '  return (RR_RDBZSET_SKIP == 55 && RR_RDBZSET_SKIP != RR_RDBCONVERT_SKIP && RR_RDBZSET_SKIP > RR_RDBLOAD_E_CONVERT\n'
                   '          && o.flags == 0) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0
