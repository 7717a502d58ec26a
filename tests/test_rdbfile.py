"""CPU tests of the RDB stream framing and the CRC-64 (include/rr_rdbfile.h) as
tests/rdbfile_reference.py states them: the check values, the library's host helpers (rr_crc64,
rr_crc64_shift, rr_rdbfile_head, rr_rdbfile_selectdb) against that statement, the reference's own
writer and parser over the golden fixtures' payloads, and the stand-alone host check program (a plain
build; tools/rdbfile_host_check.c names the sanitizer build).  The
GPU tests hold the kernels to this same statement (tests/test_gpu_rdbfile.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import redrock_old_amd as rr
from oracle import cpu as oracle

import rdb_reference as ref
import rdbfile_reference as rf
from helpers import batch_from_blobs, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- check values --------------------------------------------------------------------------------
def test_check_values():
    assert rf.crc64(0, b"123456789") == 0xE9C6D914C4B8D9CA
    assert rf.TABLE[1] == 0x7AD870C830358979 and rf.TABLE[2] == 0xF5B0E190606B12F2
    assert rf.dump(rr.T_STRING, ref.save_raw_string(b"a")) == bytes.fromhex("0001610900" "6f0cbe57dbb01e05")
    assert rr.crc64(0, b"123456789") == 0xE9C6D914C4B8D9CA


def test_reference_long_path_equals_the_loop():
    rng = np.random.default_rng(5)
    for n in (1 << 14, (1 << 14) + 1, 40000):
        d = rng.integers(0, 256, n, dtype=np.uint8)
        for c in (0, 0xDEADBEEF12345678):
            assert rf.crc64(c, d) == rf.crc64_simple(c, d.tobytes())


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 4097])
def test_rr_crc64_equals_reference(n):
    rng = np.random.default_rng(100 + n)
    buf = rng.integers(0, 256, n + 32, dtype=np.uint8)
    for mis in range(16):
        d = buf[mis:mis + n]
        want0 = rf.crc64_simple(0, d.tobytes())
        assert int(rr.lib().rr_crc64(0, buf.ctypes.data + mis, n)) == want0
        init = 0x0123456789ABCDEF
        assert int(rr.lib().rr_crc64(init, buf.ctypes.data + mis, n)) == rf.crc64_simple(init, d.tobytes())


def test_combine_identities():
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, 256, 301, dtype=np.uint8).tobytes(), rng.integers(0, 256, 1234, dtype=np.uint8).tobytes()
    c = 0xFEEDFACECAFEBEEF
    for crc, sh in ((rf.crc64, rf.shift), (rr.crc64, rr.crc64_shift)):
        assert crc(0, a + b) == sh(crc(0, a), len(b)) ^ crc(0, b)
        assert crc(c, b) == crc(0, b) ^ sh(c, len(b))
        assert sh(c, 77) == crc(c, bytes(77))
    assert rr.crc64_shift(c, 1 << 33) == rf.shift(c, 1 << 33)
    assert rf.crc64(0, bytes(1000) + a) == rf.crc64(0, a)          # zero bytes in front of state 0


def test_exports_and_constants():
    L = rr.lib()
    for name in rr.RDBFILE_EXPORTS:
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "rr_rdbfile.h")).read()
    for sym, val in (("RR_RDBFILE_IDLE", rr.RDBFILE_IDLE), ("RR_RDBFILE_FREQ", rr.RDBFILE_FREQ), ("RR_RDBFILE_EOF", rr.RDBFILE_EOF),
                     ("RR_RDBFILE_NO_CKSUM", rr.RDBFILE_NO_CKSUM), ("RR_RDBFILE_E_VALUE", rr.RDBFILE_E_VALUE),
                     ("RR_RDBFILE_E_KEY", rr.RDBFILE_E_KEY), ("RR_RDBDUMP_E_SHORT", rr.RDBDUMP_E_SHORT),
                     ("RR_RDBDUMP_E_VERSION", rr.RDBDUMP_E_VERSION), ("RR_RDBDUMP_E_CRC", rr.RDBDUMP_E_CRC),
                     ("RR_CRC64_RUN", rr.CRC64_RUN), ("RR_CRC64_MAX_WAVES", rr.CRC64_MAX_WAVES),
                     ("RR_RDBDUMP_MAX_WAVES", rr.RDBDUMP_MAX_WAVES)):
        m = re.search(rf"#define {sym}\s+(\d+)u?\b", hdr)
        assert m and int(m.group(1)) == val, sym
    assert rr.CRC64_PIECE == 64 * rr.CRC64_RUN and "#define RR_CRC64_PIECE      (64u * RR_CRC64_RUN)" in hdr
    assert rr.rdbfile_bound(3, 10, 100, 7) == (7 + 27 * 3 + 10 + 100 + 9 + 15) & ~15


# ---- head and selectdb ---------------------------------------------------------------------------
REPL = (3, "0123456789abcdef0123456789abcdef01234567", 123456789012)


@pytest.mark.parametrize("repl", [None, REPL, (-1, "x" * 40, 0)])
@pytest.mark.parametrize("ctime,used", [(1700000000, 5_000_000_000), (0, 0), (127, 128), (32768, 2147483647), (2147483648, 1 << 40)])
def test_head(repl, ctime, used):
    for aof in (False, True):
        want = rf.head("6.0.20", ctime, used, repl, aof)
        need, got = rr.rdbfile_head("6.0.20", ctime, used, repl, aof)
        assert need == len(want) and got == want
        need, got = rr.rdbfile_head("6.0.20", ctime, used, repl, aof, cap=len(want) - 1)   # too small: the size, nothing written
        assert need == len(want) and got == b"\xA5" * (len(want) - 1)
        need, got = rr.rdbfile_head("6.0.20", ctime, used, repl, aof, cap=len(want) + 8)
        assert got == want + b"\xA5" * 8
    assert want[9:9 + 11 + 7] == b"\xFA\x09redis-ver\x066.0.20" and b"\xFA\x0Aredis-bits\xC0\x40" in want


@pytest.mark.parametrize("dbid", [0, 63, 64, 16383, 16384])
def test_selectdb(dbid):
    for size, exp in ((0, 0), (10, 2), (16384, 70000), (1 << 32, (1 << 32) - 1), (1 << 40, 1 << 63)):
        want = rf.selectdb(dbid, size, exp)
        need, got = rr.rdbfile_selectdb(dbid, size, exp, cap=32)
        assert need == len(want) and got == want + b"\xA5" * (32 - len(want))
        need, got = rr.rdbfile_selectdb(dbid, size, exp, cap=len(want) - 1)
        assert need == len(want) and got == b"\xA5" * (len(want) - 1)
    assert rf.selectdb(64, 10, 2) == b"\xFE\x40\x40\xFB\x0A\x02"
    assert rf.selectdb(0, 1 << 40, 0)[2:] == b"\xFB\x80\xFF\xFF\xFF\xFF\x00"       # trimmed to UINT32_MAX


# ---- the reference's writer and parser round-trip the golden fixtures' payloads -------------------
def golden_payloads():
    g = golden()
    blobs = [bytes.fromhex(fx["blob"]) for key in ("kats", "edges", "shapes") for fx in g[key]]
    data, offs = batch_from_blobs(blobs)
    values, elems, arena, _ = oracle.decode(data, offs)
    types, pdata, poffs, pst, _, _ = ref.save_batch(values, elems, arena)
    return types, pdata, poffs, pst


def test_reference_roundtrip_golden():
    types, pdata, poffs, pst = golden_payloads()
    n = len(types)
    assert n > 20 and (np.asarray(pst) == 0).sum() > 20
    keys = [b"key:%d" % i if i % 3 else str(i * 37 - 50).encode() for i in range(n)]
    kdata, koffs = b"".join(keys), np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64)
    expires = np.array([-1 if i % 2 else 1700000000000 + i for i in range(n)], np.int64)
    idle = np.arange(n, dtype=np.uint64) * 1000
    hd = rf.head("6.0.20", 1700000000, 123456, REPL) + rf.selectdb(0, n, n // 2)
    sec = rf.section(pdata, poffs, types, pst, kdata, koffs, expires, idle, None, hd, rf.IDLE | rf.EOF)
    assert sec["status"] == 0 and sec["bytes"] == len(sec["data"]) and sec["n_bad"] == int((np.asarray(pst) != 0).sum())
    p = rf.parse(sec["data"])
    assert p["version"] == 9 and p["cksum_ok"] and p["cksum"] == sec["crc"] and p["dbs"] == [(0, n, n // 2)]
    assert p["aux"][0] == (b"redis-ver", b"6.0.20") and p["aux"][1] == (b"redis-bits", b"64")
    good = [i for i in range(n) if pst[i] == 0]
    assert len(p["records"]) == len(good)
    pb = bytes(pdata)
    for (db, key, ex, idl, fq, typ, pay), i in zip(p["records"], good):
        assert (db, key, ex, idl, fq, typ) == (0, keys[i], int(expires[i]), int(idle[i]), None, int(types[i]))
        assert pay == pb[int(poffs[i]):int(poffs[i + 1])]
    # a flipped byte fails the checksum; `rdbchecksum no` writes zero and is not checked
    bad = bytearray(sec["data"])
    bad[len(hd) + 3] ^= 0x10
    assert not rf.parse(bytes(bad))["cksum_ok"]
    nock = rf.section(pdata, poffs, types, pst, kdata, koffs, None, None, None, hd, rf.EOF | rf.NO_CKSUM)
    assert nock["data"][-8:] == bytes(8) and rf.parse(nock["data"], checksum=False)["cksum_ok"]
    # DUMP: every payload verifies and comes back
    for i in good[:40]:
        d = rf.dump(int(types[i]), pb[int(poffs[i]):int(poffs[i + 1])])
        assert rf.dump_verify(d) == (0, int(types[i]), pb[int(poffs[i]):int(poffs[i + 1])])
        assert rf.dump_verify(d[:-1] + bytes([d[-1] ^ 1]))[0] == rf.E_CRC
    assert rf.dump_verify(b"\x00" * 10)[0] == rf.E_SHORT


def test_sections_chain():
    """Sections written one after the other with the checksum carried equal one section."""
    rng = np.random.default_rng(3)
    pays = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 300, 9)]
    keys = [b"k%d" % i for i in range(9)]
    pk = lambda xs: (b"".join(xs), np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64))
    ty, st = np.zeros(9, np.uint8), np.zeros(9, np.uint8)
    whole = rf.section(*pk(pays), ty, st, *pk(keys), head=b"HEAD", flags=rf.EOF, crc_in=5)
    crc, data = 5, b""
    for lo, hi, hd, fl in ((0, 3, b"HEAD", 0), (3, 4, b"", 0), (4, 9, b"", rf.EOF)):
        s = rf.section(*pk(pays[lo:hi]), ty[lo:hi], st[lo:hi], *pk(keys[lo:hi]), head=hd, flags=fl, crc_in=crc)
        crc, data = s["crc"], data + s["data"]
    assert data == whole["data"] and crc == whole["crc"]


# ---- the stand-alone host check: a plain build here; its header gives the sanitizer line ----------
def test_host_check_program(tmp_path):
    exe = str(tmp_path / "rdbfile_host_check")
    srcs = [os.path.join(ROOT, "tools", "rdbfile_host_check.c"), os.path.join(ROOT, "redrock_old_amd", "csrc", "rr_rdbfile_api.c")]
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-DRR_RDBFILE_HOST_ONLY",
                    "-I" + os.path.join(ROOT, "include")] + srcs + ["-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "rdbfile host check ok" in r.stdout, r.stdout + r.stderr
