"""CPU tests of the host half of include/rr_rdbread.h against tests/rdbread_reference.py: the record
index (rr_rdbread_index) on streams built with rdbfile_reference's writers and by hand, whole, in
chunks with carry-over and under small capacities; its errors at their offsets; the host string
reader; and the stand-alone sanitizer program.  The GPU tests hold the split and the verdict to the
same statement (tests/test_gpu_rdbread.py)."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import redrock_old_amd as rr

import rdb_reference as ref
import rdbfile_reference as rf
import rdbread_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RNG = np.random.default_rng(20261021)
rand = lambda n: RNG.integers(0, 256, n, dtype=np.uint8).tobytes()
ZL_EMPTY = struct.pack("<IIH", 11, 10, 0) + b"\xFF"
LONG = b"compressible " * 9


def lz(s):
    return R.lzf_string(R.lzf_literal(s), len(s))


def rec(typ, key_enc, payload, prefix=b""):
    return prefix + bytes([typ]) + key_enc + payload


def zset2(pairs):
    return ref.save_len(len(pairs)) + b"".join(m + struct.pack("<d", x) for m, x in pairs)


def loader_records():
    """One record of each of the eight loader types, with LZF and integer strings as keys, members and nodes."""
    return [
        rec(0, R.raw(b"str"), ref.save_raw_string(b"value")),
        rec(0, R.int_string(-7), lz(LONG)),                                            # integer key, LZF value
        rec(2, lz(b"set:" + LONG), R.counted([R.raw(b"m1"), R.int_string(77), lz(LONG)])),   # LZF key
        rec(4, R.raw(b"hash"), ref.save_len(2) + R.raw(b"f") + R.int_string(70000) + lz(LONG) + R.raw(b"")),
        rec(5, R.int_string(32767), zset2([(R.raw(b"a"), 1.5), (lz(LONG), -2.0)])),
        rec(11, R.raw(b"iset"), R.raw(struct.pack("<II", 2, 2) + struct.pack("<hh", 1, 2))),
        rec(12, R.raw(b"zzl"), R.raw(ZL_EMPTY)),
        rec(13, R.raw(b"hzl"), lz(ZL_EMPTY * 3)),
        rec(14, R.raw(b"ql"), R.counted([R.raw(ZL_EMPTY), lz(ZL_EMPTY * 3), R.int_string(5)])),
    ]


def legacy_records():
    nan, inf = float("nan"), float("inf")
    return [
        rec(1, R.raw(b"list"), R.counted([R.raw(b"a"), R.int_string(5), lz(LONG)])),
        rec(3, R.raw(b"zset"), ref.save_len(4) + b"".join(R.raw(m) + R.old_double(x) for m, x in
                                                            ((b"a", nan), (b"b", inf), (b"c", -inf), (b"d", 1.5)))),
        rec(9, R.raw(b"zipmap"), R.raw(b"\x00\xFF")),
        rec(10, R.raw(b"lzl"), R.raw(ZL_EMPTY)),
    ]


def prefixed_records():
    out = [rec(0, R.raw(b"k" * 70), R.raw(bytes(range(256)) * 3), b"\xF9\xFF"),          # a key and a value with 2-byte lengths
           rec(0, R.raw(b"fd"), R.raw(b"v"), b"\xFD" + struct.pack("<i", -5)),
           rec(0, R.raw(b"fc2"), R.raw(b"v"), b"\xFC" + struct.pack("<q", 1) + b"\xFC" + struct.pack("<q", 1700000000123))]
    for idle in (5, 300, 70000, 1 << 33):                                              # the 1-, 2-, 5- and 9-byte forms
        out.append(rec(0, R.raw(b"idle%d" % idle), R.raw(b"v"), b"\xF8" + ref.save_len(idle) + b"\xF9\x07"))
    return out


def stream(version=9, eof=True):
    hd = rf.head("6.0.20", 1700000000, 123456, (0, "a" * 40, 1))
    hd = b"REDIS%04d" % version + hd[9:]
    body = hd + rf.selectdb(0, 9, 0) + b"".join(loader_records()) + b"".join(prefixed_records())
    body += rf.selectdb(3, 4, 0) + b"".join(legacy_records())
    if not eof:
        return body
    body += b"\xFF"
    return body + (struct.pack("<Q", rf.crc64(0, body)) if version >= 5 else b"")


def same_as_walk(got, want):
    assert got["rc"] == R.DONE
    assert list(zip(got["rec_start"].tolist(), got["rec_end"].tolist(), got["rec_db"].tolist())) == want["records"]
    assert [(int(i["opcode"]), int(i["at"]), int(i["end"])) for i in got["items"]] == want["items"]
    assert (got["eof_at"], got["has_cksum"], got["cksum"]) == (want["eof_at"], want["has_cksum"], want["cksum"])
    assert got["state"].version == want["version"] and got["state"].pos == want["end"]


# ---- the index against the reference --------------------------------------------------------------------
def test_exports_and_constants():
    L = rr.lib()
    for name in rr.RDBREAD_EXPORTS:
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "rr_rdbread.h")).read()
    for sym in ("DONE", "MORE", "FULL", "E_SLICE", "E_TRUNC", "E_OPCODE", "E_KEY", "NO_CKSUM", "E_MAGIC", "E_VERSION",
                "E_UNSUPPORTED", "E_LEN", "MAX_WAVES", "LANE_BYTES"):
        m = re.search(rf"#define RR_RDBREAD_{sym}\s+(\d+)u?\b", hdr)
        assert m and int(m.group(1)) == getattr(rr, "RDBREAD_" + sym), sym
    assert rr.RDBREAD_WAVE_STEP == 64 * rr.RDBREAD_LANE_BYTES and "(64u * RR_RDBREAD_LANE_BYTES)" in hdr
    fh = open(os.path.join(ROOT, "include", "rr_rdbfile.h")).read() + open(os.path.join(ROOT, "include", "rr_rdbconvert.h")).read()
    taken = {int(x) for x in re.findall(r"#define RR_RDB\w+_(?:E_\w+|SKIP)\s+(\d+)\b", fh)}
    assert not taken & set(range(46, 55))                                              # the numbering continues, no clash


@pytest.mark.parametrize("version", [9, 4, 5, 1])
def test_index_whole(version):
    s = stream(version)
    want = R.walk(s)
    assert len(want["records"]) == 20 and want["has_cksum"] == (version >= 5) and want["version"] == version
    assert {d for _, _, d in want["records"]} == {0, 3}
    got = rr.rdbread_index(s)
    same_as_walk(got, want)
    assert len(s) == want["end"]
    if version >= 5:
        assert got["cksum"] == rf.crc64(0, s[:-8])


def test_reference_agrees_with_the_framing_parser():
    """On a stream rdbfile_reference.parse takes (no 0xFD, no legacy type), the walk's extents split
    into what parse reports."""
    recs = loader_records() + prefixed_records()[:1] + prefixed_records()[2:]
    body = rf.head("6.0.20", 1, 2, None) + rf.selectdb(2, len(recs), 0) + b"".join(recs) + b"\xFF"
    s = body + struct.pack("<Q", rf.crc64(0, body))
    p, w = rf.parse(s), R.walk(s)
    assert p["cksum_ok"] and len(p["records"]) == len(w["records"]) == len(recs)
    for (db, key, ex, idle, freq, typ, pay), (a, b, wdb) in zip(p["records"], w["records"]):
        assert R.split_record(s[a:b]) == (0, typ, key, pay, ex, idle, freq) and wdb == db == 2
    assert [s[a:b] for a, b, _ in w["records"]] == recs
    same_as_walk(rr.rdbread_index(s), w)


def test_section_writer_output_indexes():
    """What rr_rdbfile_section's reference writes comes back record by record."""
    n = 40
    pays = [ref.save_raw_string(rand(int(k))) for k in RNG.integers(0, 200, n)]
    keys = [b"key:%d" % i if i % 3 else str(i * 1000 - 7).encode() for i in range(n)]
    pk = lambda xs: (b"".join(xs), np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64))
    ex = np.array([1700000000000 + i if i % 4 == 0 else -1 for i in range(n)], np.int64)
    hd = rf.head("6.0.20", 1, 2, None) + rf.selectdb(0, n, n // 4)
    sec = rf.section(*pk(pays), np.zeros(n, np.uint8), np.zeros(n, np.uint8), *pk(keys), ex, np.arange(n, dtype=np.uint64) * 500,
                     np.arange(n, dtype=np.uint8), hd, rf.IDLE | rf.FREQ | rf.EOF)
    got = rr.rdbread_index(sec["data"])
    same_as_walk(got, R.walk(sec["data"]))
    assert np.array_equal(got["rec_start"], sec["rec_offsets"][:n]) and np.array_equal(got["rec_end"], sec["rec_offsets"][1:])
    assert got["cksum"] == sec["crc"] and got["eof_at"] == int(sec["rec_offsets"][n])
    for i in range(n):
        a, b = int(got["rec_start"][i]), int(got["rec_end"][i])
        assert R.split_record(sec["data"][a:b]) == (0, 0, keys[i], pays[i], int(ex[i]), 500 * i, i)


# ---- incremental use ------------------------------------------------------------------------------------
def feed(s, chunk, max_recs=None, max_items=None):
    """The stream in chunks of `chunk` bytes with carry-over: (records, items, the DONE result's fields)."""
    st = rr.RdbReadState()
    buf, base, fed = b"", 0, 0
    recs, items = [], []
    while True:
        r = rr.rdbread_index(buf, st, max_recs, max_items)
        recs += [(a + base, b + base, d) for a, b, d in zip(r["rec_start"].tolist(), r["rec_end"].tolist(), r["rec_db"].tolist())]
        items += [(int(i["opcode"]), int(i["at"]) + base, int(i["end"]) + base) for i in r["items"]]
        if r["rc"] == R.DONE:
            return recs, items, (r["eof_at"] + base, r["has_cksum"], r["cksum"], st.pos + base)
        assert r["rc"] in (R.MORE, R.FULL), r["rc"]
        if r["rc"] == R.MORE:
            assert fed < len(s), "MORE on a complete stream"
            buf, base = buf[st.pos:], base + st.pos                                    # keep the incomplete one's bytes
            st.pos = 0
            buf += s[fed:fed + chunk]
            fed += chunk


def test_chunks_of_every_size():
    s = stream(9)
    assert 1500 < len(s) < 3000
    w = R.walk(s)
    want = (w["records"], w["items"], (w["eof_at"], True, w["cksum"], len(s)))
    for chunk in range(1, 65):
        assert feed(s, chunk) == want, chunk


def test_capacities():
    s = stream(9)
    w = R.walk(s)
    nr, ni = len(w["records"]), len(w["items"])
    want = (w["records"], w["items"], (w["eof_at"], True, w["cksum"], len(s)))
    # exact: the 0xFF comes next, so the walk is done
    same_as_walk(rr.rdbread_index(s, max_recs=nr, max_items=ni), w)
    # one at a time, and one short of exact
    assert feed(s, 1 << 20, 1, 1) == want
    assert feed(s, 7, 1, 1) == want
    assert feed(s, 1 << 20, nr - 1, ni - 1) == want
    # 0: FULL at the first one of that kind, the position behind the last one reported
    r = rr.rdbread_index(s, max_recs=0)
    assert r["rc"] == R.FULL and r["state"].pos == w["records"][0][0] and len(r["rec_start"]) == 0
    assert [int(i["at"]) for i in r["items"]] == [a for _, a, _ in w["items"] if a < w["records"][0][0]]
    r = rr.rdbread_index(s, max_items=0)
    assert r["rc"] == R.FULL and r["state"].pos == 9 == w["items"][0][1] and len(r["rec_start"]) == 0
    r2 = rr.rdbread_index(s, r["state"])                                               # resumed with room
    assert r2["rc"] == R.DONE and len(r2["rec_start"]) == nr and len(r2["items"]) == ni


# ---- errors ---------------------------------------------------------------------------------------------
GOOD = rf.head("6.0.20", 1, 2, None) + rf.selectdb(0, 2, 0) + rec(0, R.raw(b"k0"), R.raw(b"v")) + rec(2, R.raw(b"k1"), R.counted([R.raw(b"m")]))
M64 = b"\x81" + b"\xFF" * 8
TAIL = rec(0, R.raw(b"after"), R.raw(b"v")) + b"\xFF" + bytes(8)


@pytest.mark.parametrize("bad,code", [
    (b"\x06" + R.raw(b"mod") + b"\x01\x02", R.E_UNSUPPORTED),          # module
    (b"\x07" + R.raw(b"mod2") + b"\x01\x02", R.E_UNSUPPORTED),         # module 2
    (b"\x0F" + R.raw(b"stream") + b"\x00", R.E_UNSUPPORTED),           # stream
    (b"\xF7\x01\x02", R.E_UNSUPPORTED),                                # MODULE_AUX
    (b"\x10" + R.raw(b"k") + R.raw(b"v"), R.E_UNSUPPORTED),            # type 16
    (b"\xF6" + R.raw(b"k") + R.raw(b"v"), R.E_UNSUPPORTED),            # type 0xF6
    (b"\xFC" + bytes(8) + b"\xF7", R.E_UNSUPPORTED),                   # an opcode behind a prefix
    (b"\xF9\x01\xFF", R.E_UNSUPPORTED),
    (b"\x00\x82" + bytes(8), R.E_LEN),                                 # length bytes of no form
    (b"\x00\xBF" + bytes(8), R.E_LEN),
    (b"\x00" + R.raw(b"k") + b"\xC4\x00\x00", R.E_LEN),                # string encoding 0xC4
    (b"\xF8\x82\x00", R.E_LEN),                                        # an idle time of no form
    (b"\x02" + R.raw(b"k") + b"\x02" + R.raw(b"m") + b"\x90", R.E_LEN),
    (b"\xFA\x83\x00", R.E_LEN),                                        # inside an item
    (b"\xFE\xBF", R.E_LEN),
])
def test_errors_at_their_offset(bad, code):
    s = GOOD + bad + TAIL
    with pytest.raises(R.Stop) as e:
        R.walk(s)
    assert (e.value.code, e.value.at) == (code, len(GOOD))
    got = rr.rdbread_index(s)
    assert got["rc"] == code and got["err_at"] == len(GOOD) == got["state"].pos
    assert list(zip(got["rec_start"].tolist(), got["rec_end"].tolist())) == [(a, b) for a, b, _ in e.value.partial["records"]]
    assert len(got["rec_start"]) == 2 and len(got["items"]) == len(e.value.partial["items"])


@pytest.mark.parametrize("bad", [
    b"\x00" + M64 + b"abc",                                            # a key of 2^64 - 1 bytes
    b"\x00" + b"\x81\x80" + bytes(7) + b"abc",                         # 2^63
    b"\x00" + R.raw(b"k") + M64 + b"abc",                              # a value of 2^64 - 1 bytes
    b"\x00" + R.raw(b"k") + b"\xC3" + M64 + b"\x05" + b"abc",          # an LZF stream of 2^64 - 1 bytes
    b"\x02" + R.raw(b"k") + M64 + R.raw(b"a") * 50,                    # a count of 2^64 - 1
    b"\x04" + R.raw(b"k") + M64 + R.raw(b"a") * 51,                    # 2 * count wraps if multiplied
    b"\x05" + R.raw(b"k") + b"\x81\x80" + bytes(7) + (R.raw(b"a") + bytes(8)) * 9,
    b"\x03" + R.raw(b"k") + M64 + (R.raw(b"a") + b"\xFC" + bytes(252)) * 3,
    b"\xF8" + M64[:5],                                                 # the buffer ends inside a length
    b"\xFA" + R.raw(b"name") + b"\x80\xFF\xFF\xFF\xFF",
])
def test_lengths_near_2_64_give_more(bad):
    s = GOOD + bad
    with pytest.raises(R.Stop) as e:
        R.walk(s)
    assert (e.value.code, e.value.at) == (R.MORE, len(GOOD))
    got = rr.rdbread_index(np.frombuffer(s, np.uint8).copy())
    assert got["rc"] == R.MORE and got["state"].pos == len(GOOD) and len(got["rec_start"]) == 2


def test_header():
    for s, code in ((b"REDIS0009", R.MORE), (b"REDIS000", R.MORE), (b"", R.MORE), (b"RODIS0009\xFF", R.E_MAGIC),
                    (b"REDIS0000\xFF", R.E_VERSION), (b"REDIS0010\xFF", R.E_VERSION), (b"REDIS00a9\xFF", R.E_VERSION),
                    (b"REDIS0005\xFF", R.MORE)):
        got = rr.rdbread_index(s)
        assert got["rc"] == code, (s, got["rc"])
        assert got["state"].pos == (9 if s == b"REDIS0009" or s == b"REDIS0005\xFF" else 0)
        if code != R.MORE:
            with pytest.raises(R.Stop) as e:
                R.walk(s)
            assert e.value.code == code and got["state"].version == 0
    got = rr.rdbread_index(b"REDIS0004\xFF")
    assert got["rc"] == R.DONE and not got["has_cksum"] and got["eof_at"] == 9 and got["state"].pos == 10
    got = rr.rdbread_index(b"REDIS0005\xFF" + struct.pack("<Q", 0x1122334455667788))
    assert got["rc"] == R.DONE and got["has_cksum"] and got["cksum"] == 0x1122334455667788 and got["state"].pos == 18


# ---- the string reader ----------------------------------------------------------------------------------
def test_string_forms():
    cases = [(R.raw(b""), b""), (R.raw(b"a"), b"a"), (R.raw(rand(63)), None), (R.raw(rand(64)), None), (R.raw(rand(16384)), None),
             (lz(LONG), LONG), (R.lzf_string(b"\x00a" + R.lzf_backref(264, 1), 265), b"a" * 265),
             (R.lzf_string(b"\x02abc" + R.lzf_backref(3, 3) + b"\x00z", 7), b"abcabcz")]
    cases += [(R.int_string(v), str(v).encode()) for v in (0, -128, 127, -32768, 32767, -2147483648, 2147483647)]
    cases += [(b"\xC1\x05\x00", b"5"), (b"\xC2\xFF\xFF\xFF\xFF", b"-1")]               # wider forms than needed
    for enc, want in cases:
        if want is None:
            want = ref_load(enc)
        buf = b"\xEE\xEE\xEE" + enc + b"\xDD"
        assert rr.rdbread_string(buf, 3) == (R.DONE, want, len(want), 3 + len(enc)), enc[:8]
        assert rr.rdbread_string(buf, 3, out_cap=len(want) + 5) == (R.DONE, want, len(want), 3 + len(enc))
        if want:
            assert rr.rdbread_string(buf, 3, out_cap=len(want) - 1) == (R.E_CAPACITY, None, len(want), 3 + len(enc))
        if len(enc) > 1:
            assert rr.rdbread_string(buf[:3 + len(enc) - 1], 3)[0] == R.MORE           # cut one byte short
    assert rr.rdbread_string(b"", 0)[0] == R.MORE
    for enc, code in ((b"\xC4\x00", R.E_LEN), (b"\x82\x00", R.E_LEN), (M64 + b"ab", R.MORE),
                      (R.lzf_string(R.lzf_literal(b"abc"), 4), R.E_KEY),               # one short of its length
                      (R.lzf_string(R.lzf_literal(b"abc"), 2), R.E_KEY),               # one over
                      (R.lzf_string(b"\x00a" + R.lzf_backref(3, 2), 4), R.E_KEY),      # a reference before the start
                      (R.lzf_string(b"", 0), R.E_KEY)):
        assert rr.rdbread_string(enc, 0)[0] == code, enc
    assert rr.rdbread_len(b"\x00\x40\x05", 1) == (R.DONE, 5, 3)
    assert rr.rdbread_len(b"\xC7", 0) == (R.DONE, 7, 1)                                 # a count site: the six bits
    assert rr.rdbread_len(b"\x81" + struct.pack(">Q", 1 << 40), 0) == (R.DONE, 1 << 40, 9)
    assert rr.rdbread_len(b"\x80\x00", 0)[0] == R.MORE and rr.rdbread_len(b"\x82", 0)[0] == R.E_LEN


def ref_load(enc):
    import rdbload_reference as ld
    return ld.Rd(enc).string()


def test_items_read_back():
    """The AUX fields and the db sizes through the helpers, as a loader would read them."""
    s = stream(9)
    got = rr.rdbread_index(s)
    aux, dbs = [], []
    for it in got["items"]:
        at = int(it["at"]) + 1
        if it["opcode"] == 0xFA:
            _, k, _, at = rr.rdbread_string(s, at)
            _, v, _, at = rr.rdbread_string(s, at)
            aux.append((k, v))
        elif it["opcode"] == 0xFE:
            dbs.append([rr.rdbread_len(s, at)[1]])
            at = rr.rdbread_len(s, at)[2]
        else:
            _, a, at = rr.rdbread_len(s, at)
            _, b, at = rr.rdbread_len(s, at)
            dbs[-1] += [a, b]
        assert at == int(it["end"])
    assert aux[:2] == [(b"redis-ver", b"6.0.20"), (b"redis-bits", b"64")] and (b"repl-id", b"a" * 40) in aux
    assert dbs == [[0, 9, 0], [3, 4, 0]]


# ---- the stand-alone sanitizer program ------------------------------------------------------------------
def test_host_check_program_under_sanitizers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for flags in (["-fsanitize=address,undefined", "-static-libasan"], ["-fsanitize=address,undefined"]):
        p = subprocess.run([gcc] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if p.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("gcc -fsanitize=address,undefined does not build a program that runs here")
    exe = str(tmp_path / "rdbread_host_check")
    srcs = [os.path.join(ROOT, "tools", "rdbread_host_check.c"), os.path.join(ROOT, "redrock_old_amd", "csrc", "rr_rdbread_api.c")]
    subprocess.run([gcc, "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags + ["-DRR_RDBREAD_HOST_ONLY", "-I" + os.path.join(ROOT, "include")]
                   + srcs + ["-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "rdbread host check ok" in r.stdout, r.stdout + r.stderr
