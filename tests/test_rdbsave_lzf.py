"""CPU tests of the LZF side of include/rr_rdbsave.h: tests/lzf_reference.py's decompressor on
hand-written streams, each next to the lzf_d.c line that decides it; its compressor (the size
yardstick of tests/test_gpu_rdbsave_lzf.py) round-tripped; the loader of LZF strings; the header as
C99; and the one compile-time knob rr_rdbsave.hip keeps, cross-compiled with a non-default value."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import redrock_old_amd as rr

import lzf_reference as lz
import rdb_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redrock_old_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_literal_runs():
    assert lz.decompress(b"\x00A", 1) == b"A"                              # lzf_d.c:72-74: ctrl 0 is one byte
    body = bytes(range(32))
    assert lz.decompress(b"\x1f" + body, 32) == body                       # ctrl 31: 32 bytes, the longest run
    assert lz.decompress(b"\x00A\x01BC", 3) == b"ABC"                      # :185 the loop goes on while input is left


def test_back_references():
    abc = b"\x02abc"
    assert lz.decompress(abc + b"\x20\x02", 6) == b"abcabc"                # :108 l = 1: 3 bytes; :110, :131 offset 2 + 1
    assert lz.decompress(abc + b"\xc0\x02", 11) == b"abc" + b"abcabcab"    # l = 6: 8 bytes, the longest short form
    assert lz.decompress(abc + b"\xe0\x00\x02", 12) == b"abc" * 4          # :119-121 l = 7 + 0: 9 bytes
    assert lz.decompress(abc + b"\xe0\xff\x02", 267) == (b"abc" * 89)[:267]   # l = 7 + 255: 264 bytes
    assert lz.decompress(b"\x00x\x20\x00", 4) == b"xxxx"                   # offset 1: :163-165 octet by octet, overlapping
    assert lz.decompress(b"\x01xy\xe0\x01\x01", 12) == b"xy" * 6           # an overlapping copy at offset 2
    far = bytes(np.random.default_rng(1).integers(0, 256, 8192, dtype=np.uint8))
    lits = b"".join(b"\x1f" + far[k:k + 32] for k in range(0, 8192, 32))
    assert lz.decompress(lits + b"\x3f\xff", 8195) == far + far[:3]        # offset (0x1f << 8 | 0xff) + 1 = 8192


def test_rejections():
    assert lz.decompress(b"\x02ab", 3) is None                             # :83 literals past the input
    assert lz.decompress(b"\x02abc\x20", 6) is None                        # :113 a reference without its offset byte
    assert lz.decompress(b"\x02abc\xe0", 12) is None                       # :113 nor its length byte
    assert lz.decompress(b"\x02abc\xe0\x00", 12) is None                   # :123 length byte, then no offset byte
    assert lz.decompress(b"\x02abc\x20\x03", 6) is None                    # :139 offset 4 at position 3: before the start
    assert lz.decompress(b"\x20\x00", 3) is None                           # :139 a reference first
    assert lz.decompress(b"\x02abc", 2) is None                            # :76 literals past the output
    assert lz.decompress(b"\x02abc\x20\x02", 5) is None                    # :133 a reference past the output
    assert lz.decompress(b"\x02abc\x20\x02", 6) == b"abcabc"
    assert len(lz.decompress(b"\x02abc", 10)) == 3                         # (a short result: the caller's test, rdb.c:388)


def _gpu_test_strings():
    """The shapes of the GPU test's strings (tests/test_gpu_rdbsave_lzf.py), smaller where only the
    length differs."""
    rng = np.random.default_rng(3)

    def rand(n):
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))
    out = [b"z" * k for k in (20, 21, 22, 24, 25, 4096)] + [rand(k) for k in (21, 64, 4096)]
    out += [b"q" * k for k in (63, 64, 16383, 16384)] + [(b"abcdefg" * 3000)[:k] for k in (63, 64, 16383, 16384)]
    out += [rand(r) + bytes(300) for r in range(30, 75, 7)]
    r = rand(8193)
    out += [r[:8192] + r[:100] + bytes(600), r + r[:100] + bytes(600), r[:100] + bytes(8092) + r[:100]]
    for rep in (3, 8, 9, 10, 264, 265, 266, 600):
        body = rand(rep)
        out.append(rand(40) + body + b"\x01\x02" + body + bytes(80))
    out += [rand(10) + (rand(p) * 400)[:700] for p in (1, 2, 3, 5)]
    out += [rand(k) + b"r" * 200 for k in (31, 32, 33, 64, 65)] + [rand(30) + b"s" * 100, b"t" * 100 + b"!"]
    out += [(rand(5000) * 14)[:k] for k in (65535, 65536, 70000)]
    return out


def test_compress_round_trips():
    n_lzf = 0
    for s in _gpu_test_strings():
        c = lz.compress(s, len(s) - 4)
        if c is not None:
            assert len(c) <= len(s) - 4 and lz.decompress(c, len(s)) == s
            n_lzf += 1
        full = lz.compress(s, 2 * len(s) + 16)                             # room enough: never refused
        assert full is not None and lz.decompress(full, len(s)) == s
    assert n_lzf > 30
    assert lz.compress(b"", 10) is None and lz.compress(b"abc", 0) is None  # lzf_c.c:130


def test_loader_expands_lzf_strings():
    s = b"hello hello hello hello hello"
    enc = lz.save_lzf_string(s)
    assert enc[0] == 0xC3 and enc[2] == len(s)                             # rdb.c:323-346
    assert lz.load(rr.T_STRING, enc) == (("string", s), [(enc[1], len(s), enc[3:], s)])
    assert lz.save_lzf_string(b"x" * 20) == ref.save_raw_string(b"x" * 20)  # rdb.c:426: len > 20
    assert lz.save_lzf_string(b"12345") == ref.save_raw_string(b"12345")   # the integer attempt first, :416
    payload = ref.save_len(2) + enc + ref.save_raw_string(b"7") + enc + ref.save_raw_string(b"plain")
    assert lz.load(rr.T_HASH_HT, payload)[0] == ("hash", [s, b"7", s, b"plain"])
    zs = ref.save_len(1) + enc + bytes(8)
    assert lz.load(rr.T_ZSET_SKIPLIST, zs)[0] == ("zset", [s, 0])
    with pytest.raises(AssertionError):
        lz.load(rr.T_STRING, enc[:-1])
    bad = bytes([0xC3, enc[1], len(s) + 1]) + enc[3:]                      # announces one byte more than the stream gives
    with pytest.raises(AssertionError):
        lz.load(rr.T_STRING, bad)


def test_yardstick_compresses_config_3():
    """The corpus of the GPU size test is worth measuring on: lzf_c.c's rule puts at least half of
    config 3's eligible strings into the LZF form."""
    data, offs = rr.gen_batch(3, 300)
    values, elems, arena, _ = rr.host_decode(data, offs)
    ab = arena.tobytes()
    strings = [s for val, descs in ref.flat_values(values, elems, arena) for s in lz.eligible_strings(val, descs, ab)]
    assert len(strings) == 300
    assert 2 * sum(lz.compress(s, len(s) - 4) is not None for s in strings) >= len(strings)


def test_header_compiles_as_c99_with_the_flag(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rr_rdbsave.h"\n'
                   'int main(void){ rr_rdbsave_opts o = {RR_RDBSAVE_DEFAULT_FILL, RR_RDBSAVE_LZF};\n'
                   '  rr_rdbsave_opts z = {RR_RDBSAVE_DEFAULT_FILL, 0};\n'
                   '  return (int)(o.flags - 1u + z.flags) + (int)sizeof(o) - 8; }\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_python_options_word():
    assert rr.RDBSAVE_LZF == 1
    o = rr.RdbSaveOpts(-2, rr.RDBSAVE_LZF)
    assert o.flags == 1 and rr.RdbSaveOpts.flags.offset == 4 and rr.RdbSaveOpts.flags.size == 4


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")
@pytest.mark.parametrize("flags", ["-DRR_LZF_HASH_LOG=9", "-DRR_LZF_HASH_LOG=13"])
def test_hash_log_variant_compiles(flags):
    """RR_LZF_HASH_LOG, the knob rr_rdbsave.hip keeps (the LZF table's size): a front-end pass of the
    device code with non-default values, as tests/test_build_variants.py does for the other sources."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only",
           "-Wno-unused-command-line-argument", *flags.split(), "rr_rdbsave.hip"]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
