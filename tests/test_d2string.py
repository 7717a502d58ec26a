"""CPU tests of rr_d2string (include/rr_d2string.h): byte for byte the reference's d2string, whose last
branch is the C library's snprintf("%.17g").  The yardstick is tests/rdbzset_reference.d2string, Python's
'%.17g'; this file first holds that to the C library's own snprintf over every input it uses.  The GPU
tests hold rr_d2string_batch to the same list (tests/test_gpu_rdbzset.py)."""
import os
import re
import subprocess

import numpy as np

import redrock_old_amd as rr

import rdbzset_reference as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_bits(n=200_000, seed=2024):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
    assert int((((b >> np.uint64(52)) & np.uint64(0x7FF)) == 0x7FF).sum()) > 0        # NaN patterns among them
    return b


def check(bits):
    longest = 0
    for b in bits.tolist():
        want = zr.d2string(b)
        v = zr.to_double(b)
        if v == v:
            assert zr.libc_g17(v) == ("%.17g" % v).encode(), hex(b)   # the yardstick against the reference's own call
        got = rr.d2string(v) if v == v else None
        if got is None:                                               # (a NaN's payload does not survive a Python float)
            continue
        assert got == want, (hex(b), got, want)
        longest = max(longest, len(got))
    return longest


def test_examples():
    for v, text in zr.EXAMPLES:
        assert rr.d2string(v) == text == zr.d2string(zr.to_bits(v))
        assert rr.d2string(-v) == b"-" + text
    assert rr.d2string(float("nan")) == b"nan" and rr.d2string(-float("nan")) == b"nan"
    assert rr.d2string(float("inf")) == b"inf" and rr.d2string(float("-inf")) == b"-inf"
    assert rr.d2string(0.0) == b"0" and rr.d2string(-0.0) == b"-0"
    assert rr.d2string(17.0) == b"17" and rr.d2string(1.5) == b"1.5"
    # the ll2string window's edges (util.c:542-544) and the notation switches
    assert rr.d2string(2.0**52 - 1) == b"4503599627370495" and rr.d2string(-(2.0**52 - 1)) == b"-4503599627370495"
    assert rr.d2string(-(2.0**52)) == b"-4503599627370496" and rr.d2string(2.0**52 - 0.5) == b"4503599627370495.5"
    assert rr.d2string(2.0**53) == b"9007199254740992"
    assert rr.d2string(9.9999999999999991e-05) == b"9.9999999999999991e-05" and rr.d2string(99999999999999984.0) == b"99999999999999984"
    assert rr.d2string(1 + 2.0**-17) == b"1.0000076293945312"        # ...3125: a tie, to even


def test_edge_list_is_byte_exact():
    bits = zr.edge_scores()
    assert 5000 < len(bits) < 16000
    assert check(bits) == zr.D2STRING_MAX


def test_ties_round_to_even_both_ways():
    up = down = 0
    for v in zr.tie_scores():
        exact = "%.25f" % v                                           # every tie has at most 17 fractional digits: exact
        digits = exact.replace(".", "").lstrip("0").rstrip("0")
        assert len(digits) == 18 and digits[-1] == "5", (v, exact)
        got = rr.d2string(v).replace(b".", b"").decode()
        assert got == zr.d2string(zr.to_bits(v)).replace(b".", b"").decode()
        kept = int(digits[:17])
        got17 = int(got.ljust(17, "0"))
        assert got17 in (kept, kept + 1) and got17 % 2 == 0, (v, got)
        up += got17 == kept + 1
        down += got17 == kept
    assert up > 500 and down > 500


def test_random_bit_patterns():
    assert check(random_bits()) <= zr.D2STRING_MAX


def test_nan_payloads_through_the_c_entry():
    """Every NaN pattern prints nan (Python floats keep the bits when they are passed as a double)."""
    import ctypes as C
    lib = rr.lib()
    buf = C.create_string_buffer(32)
    for b in (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FF4000000000000):
        n = lib.rr_d2string(buf, C.c_double.from_buffer_copy(C.c_uint64(b)))
        assert buf.raw[:n] == b"nan"


def test_library_exports_every_d2string_symbol():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rr_d2string.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(rr_[a-z_0-9]+)\s*\(", txt)))
    assert len(syms) == 3 and all(s.startswith("rr_d2string") for s in syms)
    lib = rr.lib()
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/rr_d2string.h but not exported"
        assert getattr(lib, s).argtypes, f"{s} not bound"
    assert sorted(rr.D2STRING_EXPORTS) == syms
    for name, py in (("RR_D2STRING_MAX", rr.D2STRING_MAX), ("RR_D2STRING_SLOT", rr.D2STRING_SLOT)):
        assert int(re.search(rf"#define {name}\s+(\d+)", txt).group(1)) == py
    assert rr.D2STRING_MAX == zr.D2STRING_MAX == len("-4.9406564584124654e-324")


def test_d2string_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rr_d2string.h"\n'
                   'int main(void){ return (RR_D2STRING_MAX == 24 && RR_D2STRING_SLOT == 32) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_the_arithmetic_is_one_text_without_library_calls(tmp_path):
    """rr_d2string.c and its header compile alone as strict C99; neither calls a printing or parsing function."""
    csrc = os.path.join(ROOT, "redrock_old_amd", "csrc")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-c", os.path.join(csrc, "rr_d2string.c"),
                    "-o", str(tmp_path / "d.o")], check=True)
    for name in ("rr_d2string_impl.h", "rr_d2string.c"):
        code = re.sub(r"/\*.*?\*/", "", open(os.path.join(csrc, name)).read(), flags=re.S)
        assert not re.search(r"\b(s?n?printf|strto[a-z]+|ato[a-z]+|double\s+[a-z_]+\s*=|float)\b", code), name
    hip = open(os.path.join(csrc, "rr_rdbzset.hip")).read()
    assert '#include "rr_d2string_impl.h"' in hip and "printf" not in hip
