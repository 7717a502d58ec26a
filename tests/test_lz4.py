"""CPU tests of the LZ4 block codec's contract (include/rr_lz4.h): the Python statement of the
acceptance rule (tests/lz4_reference.py) pinned by hand-built streams and by pyarrow's lz4_raw
codec (a later LZ4 release, independent of this text); the ABI of the new header; the compile-time
knobs of rr_lz4.hip."""
import os
import re
import subprocess
import sys

import pytest

import redrock_old_amd as rr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lz4_reference as ref  # noqa: E402
import lz4_streams  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "redrock_old_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
HAND = lz4_streams.hand_built()


def pyarrow_decode(stream):
    """None (no preamble), ("ERR",) or ("OK", bytes) from pyarrow's lz4_raw on the raw block."""
    import pyarrow as pa
    h = ref.read_varint32(stream)
    if h is None:
        return None
    try:
        return "OK", pa.Codec("lz4_raw").decompress(stream[h[1]:], decompressed_size=h[0], asbytes=True)
    except (OSError, ValueError):
        return ("ERR",)


@pytest.mark.parametrize("name,stream,status,out,dev", HAND, ids=[h[0] for h in HAND])
def test_hand_built_verdict(name, stream, status, out, dev):
    got = ref.decode(stream)
    assert (ref.STATUS_NAMES[got[0]], got[1], got[2]) == (ref.STATUS_NAMES[status], out, dev)


def test_hand_built_classes_present():
    names = {h[0] for h in HAND}
    assert len(names) == len(HAND) >= 50
    for need in ("empty_input", "lone_token_lit1", "lit_ext_0x255", "lit_ext_1x255", "lit_ext_2x255", "match_ext_0x255",
                 "match_ext_1x255", "match_ext_2x255", "offset_1", "offset_2", "offset_3", "offset_4", "offset_8",
                 "offset_65535", "offset_eq_produced", "offset_one_past_start", "match_ends_5_before_n",
                 "match_ends_4_before_n", "last_run_one_before_end", "last_run_at_end", "last_run_one_after_end",
                 "n_one_less", "n_one_more", "offset_0", "varint_1_bytes", "varint_5_bytes", "varint_6_bytes"):
        assert need in names, need


def test_hand_built_agree_with_pyarrow():
    """Outside the two deviation classes pyarrow's release gives every hand-built stream the same
    verdict and bytes."""
    for name, stream, status, out, dev in HAND:
        p = pyarrow_decode(stream)
        if dev is not None or p is None:
            continue
        assert (p[0] == "OK") == (status == ref.OK), name
        if status == ref.OK:
            assert p[1] == out, name


def test_mutated_streams_agree_with_pyarrow():
    """20,000 seeded streams: the same verdict and the same bytes as pyarrow's lz4_raw, the two
    deviation classes left out."""
    streams = lz4_streams.mutated(20000)
    acc = rej = left = 0
    for s in streams:
        st, out, dev = ref.decode(s)
        if dev is not None:
            left += 1
            continue
        p = pyarrow_decode(s)
        if st == ref.OK:
            acc += 1
            assert p[0] == "OK" and p[1] == out, s.hex()
        else:
            rej += 1
            assert p is None or p[0] == "ERR", (ref.STATUS_NAMES[st], s.hex())
    n = len(streams)
    print(f"accepted {acc / n:.3f} rejected {rej / n:.3f} left out {left / n:.3f}")
    assert left <= 0.25 * n and acc >= 0.20 * n and rej >= 0.20 * n, (acc, rej, left)


def test_encoder_rule_checker():
    b = lz4_streams.Block().seq(b"0123456789abcdefghij", 8, 20).seq(b"final")
    assert ref.check_encoder_rules(b.stream()) is None
    B = lz4_streams.Block
    assert "ends at" in ref.check_encoder_rules(B().seq(b"0123456789abcdefghij", 8, 20).seq(b"fina").stream())
    assert "starts at" in ref.check_encoder_rules(B().seq(b"0123456789abcdefghij", 8, 4).seq(b"final-runxy", 4, 4).seq(b"final").stream())
    assert "below 13" in ref.check_encoder_rules(B().seq(b"abc", 1, 4).seq(b"final").stream())
    assert ref.check_encoder_rules(lz4_streams.Block().seq(b"hello").stream()) is None
    assert ref.check_encoder_rules(b"\x00\x00") is None


# ---- ABI ---------------------------------------------------------------------------------------
def declared_symbols(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(rr_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_lz4_symbol():
    lib = rr.lib()
    syms = declared_symbols("rr_lz4.h")
    assert len(syms) == 6 and all(s.startswith("rr_lz4_") for s in syms)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/rr_lz4.h but not exported"
    assert sorted(rr.LZ4_EXPORTS) == syms
    assert lib.rr_lz4_max_compressed_length(16384) == 5 + 16384 + 64 + 16
    assert lib.rr_lz4_compress_bound(3, 1000) >= 3 * 21 + 1000 + 1000 // 255
    assert rr.LZ4_STATUS == {i: n for i, n in ref.STATUS_NAMES.items()}


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rr_lz4.h"\n#include "rr_kv.h"\n'
                   "int main(void){ return RR_LZ4_E_CAPACITY - 6 + RR_KV_LZ4 - 2 + (int)(RR_KV_SNAPPY & RR_KV_LZ4); }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


# ---- the knobs of rr_lz4.hip ---------------------------------------------------------------------
VARIANTS = ["-DRR_LZ4_DEC_WIN=16384", "-DRR_LZ4_HASH_LOG=13", "-DRR_LZ4_HASH_LOG=10 -DRR_LZ4_DEC_WIN=32768"]


def test_every_lz4_knob_has_a_variant():
    text = open(os.path.join(CSRC, "rr_lz4.hip")).read()
    knobs = set(re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b.*?\b(RR_[A-Z0-9_]+)", text, re.M))
    assert knobs and all(k.startswith("RR_LZ4_") for k in knobs), knobs
    assert knobs <= set(re.findall(r"-D(RR_[A-Z0-9_]+)", " ".join(VARIANTS)))
    for other in ("rr_kernels.hip", "rr_flat_device.h", "rr_util.hip", "rr_decode_class.h", "rr_snappy.hip"):
        assert "RR_LZ4_" not in open(os.path.join(CSRC, other)).read(), other


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("flags", VARIANTS)
def test_lz4_variant_compiles(flags):
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-Wno-unused-command-line-argument",
           *flags.split(), "rr_lz4.hip"]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
