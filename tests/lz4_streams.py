"""LZ4 test streams (include/rr_lz4.h framing: varint32 N + one raw block).

hand_built()   streams written out by hand, each with the verdict the acceptance rule gives and the
               line of LZ4 1.9.2's lz4.c (reference tree, deps/lz4/lib) that decides it
mutated(n, seed)   pyarrow-compressed inputs of 1-5,000 bytes (compressible and random) with 1-3 bit
               flips, deletions or insertions and N off by -1, 0, +1 or +3
"""
import numpy as np

from lz4_reference import E_HEADER, E_LENGTH, E_OFFSET, E_OVERFLOW, E_TRUNC, OK, varint32


def _ext(v):
    """Length-extension bytes for the part of a length past 15."""
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return bytes(out)


class Block:
    """A raw block built sequence by sequence, with the bytes a naive expansion gives."""

    def __init__(self):
        self.src = bytearray()
        self.out = bytearray()

    def seq(self, lits: bytes, offset=None, mlen=None):
        L = len(lits)
        m = 0 if mlen is None else mlen - 4
        self.src.append((min(L, 15) << 4) | min(m, 15))
        if L >= 15:
            self.src += _ext(L - 15)
        self.src += lits
        self.out += lits
        if offset is not None:
            self.src += bytes([offset & 0xFF, offset >> 8])
            if m >= 15:
                self.src += _ext(m - 15)
            for _ in range(mlen):
                self.out.append(self.out[-offset] if 0 < offset <= len(self.out) else 0)
        return self

    def stream(self, n=None):
        return varint32(len(self.out) if n is None else n) + bytes(self.src)


def _lits(n, seed=1):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def hand_built():
    """[(name, stream, status, output or None, deviation or None)]"""
    H = []

    def add(name, stream, status, out=None, dev=None):
        H.append((name, bytes(stream), status, None if out is None else bytes(out), dev))

    def ok(name, b):
        add(name, b.stream(), OK, b.out)

    # empty input, lone tokens
    add("empty_input", b"", E_HEADER)                                  # no preamble
    add("n0_no_block", b"\x00", E_TRUNC)                               # srcSize == 0, lz4.c:1701-1707
    add("n0_token0", b"\x00\x00", OK, b"")                             # lz4.c:1704
    add("n0_token1", b"\x00\x10", E_OVERFLOW)                          # lz4.c:1704: not the byte 00
    add("n1_no_block", b"\x01", E_TRUNC)                               # lz4.c:1707
    add("lone_token_lit1_missing", b"\x01\x10", E_TRUNC)               # ip + length != iend, lz4.c:1945
    add("lone_token_lit1", b"\x01\x10A", OK, b"A")
    add("lone_token_zero_for_n1", b"\x01\x00", E_LENGTH, dev="early_end")   # LZ4 returns 0
    # literal-length extensions of 0, 1 and 2 bytes of 255 (one last run)
    for k, L in ((0, 15), (1, 15 + 255), (2, 15 + 510)):
        ok(f"lit_ext_{k}x255", Block().seq(_lits(L, k)))
    ok("lit_ext_plus7", Block().seq(_lits(15 + 255 + 7)))
    add("lit_ext_byte_missing", varint32(15) + b"\xF0" + _lits(15), E_TRUNC)   # initial check, lz4.c:1634
    # match-length extensions of 0, 1 and 2 bytes of 255
    for k, M in ((0, 19), (1, 19 + 255), (2, 19 + 510), (None, 19 + 255 + 9)):
        ok(f"match_ext_{k}x255" if k is not None else "match_ext_plus9",
           Block().seq(_lits(20, 7), 8, M).seq(b"final"))
    b = Block().seq(_lits(20, 7), 8, 19).seq(b"final")
    s = b.stream()
    add("match_ext_byte_at_end", s[:25] + b"\xff" * 12, E_TRUNC)   # ip >= iend - 4, lz4.c:1972-1973
    # offsets
    for off in (1, 2, 3, 4, 8):
        ok(f"offset_{off}", Block().seq(b"0123456789abcdefghij", off, 37).seq(b"final"))
        ok(f"offset_{off}_short", Block().seq(b"0123456789abcdefghij", off, 4).seq(b"final-literals"))
    ok("offset_65535", Block().seq(_lits(65535, 3), 65535, 70).seq(b"final"))
    ok("offset_65535_of_65536", Block().seq(_lits(65536, 3), 65535, 70).seq(b"final"))
    ok("offset_eq_produced", Block().seq(b"0123456789abcdefghij", 20, 30).seq(b"final"))
    b = Block().seq(b"0123456789abcdefghij", 21, 30).seq(b"final")
    add("offset_one_past_start", b.stream(), E_OFFSET)                 # match < lowPrefix, lz4.c:1981
    add("offset_65535_one_past_start", Block().seq(_lits(65534, 3), 65535, 70).seq(b"final").stream(), E_OFFSET)
    b = Block().seq(b"0123456789abcdefghij", 0, 30).seq(b"final")
    add("offset_0", b.stream(), E_OFFSET, dev="offset0")                # deviation (1.9.2: lz4.c:2030-2031 copies)
    add("offset_0_short_block", Block().seq(b"abcdefgh", 0, 8).seq(b"final").stream(), E_OFFSET, dev="offset0")
    # a match ending 5 and 4 bytes before N (a 40-byte run before it: no shortcut)
    ok("match_ends_5_before_n", Block().seq(_lits(40, 5), 8, 30).seq(b"final"))
    add("match_ends_4_before_n", Block().seq(_lits(40, 5), 8, 30).seq(b"fina").stream(), E_OVERFLOW)   # lz4.c:2047
    ok("match_ends_5_before_n_small", Block().seq(_lits(20, 5), 8, 8).seq(b"final"))
    # the shortcut (lz4.c:1863-1888) takes a 14-byte run that ends 3 bytes before the input's end
    # and copies an 18-byte match to the very end of a 32-byte output: LZ4 1.9.2 accepts
    b = Block().seq(b"0123456789abcd", 8, 18).seq(b"")
    add("shortcut_match_to_n", b.stream(), OK, b.out)
    # a literal run that must be the last one
    b = Block().seq(_lits(20, 9), 8, 20).seq(b"final")
    s = b.stream()
    add("last_run_at_end", s, OK, b.out)
    add("last_run_one_after_end", s[:-1], E_TRUNC)                     # ip + length > iend, lz4.c:1945
    add("last_run_one_before_end", s + b"!", E_OVERFLOW)               # ip + length != iend, lz4.c:1945 (run inside N - 12)
    add("mid_run_within_12_of_n", Block().seq(_lits(20, 9), 8, 20).seq(b"xy", 4, 4).seq(b"final").stream(),
        E_OVERFLOW)                                                    # cpy > oend - MFLIMIT, lz4.c:1910, 1945
    b = Block().seq(_lits(20, 9), 8, 20).seq(_lits(16, 2), 8, 4)       # a 16-byte run, 5 input bytes after it
    add("mid_run_within_8_of_input_end", b.stream(len(b.out) + 40) + b"\x20ab", E_TRUNC)   # lz4.c:1910, 1945
    # N one less / one more than produced
    b = Block().seq(_lits(20, 9), 8, 20).seq(b"final")
    add("n_one_less", b.stream(len(b.out) - 1), E_OVERFLOW)            # the match ends inside the last 5, lz4.c:2047
    add("n_one_more", b.stream(len(b.out) + 1), E_LENGTH, dev="early_end")
    add("n_one_more_literals_only", Block().seq(b"hello").stream(6), E_LENGTH, dev="early_end")
    add("n_one_less_literals_only", Block().seq(b"hello").stream(4), E_OVERFLOW)
    # varints of 1-5 bytes (padded encodings of 5), a 6-byte one, a 5th byte of 16
    for k in range(1, 6):
        pre = b"\x05" if k == 1 else b"\x85" + b"\x80" * (k - 2) + b"\x00"
        add(f"varint_{k}_bytes", pre + b"\x50hello", OK, b"hello")
    add("varint_6_bytes", b"\x85\x80\x80\x80\x80\x00\x50hello", E_HEADER)
    add("varint_5th_byte_16", b"\x85\x80\x80\x80\x10\x50hello", E_HEADER)
    add("varint_unterminated", b"\x85", E_HEADER)
    return H


def _compressible(rng, n):
    words = [bytes(rng.integers(97, 123, int(rng.integers(1, 9)), dtype=np.uint8)) for _ in range(int(rng.integers(2, 40)))]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))]
        if rng.random() < 0.1:
            out += bytes([out[-1]]) * int(rng.integers(1, 300))
    return bytes(out[:n])


def mutated(count, seed=20241):
    """The seeded set of framed streams."""
    import pyarrow as pa
    codec = pa.Codec("lz4_raw")
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(5000 ** rng.random())
        n = min(max(n, 1), 5000)
        data = _compressible(rng, n) if rng.random() < 0.6 else bytes(rng.integers(0, 256, n, dtype=np.uint8))
        raw = bytearray(codec.compress(data, asbytes=True))
        for _ in range(int(rng.choice([1, 1, 1, 2, 2, 3]))):
            kind = int(rng.choice([0, 0, 0, 1, 2]))
            at = int(rng.integers(0, max(len(raw), 1)))
            if kind == 0 and raw:
                raw[at] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1 and len(raw) > 1:
                del raw[at]
            else:
                raw.insert(at, int(rng.integers(0, 256)))
        N = max(n + int(rng.choice([-1, 0, 0, 0, 0, 0, 1, 3])), 0)
        out.append(varint32(N) + bytes(raw))
    return out
