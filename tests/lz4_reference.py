"""The LZ4 block acceptance rule of include/rr_lz4.h in plain Python, and the encoder-side validity
check.  (oracle/ holds the project's other references; this one lives with the tests.)

A stream is a varint32 N (read by the snappy preamble's rule: at most 5 bytes, the 5th below 16)
and one raw LZ4 block.  The block is accepted exactly when LZ4_decompress_safe of LZ4 1.9.2, given
a destination of exactly N bytes, returns N — restated below from LZ4_decompress_generic
(deps/lz4/lib/lz4.c:1658-2072 of the reference tree; endOnInputSize, full block, noDict), line
numbers next to each test — with two stricter deviations: offset 0 (1.9.2 copies garbage) is
OFFSET, and a block that ends cleanly before N bytes (LZ4 returns the smaller count) is LENGTH.

decode(stream) -> (status, bytes or None, deviation or None): deviation names the class
("offset0" / "early_end") when one of the two deviations decided the verdict.
"""
OK, E_HEADER, E_TRUNC, E_OFFSET, E_OVERFLOW, E_LENGTH, E_CAPACITY = range(7)
STATUS_NAMES = {0: "OK", 1: "HEADER", 2: "TRUNC", 3: "OFFSET", 4: "OVERFLOW", 5: "LENGTH", 6: "CAPACITY"}

MINMATCH, LASTLITERALS, MFLIMIT = 4, 5, 12          # lz4.c:189-193
FASTLOOP_SAFE_DISTANCE = 64                          # lz4.c:195


def read_varint32(s: bytes):
    """(value, bytes used) or None."""
    v = 0
    for i in range(min(len(s), 5)):
        c = s[i]
        if i == 4 and (c & 0x7F) >= 16:
            return None
        v |= (c & 0x7F) << (7 * i)
        if c < 128:
            return v, i + 1
    return None


def varint32(n: int) -> bytes:
    out = bytearray()
    while n >= 128:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def decode_block(src: bytes, N: int):
    """The raw block: (status, bytes or None, deviation or None)."""
    S = len(src)
    if N == 0:                                           # lz4.c:1701-1705
        if S == 1 and src[0] == 0:
            return OK, b"", None
        return (E_TRUNC if S == 0 else E_OVERFLOW), None, None
    if S == 0:                                           # lz4.c:1707
        return E_TRUNC, None, None
    out = bytearray()
    ip = 0
    fast = N >= FASTLOOP_SAFE_DISTANCE                   # lz4.c:1711 (op == 0)
    while True:
        token = src[ip]                                  # lz4.c:1721 / 1849 (ip < S: see below)
        ip += 1
        L, M = token >> 4, token & 15
        op = len(out)
        # the literal run checked by the end rules unless a shortcut takes it:
        #   fast loop, L < 15: ip <= S - 17 (lz4.c:1751); L == 15: the run ends at or before
        #   N - 32 and S - 32 (lz4.c:1738), which implies both end rules
        #   safe loop: L < 15, ip < S - 16 and op <= N - 32 (lz4.c:1863-1865)
        short = L != 15 and ip < S - 16 and (fast or op <= N - 32)
        if L == 15:
            if ip >= S - 15:                             # initial check, lz4.c:1634 with 1729 / 1898
                return E_TRUNC, None, None
            while True:
                s = src[ip]
                ip += 1
                L += s
                if ip >= S - 15 or s != 255:             # loop check: no error for literals, lz4.c:1642, 1730 / 1899
                    break
        if fast and not short and (L != 15 or op + L > N - 32 or ip + L > S - 32):
            fast = False                                 # safe_literal_copy: the safe loop from here on (lz4.c:1738, 1751)
        if not short and (op + L > N - MFLIMIT or ip + L > S - (2 + 1 + LASTLITERALS)):   # lz4.c:1910
            if ip + L > S:                               # lz4.c:1945
                return E_TRUNC, None, None
            if op + L > N:
                return E_OVERFLOW, None, None
            if ip + L != S:                              # not the last run
                return (E_OVERFLOW if op + L > N - MFLIMIT else E_TRUNC), None, None
            out += src[ip:ip + L]
            if len(out) != N:                            # deviation: LZ4 returns the smaller count
                return E_LENGTH, None, "early_end"
            return OK, bytes(out), None
        out += src[ip:ip + L]
        ip += L
        op += L
        offset = src[ip] | (src[ip + 1] << 8)            # lz4.c:1764 / 1873 / 1963 (ip + 2 <= S by the tests above)
        ip += 2
        quick = short and M != 15 and offset >= 8 and offset <= op   # lz4.c:1788-1798 / 1878-1888: no end test
        if M == 15:
            while True:                                  # lz4.c:1774 / 1972: lencheck S - 4, every error counts
                s = src[ip]
                ip += 1
                M += s
                if ip >= S - LASTLITERALS + 1:
                    return E_TRUNC, None, None
                if s != 255:
                    break
        M += MINMATCH
        if offset == 0:                                  # deviation: not checked by 1.9.2 (lz4.c:2031 copies garbage)
            return E_OFFSET, None, "offset0"
        if offset > op:                                  # lz4.c:1773 / 1801 / 1981
            return E_OFFSET, None, None
        if fast and op + M >= N - FASTLOOP_SAFE_DISTANCE:   # lz4.c:1778 / 1783: the safe loop from here on
            fast = False
            quick = False
        if not fast and not quick and op + M > N - LASTLITERALS:   # lz4.c:2047
            return E_OVERFLOW, None, None
        if offset >= M:
            out += out[op - offset:op - offset + M]
        else:                                            # an overlapping match repeats its last `offset` bytes
            out += (bytes(out[op - offset:]) * (M // offset + 1))[:M]
        # the next token is inside the input: after a checked run ip + L <= S - 8, after a
        # shortcut ip <= S - 1, and a match extension leaves ip < S - 4


def decode(stream: bytes):
    """The framed stream: (status, bytes or None, deviation or None)."""
    h = read_varint32(stream)
    if h is None:
        return E_HEADER, None, None
    return decode_block(stream[h[1]:], h[0])


def sequences(src: bytes):
    """The token walk of a raw block decode_block() accepts: (L, None, None) for the last literal
    run, (L, offset, M) with M the whole match length for every sequence before it; None as the
    last item when the block ends before its last literal run."""
    ip = 0
    while True:
        if ip >= len(src):
            yield None
            return
        token = src[ip]
        ip += 1
        L, M = token >> 4, token & 15
        if L == 15:
            while True:
                s = src[ip]
                ip += 1
                L += s
                if s != 255:
                    break
        ip += L
        if ip == len(src):
            yield L, None, None
            return
        offset = src[ip] | (src[ip + 1] << 8)
        ip += 2
        if M == 15:
            while True:
                s = src[ip]
                ip += 1
                M += s
                if s != 255:
                    break
        yield L, offset, M + MINMATCH


def check_encoder_rules(stream: bytes):
    """The encoder-side end rules (lz4_Block_format.md, "End of block restrictions") on a framed
    stream decode() accepts: the last 5 bytes are literals and the last match starts at least 12
    bytes before the end; a block below 13 bytes is one literal run.  Returns None or a message."""
    h = read_varint32(stream)
    if h is None:
        return "bad preamble"
    N, src = h[0], stream[h[1]:]
    op = nseq = 0
    for q in sequences(src):
        if q is None:
            return "block ends before its last literal run"
        L, offset, M = q
        op += L
        nseq += 1
        if offset is None:
            if op != N:
                return f"{op} bytes, {N} announced"
            if N >= 1 and nseq > 1 and L < LASTLITERALS:
                return f"last literal run of {L} bytes"
            return None
        if N < MFLIMIT + 1:
            return "a match in a block below 13 bytes"
        if offset == 0 or offset > op:
            return f"offset {offset} at output {op}"
        if op > N - MFLIMIT:
            return f"a match starts at {op}, {N - op} bytes before the end"
        if op + M > N - LASTLITERALS:
            return f"a match ends at {op + M}, {N - op - M} bytes before the end"
        op += M
