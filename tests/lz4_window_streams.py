"""Hand-built LZ4 streams aimed at the LDS-window decompressor (lz4_dec_kernel in
redrock_old_amd/csrc/rr_lz4.hip): its bail-out to the global path, the wave's copies over
length x offset x alignment, and a seeded generator of valid blocks with a mutated round of them.
No tests here: tests/test_lz4_window_streams.py pins every stream to tests/lz4_reference.py and to
the path it is meant for (CPU), tests/test_gpu_lz4_window.py runs them on the GPU.

route() restates where the kernel sends a block, from the kernel's own conditions (w: the window,
RR_LZ4_DEC_WIN or RR_LZ4_DEC_WINDOW; s0: the block's address mod 4; clen: the whole stream):
  entry     N <= w and ((s0 + clen + 15) & ~15) <= w                    (lz4_dec_kernel)
  D         w + 16 - 16 * ((s0 + clen + 15) >> 4)                       (the staged bytes' base)
  match     bails when op + len > D + next       (next: the first input byte not read yet)
  literals  bails when op > D + p                (p: the run's first byte)
with the acceptance rule's checks (lz4_walk) in front of them, in the kernel's order, so an error
before the first bailing sequence is the LDS path's verdict and one after it is the global path's.

The literal-side test can not fire.  Positions are input positions from the block's dword (s0 +
the index in the stream).  op = 0 <= D + p at the first token.  A run of L literals from p moves
both sides by L.  A match that does not bail leaves op + len <= D + next, and the next run starts
after at least a token, next + 1.  So op <= D + p holds at every run, route() never returns
'bail-literal' and no stream for it exists; walk() still evaluates the test where the kernel
does, so a stream that reached it would show.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

from lz4_reference import read_varint32, varint32

W = 18432                         # RR_LZ4_DEC_WIN's default (test_lz4_window_streams.py compares it with the source)
WINDOWS = (1024, 4096, W)         # the windows route() is used at (RR_LZ4_DEC_WINDOW shrinks the window)
WAVE = 64
OK, HEADER, TRUNC, OFFSET, OVERFLOW, LENGTH, CAPACITY = range(7)
FILL_OK, FILL_TRUNC = b"\x00\x00", b"\x00"    # filler streams of no output: accepted, rejected
MINMATCH, LASTLITERALS, MFLIMIT, FASTLOOP = 4, 5, 12, 64


def _ext(v):
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return bytes(out)


class Seqs:
    """A raw block built sequence by sequence: the bytes a naive expansion gives (the rule of
    lz4_streams.Block.out: out[op + j] = out[op - offset + j], a byte at a time, written here as
    the last `offset` bytes repeated) and the copies a decoder has to make.
    ops: ('lit', index of the run's first byte in the block, op, L) and ('match', op, offset, len)."""

    def __init__(self, rng=None):
        self.src = bytearray()
        self.out = bytearray()
        self.ops = []
        self.valid = True
        self.rng = rng

    @property
    def op(self):
        return len(self.out)

    def seq(self, lits=b"", offset=None, mlen=None):
        lits = bytes(lits)
        L = len(lits)
        m = 0 if mlen is None else mlen - MINMATCH
        self.src.append((min(L, 15) << 4) | min(m, 15))
        if L >= 15:
            self.src += _ext(L - 15)
        self.ops.append(("lit", len(self.src), self.op, L))
        self.src += lits
        self.out += lits
        if offset is not None:
            self.src += bytes([offset & 0xFF, offset >> 8])
            if m >= 15:
                self.src += _ext(m - 15)
            self.ops.append(("match", self.op, offset, mlen))
            if 0 < offset <= self.op:
                seg = bytes(self.out[self.op - offset:])
                self.out += (seg * (mlen // offset + 1))[:mlen]
            else:   # a rejected offset: the bytes it would have made, so later positions stay
                self.out += bytes(mlen)
                self.valid = False
        return self

    def rseq(self, nlits, offset=None, mlen=None):
        return self.seq(self.rng.integers(0, 256, nlits, dtype=np.uint8).tobytes(), offset, mlen)

    def stream(self, n=None):
        return varint32(self.op if n is None else n) + bytes(self.src)


class Walk(NamedTuple):
    route: str          # 'header', 'global', 'lds', 'bail-match' or 'bail-literal'
    status: int         # lz4_walk's verdict
    nseq: int           # sequences read (the failing one included)
    event: int          # index of the first bailing sequence (-1: none)
    bad: int            # index of the failing sequence (-1: none, or LENGTH)
    margins: tuple      # per match reached: D + next - (op + len) (0: equality, below: it bails)
    ops: tuple          # the copies made, as Seqs.ops


def walk(stream, s0=0, w=W, ge=False, d_add=0):
    """lz4_dec_kernel's way with one stream at address s0 (mod 4) under window w.  ge / d_add: the
    match test with >= for >, D moved by d_add (deliberately wrong kernels, for the tests)."""
    s0 &= 3
    clen = len(stream)
    v = i = 0
    ok = False
    while i < min(clen, 5):                       # the varint32 length kernel
        c = stream[i]
        if i == 4 and (c & 0x7F) >= 16:
            break
        v |= (c & 0x7F) << (7 * i)
        i += 1
        if c < 128:
            ok = True
            break
    if not ok:
        return Walk("header", HEADER, 0, -1, -1, (), ())
    N, end = v, s0 + clen
    eligible = N <= w and ((s0 + clen + 15) & ~15) <= w
    D = w + 16 - 16 * ((s0 + clen + 15) >> 4) + d_add
    hl = i

    def b(p):                                     # the input byte at position p (past the end: padding)
        return stream[p - s0] if p < end else 0

    def done(status, nseq, event, how, bad, margins, ops):
        r = "global" if not eligible else how if event >= 0 else "lds"
        return Walk(r, status, nseq, event, bad, tuple(margins), tuple(ops))

    ip = s0 + hl
    if N == 0:                                    # lz4_block
        st = OK if end - ip == 1 and b(ip) == 0 else TRUNC if end == ip else OVERFLOW
        return done(st, 0, -1, None, -1, (), ())
    if end == ip:
        return done(TRUNC, 0, -1, None, -1, (), ())
    op, idx, event, how = 0, 0, -1, None
    margins, ops = [], []
    fast = N >= FASTLOOP

    def ext(p, lim):                              # length_ext: (sum, position after, hit)
        tot = 0
        while True:
            s = b(p)
            p += 1
            tot += s
            if p >= lim:
                return tot, p, True
            if s != 255:
                return tot, p, False

    while True:                                   # lz4_walk
        token = b(ip)
        ip += 1
        L, M = token >> 4, token & 15
        shrt = L != 15 and ip + 16 < end and (fast or op + 32 <= N)
        if L == 15:
            if ip + 15 >= end:
                return done(TRUNC, idx + 1, event, how, idx, margins, ops)
            t, ip, _ = ext(ip, end - 15)
            L += t
        if fast and not shrt and ((token >> 4) != 15 or op + L + 32 > N or ip + L + 32 > end):
            fast = False
        if not shrt and (op + L + MFLIMIT > N or ip + L + (2 + 1 + LASTLITERALS) > end):
            if ip + L > end:
                st = TRUNC
            elif op + L > N:
                st = OVERFLOW
            elif ip + L != end:
                st = OVERFLOW if op + L + MFLIMIT > N else TRUNC
            else:
                st = None
            if st is not None:
                return done(st, idx + 1, event, how, idx, margins, ops)
            if eligible and event < 0 and op > D + ip:
                event, how = idx, "bail-literal"
            ops.append(("lit", ip - s0 - hl, op, L))
            return done(OK if op + L == N else LENGTH, idx + 1, event, how, -1, margins, ops)
        if eligible and event < 0 and op > D + ip:
            event, how = idx, "bail-literal"
        ops.append(("lit", ip - s0 - hl, op, L))
        ip += L
        op += L
        off = b(ip) | (b(ip + 1) << 8)
        ip += 2
        quick = shrt and M != 15 and off >= 8 and off <= op
        if M == 15:
            t, ip, hit = ext(ip, end - LASTLITERALS + 1)
            M += t
            if hit:
                return done(TRUNC, idx + 1, event, how, idx, margins, ops)
        M += MINMATCH
        if off == 0 or off > op:
            return done(OFFSET, idx + 1, event, how, idx, margins, ops)
        if fast and op + M + FASTLOOP >= N:
            fast = False
            quick = False
        if not fast and not quick and op + M + LASTLITERALS > N:
            return done(OVERFLOW, idx + 1, event, how, idx, margins, ops)
        margins.append(D + ip - (op + M))
        if eligible and event < 0 and (op + M >= D + ip if ge else op + M > D + ip):
            event, how = idx, "bail-match"
        ops.append(("match", op, off, M))
        op += M
        idx += 1


def route(stream, s0=0, w=W, ge=False, d_add=0):
    """Where the kernel sends the block: 'header', 'global', 'lds' or 'bail-match' ('bail-literal'
    can not occur: the module's docstring)."""
    return walk(stream, s0, w, ge, d_add).route


def pack_at(streams, alignments):
    """Stream i at an address = alignments[i] mod 16 of the batch's buffer.  The blocks of a batch
    are contiguous, so the gap before a stream is filler streams of no output: FILL_OK (2 bytes,
    accepted) and, for an odd gap, one FILL_TRUNC (1 byte, rejected).  Returns (data, offsets of
    every block, the indices of the real blocks among them)."""
    parts, real, at = [], [], 0
    for s, a in zip(streams, alignments):
        gap = (a - at) & 15
        parts += [FILL_OK] * (gap >> 1) + [FILL_TRUNC] * (gap & 1)
        at += gap
        real.append(len(parts))
        parts.append(s)
        at += len(s)
    offs = np.zeros(len(parts) + 1, np.uint64)
    offs[1:] = np.cumsum([len(x) for x in parts])
    raw = b"".join(parts)
    data = np.zeros(((len(raw) + 15) & ~15) or 16, np.uint8)
    data[:len(raw)] = np.frombuffer(raw, np.uint8)
    return data, offs, np.array(real, np.int64)


class Case(NamedTuple):
    name: str
    stream: bytes
    s0: int                       # the block's address mod 16 in its batch (route() takes it mod 4)
    w: int                        # the window the stream is built for
    route: str                    # where the family says it goes
    status: int                   # the verdict the family says it gets
    expected: Optional[bytes]     # the builder's output (status OK)
    kind: str = ""                # the family's own label
    ops: tuple = ()               # the builder's copies (Seqs.ops)


def _case(name, b, s0, w, rt, status=OK, kind="", stream=None):
    s = b.stream() if stream is None else stream
    return Case(name, s, s0, w, rt, status, bytes(b.out) if status == OK else None, kind, tuple(b.ops))


# ---- a. the bail-out ------------------------------------------------------------------------
PREFIX = ((150, 7, 60), (40, 100, 200), (0, 2, 33))   # (literals, offset, match length): 483 bytes out


def _bail_block(seed, later, M, knob, tail="run", bad_prefix=False):
    """[the prefix,] one literal and a match of M bytes at offset 1, then the tail:
    'run'       a last run of `knob` random bytes
    'offset'    a run of `knob`, a match reaching one byte before the output's start, a last run
    'overflow'  a run of `knob`, a match that ends 4 bytes before N, a last run of 4
    Returns (Seqs, the index of the sized match among the matches)."""
    b = Seqs(np.random.default_rng(seed))
    k = 0
    if later:
        for j, (nl, off, ml) in enumerate(PREFIX):
            b.rseq(nl, b.op + nl + 1 if bad_prefix and j == 1 else off, ml)
        k = len(PREFIX)
    b.rseq(1, 1, M)
    if tail == "run":
        b.rseq(knob)
    elif tail == "offset":
        b.rseq(knob, b.op + knob + 1, 4).rseq(14)
    elif tail == "overflow":
        b.rseq(knob, 8, 4).rseq(4)
    else:
        raise KeyError(tail)
    return b, k


def _sized(w, s0, want, make, cut=0):
    """make(M) -> (Seqs, k) with M such that match k's margin is `want` in a block that enters
    the window (None: this shape can not).  cut: bytes taken off the stream's end."""
    M = w // 2
    for _ in range(8):
        b, k = make(M)
        s = b.stream()
        s = s[:len(s) - cut]
        x = walk(s, s0, w)
        if len(x.margins) <= k:
            return None
        if x.margins[k] == want:
            return (b, s, M) if x.route != "global" else None
        M += x.margins[k] - want
        if M < MINMATCH:
            return None
    return None


def _bail_pair(w, s0, seed, later, tail="run", cut=0):
    """The first knob at which the shape sits on the boundary (margin 0) and, one match byte
    longer, one past it (margin -1), both inside the window: ((Seqs, stream), (Seqs, stream))."""
    for knob in range(300, 364):
        eq = _sized(w, s0, 0, lambda M: _bail_block(seed, later, M, knob, tail), cut)
        if eq is None:
            continue
        b, k = _bail_block(seed, later, eq[2] + 1, knob, tail)
        s = b.stream()
        s = s[:len(s) - cut]
        x = walk(s, s0, w)
        if x.route == "bail-match" and x.margins[k] == -1:
            return (eq[0], eq[1]), (b, s), knob
    raise AssertionError(f"no boundary pair for w {w}, s0 {s0}, later {later}, tail {tail}")


def _entry_cases(w, s0, a):
    """N and the staged span each at w - 16, w, w + 16."""
    out = []
    for dn in (-16, 0, 16):   # a long match at offset 1: the staged bytes are few
        b = Seqs(np.random.default_rng(w + dn)).rseq(1, 1, w + dn - 13).rseq(12)
        assert b.op == w + dn
        out.append(_case(f"entry_n{dn:+d}_w{w}_s{s0}", b, a, w, "global" if dn > 0 else "lds", kind="entry"))
    for dn in (-16, 0, 16):   # one literal run: the span is the block, N stays at or below w
        for L in range(min(w, w + dn), w + dn - 120, -1):
            b = Seqs(np.random.default_rng(w + dn + 1)).rseq(L)
            if ((s0 + len(b.stream()) + 15) & ~15) == w + dn and L <= w:
                break
        else:
            raise AssertionError("no literal run of that span")
        out.append(_case(f"entry_span{dn:+d}_w{w}_s{s0}", b, a, w, "global" if dn > 0 else "lds", kind="entry"))
    return out


@functools.lru_cache(None)
def family_bail():
    """Per window and s0: blocks on the boundary of the match test and one byte past it, as the
    first sequence and after 483 assembled bytes; blocks that bail and are rejected by the global
    path; a block rejected on the LDS path before its bail point; the entry test's edges."""
    cases = []
    for w in WINDOWS:
        for s0 in range(4):
            a = s0 + 4 * ((s0 + w // 1024) & 3)      # s0 at several addresses mod 16
            tag = f"w{w}_s{s0}"
            for later in (False, True):
                shape = "later" if later else "first"
                (eb, es), (bb, bs), knob = _bail_pair(w, s0, 11 + s0, later)
                cases.append(_case(f"eq_{shape}_{tag}", eb, a, w, "lds", kind="eq", stream=es))
                cases.append(_case(f"bail_{shape}_{tag}", bb, a, w, "bail-match", kind="bail", stream=bs))
                if later:   # the same block, the prefix's second offset one byte before the start
                    M = next(o[3] for o in bb.ops[2 * len(PREFIX):] if o[0] == "match")
                    xb, _ = _bail_block(11 + s0, True, M, knob, bad_prefix=True)
                    assert len(xb.stream()) == len(bs)
                    cases.append(_case(f"offset_then_bail_{tag}", xb, a, w, "lds", OFFSET, kind="error-before"))
            for tail, cut, status in (("offset", 0, OFFSET), ("overflow", 0, OVERFLOW), ("run", 1, TRUNC)):
                _, (bb, bs), _ = _bail_pair(w, s0, 21 + s0, True, tail, cut)
                name = {"offset": "offset", "overflow": "overflow", "run": "trunc"}[tail]
                cases.append(_case(f"bail_then_{name}_{tag}", bb, a, w, "bail-match", status, kind="error-after", stream=bs))
            cases += _entry_cases(w, s0, a)
    return cases


# ---- b. the copy matrix ---------------------------------------------------------------------
MATCH_OFFS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 1000, 4099)
MATCH_LENS = ((4, 5, 18, 19) + tuple(range(63, 69)) + tuple(range(127, 131)) + tuple(range(255, 261))
              + tuple(range(1020, 1033)) + tuple(range(1087, 1091)) + (2049, 4100))
LIT_LENS = ((0, 1, 14, 15, 16) + tuple(range(63, 69)) + tuple(range(255, 261)) + tuple(range(1020, 1033))
            + (2049, 4100))
ROUND = 4 * 4 * WAVE          # body bytes a round of lds_copy's dword loop moves
REGIMES = ("byte", "dwords", "rounds", "modulo")


def _len_groups(budget=7000):
    groups, cur = [], []
    for ln in MATCH_LENS:
        if cur and sum(cur) + ln > budget:
            groups.append(tuple(cur))
            cur = []
        cur.append(ln)
    groups.append(tuple(cur))
    return groups


def regime(op_entry):
    """Which copy the LDS path makes for a Seqs.ops entry: lds_copy a byte a lane ('byte'), its
    head / dword body / tail with one round of the body ('dwords') or more ('rounds'), or the
    match's own j % offset rounds ('modulo')."""
    if op_entry[0] == "match":
        _, op, off, ln = op_entry
        if not (off >= ln and ln > WAVE):
            return "modulo"
    else:
        _, _, op, ln = op_entry
    if ln <= WAVE:
        return "byte"
    h = (4 - (op & 3)) & 3
    return "rounds" if ln - h >= ROUND + 4 else "dwords"


def copy_triples(case):
    """{(regime, source & 3, destination & 3)} of the copies of a stream that stays in the window
    (empty copies left out).  A literal's source is D + p with D a multiple of 16: its alignment
    is (s0 + index in the stream) & 3."""
    hl = 0
    while case.stream[hl] & 0x80:
        hl += 1
    hl += 1
    out = set()
    for e in case.ops:
        if e[0] == "lit":
            _, idx, op, ln = e
            src = (case.s0 & 3) + hl + idx
        else:
            _, op, off, ln = e
            src = op - off
        if ln:
            out.add((regime(e), src & 3, op & 3))
    return out


def _finish(b):
    return b.rseq(12 + b.op % 5)


@functools.lru_cache(None)
def family_matrix():
    """Matches over offset x length at every destination alignment (a prefix of 0..3 more bytes),
    offsets equal to the length and one around it, a first match that reaches output byte 0;
    literal runs over length x source alignment (s0) x destination alignment, as a middle run
    and as the last one.  Every stream stays in the default window."""
    cases = []

    def add(name, b, s0=None):
        cases.append(_case(name, b, len(cases) & 15 if s0 is None else s0, W, "lds", kind="matrix"))

    for off in MATCH_OFFS:
        for g, lens in enumerate(_len_groups()):
            for a in range(4):
                b = Seqs(np.random.default_rng(1000 * off + 10 * g + a))
                P = max(off, 12) + a                      # off == op: the first match reads output byte 0
                b.rseq(P, P, 70 if P >= 70 else 6)
                for j, ln in enumerate(lens):
                    b.rseq(j % 3, off, ln)
                add(f"off{off}_g{g}_a{a}", _finish(b))
    for ln in MATCH_LENS:
        for a in range(4):
            b = Seqs(np.random.default_rng(77000 + 10 * ln + a))
            b.rseq(ln + 1 + a, ln + 1 + a, 5)
            for j, off in enumerate((ln - 1, ln, ln + 1)):
                if off >= 1 and not (ln == 4100 and off == ln + 1):
                    b.rseq(j, off, ln)
            add(f"len{ln}_offs_around_a{a}", _finish(b))
    for L in LIT_LENS:
        for a in range(4):
            for s0 in range(4):
                b = Seqs(np.random.default_rng(99000 + 10 * L + a))
                if L >= 5:
                    b.rseq(8, 3, 4 + a).rseq(L, 5, 9).rseq(L)
                else:   # a last run below 5 bytes is accepted only behind LZ4's shortcut (lz4.c:1863-1888)
                    b.rseq(8, 3, 4 + a).rseq(L, 5, 9).rseq(4, 2, 4).rseq(14, 8, 18).rseq(L)
                add(f"lit{L}_a{a}_s{s0}", b, s0 + 4 * a)
    return cases


def sequence_at(case, byte):
    """The index in case.ops of the copy that makes output byte `byte`, and the entry."""
    for i, e in enumerate(case.ops):
        op, ln = (e[2], e[3]) if e[0] == "lit" else (e[1], e[3])
        if op <= byte < op + ln:
            return i, e
    return -1, None


# ---- c. fuzz --------------------------------------------------------------------------------
LIT_CLASSES = ((0, 0), (1, 14), (15, 15), (16, 40), (269, 271), (272, 900))
MATCH_CLASSES = ((4, 18), (19, 19), (20, 70), (273, 275), (276, 2000))


def random_valid_block(rng, max_out):
    """A valid block of at most max_out bytes (at least 13) mixing every token form: L and M below,
    at and above 15, runs of no literals, offsets short, far and back to output byte 0."""
    b = Seqs(rng)
    nseq = int(rng.integers(0, 60))
    last = int(rng.integers(12, 40))
    first = True
    for _ in range(nseq):
        lo, hi = LIT_CLASSES[int(rng.integers(len(LIT_CLASSES)))]
        L = int(rng.integers(lo, hi + 1))
        if first and L == 0:
            L = 1
        lo, hi = MATCH_CLASSES[int(rng.integers(len(MATCH_CLASSES)))]
        M = int(rng.integers(lo, hi + 1))
        if b.op + L + M + last > max_out:
            break
        at = b.op + L
        x = rng.random()
        off = int(rng.integers(1, min(at, 8) + 1)) if x < 0.4 else at if x < 0.5 else int(rng.integers(1, at + 1))
        b.rseq(L, off, M)
        first = False
    return b.rseq(min(last, max_out - b.op))


def mutate(rng, stream):
    """1-3 changes: a byte overwritten or a bit flipped (the preamble included), a byte deleted or
    inserted, the announced length off by -1, +1 or +3, the preamble cut or overlong."""
    m = bytearray(stream)
    for _ in range(int(rng.integers(1, 4))):
        x = rng.random()
        at = int(rng.integers(0, max(len(m), 1)))
        if x < 0.45 and m:
            m[at] = int(rng.integers(256))
        elif x < 0.65 and m:
            m[at] ^= 1 << int(rng.integers(8))
        elif x < 0.75 and len(m) > 1:
            del m[at]
        elif x < 0.85:
            m.insert(at, int(rng.integers(256)))
        elif x < 0.95:
            v = i = 0
            while i < len(m) and i < 5:
                v |= (m[i] & 0x7F) << (7 * i)
                i += 1
                if m[i - 1] < 128:
                    break
            m[:i] = varint32(max(v + int(rng.choice([-1, 1, 3])), 0))
        elif x < 0.975:
            m[:1] = b"\xff\xff\xff\xff\x7f"          # a 5th byte of 16 or more
        else:
            m = bytearray([m[0] | 0x80]) if m else m   # ends inside the preamble
    return bytes(m)


FUZZ_N = 300
MAX_ANNOUNCED = 1 << 16


@functools.lru_cache(None)
def fuzz_valid(seed=1):
    """FUZZ_N valid blocks as Cases (window: the default; the GPU test also runs them under 4096
    and 0), a fifth of them up to the whole window."""
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(FUZZ_N):
        x = rng.random()
        b = random_valid_block(rng, W if x < 0.2 else int(rng.integers(13, 6000)))
        s0 = int(rng.integers(16))
        cases.append(_case(f"valid{seed}_{k}", b, s0, W, route(b.stream(), s0)))
    return cases


@functools.lru_cache(None)
def fuzz_mutated(seed=1):
    """[(stream, s0)]: two mutations of each valid block (one that announces more than
    MAX_ANNOUNCED bytes is drawn again: the batch's output is allocated)."""
    rng = np.random.default_rng(seed + 1000003)
    out = []
    for c in fuzz_valid(seed):
        for _ in range(2):
            while True:
                m = mutate(rng, c.stream)
                h = read_varint32(m)
                if h is None or h[0] <= MAX_ANNOUNCED:
                    break
            out.append((m, c.s0))
    return out
