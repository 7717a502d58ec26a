"""Hand-built snappy streams aimed at the LDS-window decompressor (dec_block_lds in
redrock_old_amd/csrc/rr_snappy.hip): its bail-out to the global path, the 64-tag batch, the
64-position speculation round, the back-reference copies, and a seeded generator of valid tag
sequences with a mutated round of them.  No tests here: tests/test_snappy_streams.py pins every
stream to the oracle and to the path it is meant for (CPU), tests/test_gpu_snappy_window.py runs
them on the GPU.

route() restates where the kernel sends a block, from the kernel's own conditions:
  entry     expected <= W and ((s0 + clen + 15) & ~15) <= W            (snz_dec_kernel)
  D         W + 16 - 16 * ((s0 + clen + 15) >> 4)                      (the staged bytes' base)
  literal   bails when D + tq < tpos + 8                               (tq: its bytes' position)
  copy      bails when tpos + len > D + tpn                            (tpn: the next tag)
with the serial decoder's checks in front of them, in its order, so an error before the first
bailing tag is the LDS path's verdict and one after it is the global path's.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

from snappy_corpus import copy1, copy2, copy4, corpus, lit, varint

W = 18432                      # RR_SNZ_DEC_WIN's default (test_snappy_streams.py compares it with the source)
BATCH = 64                     # tags a batch (a lane each)
ROUND = 64                     # positions a speculation round (RR_SNZ_SPEC 1)
OK, HEADER, TRUNC, OFFSET, OVERFLOW, LENGTH = 0, 1, 2, 3, 4, 5
FILL = {1: b"\x00", 2: b"\x80\x00", 3: b"\x80\x80\x00"}   # valid streams of 0 bytes of output


def lit_n(b, nb):
    """A literal with nb extra length bytes (0: the length in the tag byte); any nb that holds the
    length is valid, the shortest or not."""
    n = len(b) - 1
    if nb == 0:
        assert n < 60
        return bytes([n << 2]) + b
    assert n < (1 << (8 * nb))
    return bytes([(59 + nb) << 2]) + n.to_bytes(nb, "little") + b


class Stream:
    """Tags appended one by one, the expected output tracked here (not by a decoder)."""

    def __init__(self, rng=None):
        self.tags = []
        self.out = bytearray()
        self.clen = 0          # compressed bytes so far, without the preamble
        self.valid = True
        self.rng = rng

    @property
    def pos(self):
        return len(self.out)

    @property
    def ntags(self):
        return len(self.tags)

    def _add(self, tag):
        self.tags.append(tag)
        self.clen += len(tag)

    def lit(self, b, nb=None):
        b = bytes(b)
        self._add(lit(b) if nb is None else lit_n(b, nb))
        self.out += b
        return self

    def rlit(self, n, nb=None):
        return self.lit(self.rng.integers(0, 256, n, dtype=np.uint8).tobytes(), nb)

    def copy(self, off, ln, kind=2):
        pos = self.pos
        assert 0 < off <= pos
        self._add({1: copy1, 2: copy2, 4: copy4}[kind](off, ln))
        # out[pos + j] = out[pos - off + j % off] for j < ln
        src = bytes(self.out[pos - off:pos])
        self.out += (src * (ln // off + 1))[:ln]
        return self

    def raw(self, tag, adv=0):
        """A tag the decoder must reject (or bytes that are no whole tag); adv: the output
        bytes it would have made, so later tags keep positions a decoder that went on would see."""
        self._add(bytes(tag))
        self.out += bytes(adv)
        self.valid = False
        return self

    def pad_to(self, nbytes):
        """Literals up to exactly nbytes of tag bytes in all (from the first tag's position)."""
        rem = nbytes - self.clen
        assert rem == 0 or rem >= 2
        while rem:
            k = rem if rem <= 61 else min(61, rem - 2)
            self.rlit(k - 1)
            rem -= k
        return self

    def finish(self, announce=None):
        out = bytes(self.out)
        s = varint(len(out) if announce is None else announce) + b"".join(self.tags)
        return s, (out if self.valid and announce is None else None)


class Walk(NamedTuple):
    route: str          # 'header', 'global', 'lds', 'bail-literal' or 'bail-copy'
    ntags: int          # tags the serial decoder reads (the failing one included)
    status: int         # the serial decoder's verdict
    event: int          # index of the first bailing tag (-1: none)
    bad: int            # index of the failing tag (-1: none, or LENGTH)
    indep: int          # back-references the LDS path copies together / in stream order
    ordered: int        # (counted for streams that stay on the LDS path and decode)


def walk(stream, s0=0, w=W):
    n = len(stream)
    v = shift = i = 0
    ok = False
    while i < n and shift < 32:          # snz_len_kernel
        c = stream[i]
        i += 1
        if shift == 28 and (c & 0x7F) >= 16:
            break
        v |= (c & 0x7F) << shift
        shift += 7
        if c < 128:
            ok = True
            break
    if not ok:
        return Walk("header", 0, HEADER, -1, -1, 0, 0)
    expected, end = v, s0 + n
    eligible = expected <= w and ((s0 + n + 15) & ~15) <= w
    D = w + 16 - 16 * ((s0 + n + 15) >> 4)
    p, pos, idx, event, how, status = s0 + i, 0, 0, -1, None, None
    copies = []                          # (tag index, tpos, off, len)
    while p < end and status is None:
        c = stream[p - s0]
        ty = c & 3
        if ty == 0:
            ln = (c >> 2) + 1
            nb = ln - 60 if ln >= 61 else 0
            tq = p + 1 + nb
            if tq > end:
                status = TRUNC
            else:
                if nb:
                    ln = int.from_bytes(stream[p + 1 - s0:tq - s0], "little") + 1
                if ln > end - tq:
                    status = TRUNC
                elif ln > expected - pos:
                    status = OVERFLOW
                else:
                    if eligible and event < 0 and D + tq < pos + 8:
                        event, how = idx, "bail-literal"
                    pos += ln
                    p = tq + ln
        else:
            nb = 1 if ty == 1 else 2 if ty == 2 else 4
            tq = p + 1 + nb
            if tq > end:
                status = TRUNC
            else:
                x = int.from_bytes(stream[p + 1 - s0:tq - s0], "little")
                ln, off = (4 + ((c >> 2) & 7), ((c >> 5) << 8) | x) if ty == 1 else ((c >> 2) + 1, x)
                if off == 0 or off > pos:
                    status = OFFSET
                elif ln > expected - pos:
                    status = OVERFLOW
                else:
                    if eligible and event < 0 and pos + ln > D + tq:
                        event, how = idx, "bail-copy"
                    copies.append((idx, pos, off, ln))
                    pos += ln
                    p = tq
        idx += 1
    bad = idx - 1 if status is not None else -1
    if status is None:
        status = OK if pos == expected else LENGTH
    r = "global" if not eligible else how if event >= 0 else "lds"
    indep = ordered = 0
    if r == "lds" and status == OK:
        first = {}
        for k, tpos, off, ln in copies:
            c0 = first.setdefault(k // BATCH, tpos)
            if off >= ln and tpos - off + ln <= c0:
                indep += 1
            else:
                ordered += 1
    return Walk(r, idx, status, event, bad, indep, ordered)


def route(stream, s0=0, w=W):
    """(where the kernel sends the block, its number of tags)."""
    k = walk(stream, s0, w)
    return k.route, k.ntags


def pack_at(streams, alignments):
    """Like test_gpu_snappy.pack with block i of `streams` starting at an address = alignments[i]
    mod 4.  The blocks of a batch are contiguous, so the gap before a stream is a 1-3 byte valid
    stream of its own (FILL, no output).  Returns (data, offsets of every block, the indices of
    the real blocks among them)."""
    parts, real, at = [], [], 0
    for s, a in zip(streams, alignments):
        gap = (a - at) & 3
        if gap:
            parts.append(FILL[gap])
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
    s0: int                       # the block's address mod 4 in its batch
    route: str                    # where the family says it goes
    status: int                   # the verdict the family says it gets
    expected: Optional[bytes]     # the builder's output (status OK)


def _case(name, built, s0, rt, status=OK):
    s, out = built
    return Case(name, s, s0, rt, status, out if status == OK else None)


# ---- a. the bail-out ------------------------------------------------------------------------
def bail_copy_rle(tail=700):
    """lit('z'), copy2(1, 64) until 17,700 bytes are out, then one-byte literals: the copies'
    output passes the staged tags long before the tags are read."""
    s = Stream(np.random.default_rng(101)).lit(b"z")
    while s.pos < 17700:
        s.copy(1, 64)
    for _ in range(tail):
        s.rlit(1)
    return s


def bail_copy_far(ncopies=230):
    """3,000 one-byte literals, copy2(3000, 64) repeated, one-byte literals up to exactly W."""
    s = Stream(np.random.default_rng(102))
    for _ in range(3000):
        s.rlit(1)
    for _ in range(ncopies):
        s.copy(3000, 64)
    while s.pos < W:
        s.rlit(1)
    return s


def bail_literal(s0):
    """Output exactly W, ending in one long literal whose destination comes within 8 bytes of its
    source: that needs 9 or more bytes of padding behind the block, (s0 + clen) % 16 in 1..7,
    found here by route() over the number of copies and one-byte literals in front."""
    for ncopies in range(150, 230):
        for nlits in range(16):
            s = Stream(np.random.default_rng(103 + s0)).lit(b"z")
            for _ in range(nlits):
                s.rlit(1)
            for _ in range(ncopies):
                s.copy(1 + nlits, 64)
            s.rlit(W - s.pos)
            k = walk(s.finish()[0], s0)
            if k.route == "bail-literal" and k.event == k.ntags - 1:
                return s
    raise AssertionError("no bail-literal stream found")


def _replace_tag(s, idx, tag):
    """The stream with tag idx replaced by a rejected one of the same output length."""
    t = Stream()
    t.tags, t.out, t.valid = list(s.tags), bytearray(s.out), False
    t.tags[idx] = tag
    t.clen = sum(len(x) for x in t.tags)
    return t


@functools.lru_cache(None)
def family_bail():
    """Bailing blocks at every s0, each between two ordinary 16 KiB blocks; a block that bails
    and is rejected by the global path; blocks rejected on the LDS path before their bail point."""
    from oracle import cpu
    text = corpus()["text_150k"]
    plain = [cpu.snappy_compress(text[16384 * k:16384 * (k + 1)]) for k in range(4)]
    cases = []

    def ordinary(k):
        cases.append(Case(f"plain{len(cases)}", plain[k % 4], k % 4, "lds", OK, text[16384 * (k % 4):16384 * (k % 4 + 1)]))

    n = 0
    for s0 in range(4):
        for name, s, rt in (("rle", bail_copy_rle(), "bail-copy"), ("far", bail_copy_far(), "bail-copy"),
                            ("longlit", bail_literal(s0), "bail-literal")):
            ordinary(n)
            cases.append(_case(f"{name}_s{s0}", s.finish(), s0, rt))
            n += 1
        ordinary(n)
    # the bail point of the rle shape, then rejected tags around it
    rle = bail_copy_rle()
    ev = walk(rle.finish()[0], 0).event
    assert ev % BATCH >= 8 and ev % BATCH < BATCH - 8 and rle.ntags > ev + 80
    bad_off = copy2(0, 64)
    for s0 in range(4):
        # after the bail point: in its batch, and far behind it -> the global path's verdict
        cases.append(_case(f"bail_then_offset_same_batch_s{s0}", _replace_tag(rle, ev + 3, bad_off).finish(), s0, "bail-copy", OFFSET))
        cases.append(_case(f"bail_then_offset_later_s{s0}", _replace_tag(rle, rle.ntags - 5, bad_off).finish(), s0, "bail-copy", OFFSET))
        cases.append(_case(f"bail_then_length_s{s0}", rle.finish(announce=rle.pos + 1), s0, "bail-copy", LENGTH))
        # before it: in its batch, and batches earlier -> the LDS path's verdict, no bail
        cases.append(_case(f"offset_then_bail_same_batch_s{s0}", _replace_tag(rle, ev - 3, bad_off).finish(), s0, "lds", OFFSET))
        cases.append(_case(f"offset_then_bail_earlier_s{s0}", _replace_tag(rle, 10, bad_off).finish(), s0, "lds", OFFSET))
        ordinary(s0)
    return cases


# ---- b. the 64-tag batch --------------------------------------------------------------------
NTAGS = (1, 63, 64, 65, 127, 128, 129, 200)


def _mixed(rng, ntags, mix):
    s = Stream(rng).rlit(int(rng.integers(4, 40)))
    while s.ntags < ntags:
        k = s.ntags
        if mix == "lit" or (mix == "alt" and k % 2 == 0):
            s.rlit(int(rng.integers(1, 9)))
        else:
            off = int(rng.integers(1, min(s.pos, 40) + 1))
            s.copy(off, int(rng.integers(1, 65)))
    return s


def _bad_tag(kind, s, rng):
    """Append one rejected tag of `kind` to s; returns the announced length it needs (or None)."""
    if kind == "trunc":            # a literal longer than the rest of the block
        s.raw(bytes([62 << 2]) + (70000).to_bytes(3, "little") + b"abc", 3)
    elif kind == "offset0":
        s.raw(copy2(0, 7), 7)
    elif kind == "offset_past":    # (the first tag: any offset is past the start)
        s.raw(copy2(s.pos + 1, 7), 7)
    elif kind == "overflow_lit":
        b = rng.integers(0, 256, 9, dtype=np.uint8).tobytes()
        s.raw(lit(b), 9)
        return s.pos - 1
    elif kind == "overflow_copy":
        if s.pos == 0:
            s.rlit(4)
        s.raw(copy2(min(s.pos, 3), 9), 9)
        return s.pos - 1
    else:
        raise KeyError(kind)
    return None


BAD_KINDS = {"trunc": TRUNC, "offset0": OFFSET, "offset_past": OFFSET, "overflow_lit": OVERFLOW, "overflow_copy": OVERFLOW}
BAD_AT = (0, 62, 63, 64, 65)


@functools.lru_cache(None)
def family_batch():
    rng = np.random.default_rng(201)
    cases = []
    for n in NTAGS:
        for mix in ("lit", "copy", "alt"):
            cases.append(_case(f"{mix}{n}", _mixed(rng, n, mix).finish(), len(cases) & 3, "lds"))
    # the first tag of batch 2 reads the end of batch 1 (offset <= length, offset > length); a
    # copy in batch 2 whose source straddles the boundary
    for off, ln in ((1, 64), (3, 40), (7, 7), (5, 64), (40, 9), (64, 63), (64, 64), (33, 5)):
        for mix in ("lit", "alt"):
            s = _mixed(rng, BATCH, mix)
            s.copy(off, ln).rlit(3).copy(2, 11)
            cases.append(_case(f"b2_first_{mix}_{off}_{ln}", s.finish(), len(cases) & 3, "lds"))
            s = _mixed(rng, BATCH, mix)
            s.rlit(5).copy(5 + off, min(64, off + 6)).copy(1, 9)          # source [B - off, B + 6)
            cases.append(_case(f"b2_straddle_{mix}_{off}_{ln}", s.finish(), len(cases) & 3, "lds"))
    # one rejected tag at the batch's edges, the rest valid
    for kind, status in BAD_KINDS.items():
        for at in BAD_AT:
            if kind == "overflow_copy" and at == 0:
                continue   # (a copy as the first tag is OFFSET)
            s = _mixed(rng, at, "alt") if at else Stream(rng)
            assert s.ntags == at
            ann = _bad_tag(kind, s, rng)
            while s.ntags < 70:
                s.rlit(2).copy(1, 5)
            cases.append(_case(f"{kind}_at{at}", s.finish(announce=s.pos if ann is None else ann), len(cases) & 3, "lds", status))
    # a tag cut off by the block's end: after its first byte, before its last
    for at in BAD_AT:
        for tag in (copy1(1, 4), copy2(1, 4), copy4(1, 4), bytes([63 << 2, 1, 0, 0, 0])):
            for cut in sorted({1, len(tag) - 1}):
                s = _mixed(rng, at, "alt") if at else Stream(rng)
                s.raw(tag[:cut])
                cases.append(_case(f"cut{cut}_type{tag[0] & 3}_at{at}", s.finish(announce=s.pos + 4), len(cases) & 3, "lds", TRUNC))
    # LENGTH: the block ends after tag `at` one byte short of the announced length
    for at in BAD_AT:
        s = _mixed(rng, at + 1, "alt")
        cases.append(_case(f"length_at{at}", s.finish(announce=s.pos + 1), len(cases) & 3, "lds", LENGTH))
    # two rejected tags of different kinds: the first one's verdict
    pairs = [("offset0", "overflow_lit"), ("overflow_copy", "offset0"), ("trunc", "offset0"), ("offset0", "trunc"),
             ("overflow_lit", "trunc"), ("offset_past", "overflow_copy")]
    spots = [(10, 20), (62, 63), (1, 63), (63, 64), (60, 70), (127, 128), (64, 127)]
    for ka, kb in pairs:
        for ia, ib in spots:
            s = _mixed(rng, ia, "alt")
            ann = _bad_tag(ka, s, rng)
            while s.ntags < ib:
                s.rlit(2)
            annb = _bad_tag(kb, s, rng)
            while s.ntags < ib + 8:
                s.rlit(2).copy(1, 5)
            ann = ann if ann is not None else annb if annb is not None else s.pos
            cases.append(_case(f"two_{ka}@{ia}_{kb}@{ib}", s.finish(announce=ann), len(cases) & 3, "lds", BAD_KINDS[ka]))
    return cases


# ---- c. the 64-position speculation round ---------------------------------------------------
def _tail(s):
    return s.copy(3, 10).rlit(2).copy(1, 64, 4).rlit(70).copy(9, 4, 1)


@functools.lru_cache(None)
def family_spec():
    """The round starts at the first tag (the byte after the preamble); offsets below are from it."""
    rng = np.random.default_rng(301)
    cases = []

    def add(name, built, status=OK):
        for s0 in range(4):
            cases.append(_case(f"{name}_s{s0}", built, s0, "lds", status))

    # one literal of 62 .. 66 tag bytes, and the same offsets reached by several tags
    for size in (62, 63, 64, 65, 66):
        nb = 1
        add(f"one_literal_{size}", _tail(Stream(rng).rlit(size - 1 - nb, nb)).finish())
        add(f"tags_to_{size}", _tail(Stream(rng).pad_to(size)).finish())
    # a literal header across the round's end
    for at in (60, 61, 62, 63):
        for nb in (1, 2, 3, 4):
            for n in (5, 70, 300):
                if n - 1 < (1 << (8 * nb)):
                    add(f"lit_hdr_at{at}_nb{nb}_len{n}", _tail(Stream(rng).pad_to(at).rlit(n, nb)).finish())
    # a copy-4 tag across it
    for at in (59, 60, 61, 62, 63):
        add(f"copy4_at{at}", _tail(Stream(rng).pad_to(at).copy(int(rng.integers(1, 30)), int(rng.integers(1, 65)), 4)).finish())
    # the block's last literal: ends at the block's end / claims one byte more
    for at in (10, 60, 61, 62, 63):
        for n, nb in ((1, 0), (7, 0), (7, 1), (61, 1), (70, 2), (300, 4)):
            s = Stream(rng).pad_to(at).rlit(n, nb)
            add(f"last_lit_at{at}_len{n}_nb{nb}", s.finish())
            t = Stream(rng).pad_to(at)
            b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            t.raw(lit_n(b + b"x", nb)[:-1], n + 1)   # the length says n + 1, n bytes follow
            add(f"last_lit_short_at{at}_len{n}_nb{nb}", t.finish(), TRUNC)
    return cases


# ---- d. the back-reference matrix -----------------------------------------------------------
OFFSETS = tuple(range(1, 21)) + (31, 32, 33, 63, 64, 65)
LENGTHS = tuple(range(1, 13)) + (15, 16, 17, 31, 32, 33, 63, 64)
FRONT = 19000   # a literal in front of the same tags: the output no longer fits the window


def _kind(off, ln, k):
    return 1 if 4 <= ln <= 11 and off < 2048 and k % 2 == 0 else 2


def _matrix_streams(rng):
    """(name, builder): builder(s) appends the tags to a Stream."""
    out = []
    for off in OFFSETS:
        for a in range(4):   # the prefix's length mod 4: every length at every destination alignment
            def plain(s, off=off, a=a):
                s.rlit(off + 1 + ((a - off - 1 - s.pos) & 3) + 4 * (off % 3))
                for k, ln in enumerate(LENGTHS):
                    s.copy(off, ln, _kind(off, ln, k + a))
            out.append((f"off{off}_a{a}", plain))

            def spaced(s, off=off, a=a):
                # a short literal, the offset's copy (reads what was just written: in stream
                # order), a copy of the same length from the prefix (before the batch's first
                # copy: copied together with the others of its kind)
                start = s.pos
                s.rlit(72 + ((a - s.pos) & 3))
                plen = s.pos - start
                for k, ln in enumerate(LENGTHS):
                    s.rlit(1 + (k + a) % 3)
                    s.copy(off, ln, _kind(off, ln, k + a + 1))
                    src = start + (k * 5 + a) % (plen - ln + 1)
                    s.copy(s.pos - src, ln, 2 if k % 4 else 4)
            out.append((f"off{off}_a{a}_spaced", spaced))
    for seed in range(8):   # chains of 10 copies, each reading the one before it
        def chain(s, seed=seed):
            r = np.random.default_rng(400 + seed)
            s.rlit(int(r.integers(1, 24)))
            prev = min(s.pos, 20)
            for _ in range(10):
                off, ln = int(r.integers(1, prev + 1)), int(r.integers(1, 65))
                s.copy(off, ln, _kind(off, ln, int(r.integers(2))))
                prev = ln
        out.append((f"chain{seed}", chain))

    def far(s):
        s.rlit(2100)
        for k, ln in enumerate(LENGTHS):
            if 4 <= ln <= 11:
                s.copy(2047, ln, 1)
            s.copy(2047, ln, 2)
            s.copy(2048, ln, 2)
            s.rlit(1 + k % 3)
    out.append(("far_2047_2048", far))

    def small4(s):
        s.rlit(9)
        for off in (1, 2, 3, 4, 7, 9):
            for ln in (1, 3, 4, 5, 11, 33, 64):
                s.copy(off, ln, 4)
    out.append(("copy4_small_offsets", small4))
    return out


@functools.lru_cache(None)
def family_matrix(front=False):
    cases = []
    for name, build in _matrix_streams(None):
        s = Stream(np.random.default_rng(len(cases) + 500))
        if front:
            s.rlit(FRONT)
        build(s)
        cases.append(_case(name + ("_front" if front else ""), s.finish(), len(cases) & 3, "global" if front else "lds"))
    return cases


# ---- e. fuzz ----------------------------------------------------------------------------------
LIT_CLASSES = ((1, 4), (59, 62), (63, 70), (255, 258), (259, 3000))
COPY_OFFSETS = tuple(range(1, 21)) + (63, 64, 65, 2047, 2048)


def random_valid_stream(rng, max_out, max_clen=W - 32):
    """A valid tag sequence of at most max_out output bytes in at most max_clen compressed ones
    (so it can enter the LDS path at any alignment).  Returns the Stream."""
    s = Stream(rng)
    max_tags = int(rng.integers(1, 700))
    budget = max_clen - 3   # (the preamble)

    def literal():
        room = min(max_out - s.pos, budget - s.clen - 5)
        if room < 1:
            return False
        lo, hi = LIT_CLASSES[int(rng.integers(len(LIT_CLASSES)))]
        n = int(rng.integers(lo, hi + 1))
        n = n if n <= room else int(rng.integers(1, room + 1))
        nb0 = 0 if n <= 60 else ((n - 1).bit_length() + 7) // 8
        nb = int(rng.integers(max(nb0, 1), 5)) if rng.random() < 0.3 else nb0
        s.rlit(n, nb)
        return True

    def copy(off=None):
        room = max_out - s.pos
        if s.pos == 0 or room < 1 or budget - s.clen < 5:
            return False
        kind = (1, 2, 4)[int(rng.integers(3))]
        if kind == 1 and room < 4:
            kind = 2
        if off is None:
            cand = [o for o in COPY_OFFSETS + (s.pos,) if o <= s.pos and (kind != 1 or o < 2048) and (kind != 2 or o < 65536)]
            off = cand[int(rng.integers(len(cand)))]
        elif kind == 1 and off >= 2048:
            kind = 2
        lo, hi = (4, 11) if kind == 1 else (1, 64)
        ln = int(rng.integers(lo, min(hi, room) + 1))
        s.copy(off, ln, kind)
        return ln

    literal()
    while s.ntags < max_tags and s.pos < max_out:
        x = rng.random()
        if x < 0.35:
            done = literal()
        elif x < 0.85:
            done = copy()
        else:   # a run of dependent copies, each reading the previous one's output
            done = prev = copy()
            for _ in range(int(rng.integers(1, 10))):
                if not prev:
                    break
                prev = copy(int(rng.integers(1, prev + 1)))
        if not done:
            break
    if rng.random() < 0.5:   # literals up to max_out (or the compressed budget)
        while literal():
            pass
    return s


def mutate(rng, stream):
    """1-3 bytes after the preamble overwritten (the announced length stays)."""
    h = 0
    while stream[h] & 0x80:
        h += 1
    h += 1
    m = bytearray(stream)
    for _ in range(int(rng.integers(1, 4))):
        m[int(rng.integers(h, len(m)))] = int(rng.integers(256))
    return bytes(m)


FUZZ_N = 300
MUT_INPUTS = ("text_150k", "markup_100k", "blobs_cfg4_200k", "pattern_4", "zeros_100k")


@functools.lru_cache(None)
def fuzz_valid(seed=1):
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(FUZZ_N):
        # (a quarter announce the whole window: only there can the output catch up with the tags)
        s = random_valid_stream(rng, W if rng.random() < 0.25 else int(rng.integers(1, W + 1)))
        built = s.finish()
        s0 = int(rng.integers(4))
        cases.append(_case(f"valid{seed}_{k}", built, s0, walk(built[0], s0).route))
    return cases


@functools.lru_cache(None)
def fuzz_mutated(seed=1):
    """(stream, s0): a mutation of each valid stream, 40 of each compressed corpus prefix."""
    from oracle import cpu
    rng = np.random.default_rng(seed + 1000003)
    out = [(mutate(rng, c.stream), c.s0) for c in fuzz_valid(seed)]
    c = corpus()
    for name in MUT_INPUTS:
        z = cpu.snappy_compress(c[name][:12000])
        out += [(mutate(rng, z), int(rng.integers(4))) for _ in range(40)]
    return out
