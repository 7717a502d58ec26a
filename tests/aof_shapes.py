"""Flat batches for rr_aof_batch where tests/test_gpu_aof.py's do not reach: a different score text in
every lane, a lane's parser state reused after a long number (inside a value, across rounds and across
the values of one wave), costs past 2^24, offsets past 2^32, wave_copy at every source x destination
alignment for bodies and keys, every "$len" / "*argc" digit seam, the intset widths' range rule, the
status precedence across rounds, and the batches of the host-entry and graph-replay tests.  Plain
Python and numpy on flat_forge.Flat, no GPU code.  tests/test_aof_shapes.py holds every builder to the
edge it is named for, with tests/aof_reference.py alone; tests/test_gpu_aof_edges.py holds the kernels
to the reference on them.

A builder returns a Shape: values, elems, arena, names (the keys), expires (or None) and meta, what
the tests need to know about where things sit."""
import collections
import random
import re
import struct

import numpy as np

import redrock_old_amd as rr
from oracle import pyoracle

import flat_forge as ff
import aof_reference as ar

WAVE = 64                                                 # RR_AOF_ITEMS_PER_CMD: a command is one wave round
SHORT_BODY = 32                                           # rr_stage_device.h: longer bodies go through wave_copy
L, SI, SH, HH, ZS, HZ, ZZ = (rr.T_LIST_QUICKLIST, rr.T_SET_INTSET, rr.T_SET_HT, rr.T_HASH_HT, rr.T_ZSET_SKIPLIST,
                             rr.T_HASH_ZIPLIST, rr.T_ZSET_ZIPLIST)
AGGREGATES = (L, SI, SH, HH, ZS, HZ, ZZ)
ZL = ("zl", b"x" * 30)                                    # only an empty ziplist's bytes are looked at

# score texts at the rounding edges and in every form of the grammar, and the texts that are not taken
# (tests/test_aof.py holds the host parser to them one by one)
HALFWAY = ["9007199254740993", "9007199254740992", "9007199254740994", "9007199254740995", "18014398509481990",
           "4.9406564584124654e-324", "4.9406564584124653e-324", "4.9406564584124655e-324", "9.8813129168249309e-324",
           "2.4703282292062328e-324", "2.4703282292062327e-324", "2.4703282292062329e-324",
           "7.4109846876186982e-324", "7.4109846876186981e-324", "7.4109846876186983e-324",
           "2.2250738585072014e-308", "2.2250738585072011e-308", "2.2250738585072009e-308",
           "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308",
           "1e309", "-1e309", "1e-400", "-1e-400", "0.1", "1.50", ".5", "5.", "1E5", "0", "-0", "0e0", "inf", "-inf",
           "100000000000000000000", "0.00000000000000000000000000000000000001", "1e0000000000000000000000000000000005",
           "1e99999999", "1e-99999999", "0e99999999", "00012.5000"]
REFUSED = ["nan", "-nan", "0x10", "+1", " 1", "1 ", "1e", "1e+", "", "-", ".", "123456789012345678", "1.2345678901234567891",
           "1" * 41, "0." + "0" * 38 + "1", "infinity", "INF", "Inf", "1.2.3", "1e5.0", "--1", "1,5", "١"]

Shape = collections.namedtuple("Shape", "values elems arena names expires meta")


def _word(rng, n):
    return bytes(rng.integers(97, 123, n, dtype=np.uint8))    # letters: never a number


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def add_aggregate(f, typ, cnt, k=0):
    """One value of the aggregate encoding typ with cnt items; a ziplist's entries are mixed STR and INT."""
    rng = f.rng
    w = lambda: _word(rng, int(rng.integers(0, 40)))
    if typ == rr.T_LIST_QUICKLIST:
        return f.add(typ, 0, [w() if j % 3 else int(rng.integers(-10**6, 10**6)) for j in range(cnt)])
    if typ == rr.T_SET_INTSET:
        return f.add(typ, 8, [int(rng.integers(-2**62, 2**62)) for _ in range(cnt)])
    if typ == rr.T_SET_HT:
        return f.add(typ, 0, [b"%d" % j + w() for j in range(cnt)])
    if typ == rr.T_HASH_HT:
        return f.add(typ, 0, [x for j in range(cnt) for x in (b"f%d" % j + w(), w())])
    if typ == rr.T_ZSET_SKIPLIST:
        return f.add(typ, 0, [x for j in range(cnt) for x in (b"m%d" % j + w(), ("score", _bits((j - 7) * 0.375 + k)))])
    zl = ("zl", pyoracle.build_ziplist([]) if cnt == 0 else _word(rng, 30))   # only an empty one's bytes are looked at
    if typ == rr.T_HASH_ZIPLIST:
        return f.add(typ, 0, [zl] + [x for j in range(cnt) for x in (b"f%d" % j, int(rng.integers(-300, 300)) if j % 2 else w())])
    return f.add(typ, 0, [zl] + [x for j in range(cnt) for x in (b"m%d" % j if j % 4 else j,
                                                                  b"%.17g" % ((j - 5) / 8) if j % 3 else j - 9)])


def _zz(f, scores, tag=b"m"):
    """A ZSET_ZIPLIST whose item j (lane j % 64 of round j // 64) has the score entry scores[j]."""
    return f.add(ZZ, 0, [ZL] + [x for j, s in enumerate(scores) for x in (tag + b"%d" % j, s)])


def _shape(f, names=None, expires=None, **meta):
    v, e, a = f.done()
    return Shape(v, e, a, names if names is not None else [b"k%d" % i for i in range(len(v))], expires, meta)


def reference(s, **kw):
    """tests/aof_reference.aof_batch on a Shape: (data, offsets, status, totals, slices)."""
    kd, ko = ar.keys_of(s.names)
    exp = None if s.expires is None else np.asarray(s.expires, np.int64)
    return ar.aof_batch(s.values, s.elems, s.arena, kd, ko, exp, **kw)


def ndig(v):
    return len(str(v))


def bulk_len(n):
    """The bytes of the bulk string of n bytes: "$n\\r\\n" | n bytes | "\\r\\n"."""
    return 5 + ndig(n) + n


# ---- what a score text asks of the parser (csrc/rr_strtod_impl.h), restated ----------------------------------------
_TEXT = re.compile(rb"(-?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?")


def decimal_parts(text):
    """(M, nd, E) of a text of the grammar: the value is +-M * 10^E, M with nd digits and no trailing zero."""
    m = _TEXT.fullmatch(bytes(text))
    ip, fp = m.group(2) or b"", m.group(3) or m.group(4) or b""
    sig = (ip + fp).lstrip(b"0")
    cut = sig.rstrip(b"0")
    return int(cut or b"0"), len(cut), int(m.group(5) or 0) - len(fp) + len(sig) - len(cut)


def first_exponent(text):
    """The decimal exponent of the first significant digit; None for zero, "inf" and "-inf"."""
    if bytes(text) in (b"inf", b"-inf"):
        return None
    M, nd, E = decimal_parts(text)
    return E + nd - 1 if M else None


def parse_words(text):
    """The 32-bit words of multi-word state rr_s2d_scale starts from (E < 0: M << S) or ends with (E >= 0:
    M * 5^E); 0 where it returns before touching the state."""
    first = first_exponent(text)
    if first is None or first >= 310 or first < -326:
        return 0
    M, _, E = decimal_parts(text)
    if E >= 0:
        return ((M * 5**E).bit_length() + 31) // 32
    return ((M << (((-E * 2379) >> 10) + 65)).bit_length() + 31) // 32


# ---- A. score texts, a different one in every lane ----------------------------------------------------------------
SEAM_EXPONENTS = (12, 13, 14, 26, 27, 308, 309, -12, -13, -14, -26, -27, -325, -326, -341, -342)   # 13 a step
N_TEXTS = 4096
LAST_TEXT = b"2.2250738585072011e-308"                    # ends at the arena's last byte


def _form(rng, m, e, form):
    s = str(m)
    return ("%de%d" % (m, e), "%s.%sE%+d" % (s[0], s[1:], e), "-.%de%d" % (m, e), "%d.e%d" % (m, e))[form].encode()


def score_texts(seed=20250):
    """N_TEXTS texts, all taken: HALFWAY; the seam exponents with a 1-digit and a 17-digit mantissa; texts of
    exactly 39 and 40 bytes; 17 significant digits with zeros across the point; 1,100 random mantissas in the
    four forms of tests/test_aof.py whose first digit sits at 10^-330 .. 10^-301; the same with the exponent
    uniform over [-345, 310] for the rest; shuffled, with LAST_TEXT kept last."""
    rng = random.Random(seed)
    out = [t.encode() for t in HALFWAY]
    out += [b"%de%d" % (m, e) for e in SEAM_EXPONENTS for m in (7, 12345678901234567)]
    for ln in (39, 40):
        out += [b"0" * (ln - 4) + b"12.5", b"1e" + b"0" * (ln - 5) + b"305", b"-1.25E-" + b"0" * (ln - 10) + b"310",
                b"0." + b"0" * (ln - 19) + b"12345678901234567"]
    out += [b"12345000.000012345", b"1" + b"0" * 7 + b"." + b"0" * 8 + b"1", b"-90000000.00000001e-320",
            b"1234567.0000054321e300", b"100000000000.00001e-330", b"-1000.0000000000001E+305"]
    for k in range(N_TEXTS - 1 - len(out)):
        nd = rng.randint(1, 17)
        m = rng.randint(10 ** (nd - 1), 10 ** nd - 1)
        form = rng.randint(0, 3)
        if k < 1100:
            first = rng.randint(-330, -301)
            e = max(-345, (first - nd + 1, first, first + 1, first - nd + 1)[form])
        else:
            e = rng.randint(-345, 310)
        out.append(_form(rng, m, e, form))
    rng.shuffle(out)
    return out + [LAST_TEXT]


def score_text_batch():
    """64 ZSET_ZIPLISTs of 64 items: text 64 v + j is the score entry of value v's lane j.  The last score
    text is the last thing put into the arena."""
    texts = score_texts()
    f = ff.Flat(41)
    for v in range(N_TEXTS // WAVE):
        _zz(f, texts[WAVE * v:WAVE * (v + 1)])
    return _shape(f, texts=texts)


N_INTS = 512


def score_ints(seed=20251):
    """N_INTS integer score entries: +-(2^53 + k), +-(2^63 - 1 - k), -2^63, +-2^k and +-(2^k +- 1) for k in
    53 .. 62 (where (double) v rounds), then random 63-bit values of both signs."""
    rng = random.Random(seed)
    out = [s * (2**53 + k) for k in range(9) for s in (1, -1)]
    out += [s * (2**63 - 1 - k) for k in range(8) for s in (1, -1)] + [-2**63]
    out += [s * (2**k + d) for k in range(53, 63) for d in (0, 1, -1) for s in (1, -1)]
    while len(out) < N_INTS:
        out.append(rng.choice((1, -1)) * rng.getrandbits(63))
    rng.shuffle(out)
    return out


def score_int_batch():
    ints = score_ints()
    f = ff.Flat(42)
    for v in range(N_INTS // WAVE):
        _zz(f, ints[WAVE * v:WAVE * (v + 1)])
    return _shape(f, ints=ints)


def refused_lane(j):
    return (63 + 11 * j) % WAVE                           # 11 is odd: a different lane for each of 64 values


def refused_batch():
    """Every text of REFUSED as one score entry of its own 192-item ZSET_ZIPLIST, text j at lane
    refused_lane(j) of round j % 3, every other score taken; a String behind each."""
    f = ff.Flat(43)
    names, at = [], []
    for j, t in enumerate(REFUSED):
        pos = WAVE * (j % 3) + refused_lane(j)
        scores = [b"%d.5" % k if k % 2 else k - 60 for k in range(3 * WAVE)]
        scores[pos] = t.encode()
        _zz(f, scores)
        f.add(rr.T_STRING, 0, [b"neighbour %d" % j])
        names += [b"bad%d" % j, b"good%d" % j]
        at.append(pos)
    return _shape(f, names, [5] * len(names), at=at)


# ---- B. a lane's state after a long number ------------------------------------------------------------------------
LONG_TEXT = b"12345678901234567e-340"                     # 29 words
SCHEDULES = ((LONG_TEXT, b"1", 1),
             (b"1", LONG_TEXT, b"1e308"),
             (b"1e308", b"5e-324", b"0.5"),
             (2**63 - 1, b"1e-300", b"inf"),
             # "a skiplist-style value follows a long parse", as it can be had inside one ZSET_ZIPLIST (a SCORE
             # descriptor there is RR_E_ENCODE): texts that are what a skiplist's SCOREs print, 32 words of print
             # over 29 of parse.  A real ZSET_SKIPLIST behind a long parse on the same lanes is in
             # stale_values_batch (the pairs ZZ long -> ZS)
             (LONG_TEXT, b"-1.7976931348623157e+308", b"2.2250738585072014e-308"))
FIFTH_LANES = (5, 30, 63)


def schedule_of(lane):
    return SCHEDULES[4] if lane in FIFTH_LANES else SCHEDULES[lane % 4]


def stale_rounds_batch():
    """One ZSET_ZIPLIST of 192 items: lane j's three rounds take schedule_of(j) in turn."""
    f = ff.Flat(44)
    _zz(f, [schedule_of(j % WAVE)[j // WAVE] for j in range(3 * WAVE)])
    f.add(rr.T_STRING, 0, [b"behind"])
    return _shape(f)


STALE_PAIRS = 8
# (first visit, second visit) of pair p, a ZSet of 70 items each: every order of the two encodings, long
# first on even p, short first on odd p
_PAIR_TYPES = ((ZZ, ZS), (ZS, ZS), (ZZ, ZZ), (ZS, ZZ), (ZS, ZS), (ZZ, ZS), (ZS, ZZ), (ZZ, ZZ))


def _stale_zset(f, typ, long, p):
    if typ == ZZ:
        _zz(f, [(b"%d%de-%d" % (1234567890123456, j % 10, 325 + (j + p) % 16)) if long else b"%d" % (j % 10) for j in range(70)])
    else:                                                 # subnormals: 34 words of print
        f.add(ZS, 0, [x for j in range(70) for x in (b"s%d" % j, ("score", (3**30 + 7**14 * (j + p)) if long else _bits(float(j % 10))))])


def stale_values_batch():
    """RR_AOF_MAX_WAVES + 8 values: value v and value v + RR_AOF_MAX_WAVES run on one wave of both kernels.
    Values 0 .. 7 and their partners are 70-item ZSets (_PAIR_TYPES), one of a pair with long numbers in
    every lane, the other with single digits; everything between is one shared one-element String."""
    f = ff.Flat(45)
    for p in range(STALE_PAIRS):
        _stale_zset(f, _PAIR_TYPES[p][0], p % 2 == 0, p)
    b = len(f.elems)
    f.elems.append((f.put(b"v"), 1, rr.K_STR, 0, 0))
    f.elems.append((7, 0, rr.K_INT, 0, 0))
    f.values += [(rr.T_STRING, (0, 1)[i % 2], 0, 0, 1, b + i % 2) for i in range(STALE_PAIRS, rr.AOF_MAX_WAVES)]
    for p in range(STALE_PAIRS):
        _stale_zset(f, _PAIR_TYPES[p][1], p % 2 == 1, p)
    n = rr.AOF_MAX_WAVES + STALE_PAIRS
    return _shape(f, [b"%d" % (i % 10) for i in range(n)])


# ---- C. costs past 2^24 -------------------------------------------------------------------------------------------
SEAM = 1 << 24
MIB = 1 << 20


def seam24_batch():
    """Aliased descriptors on one region of 2^24 + 64 letters: Strings of 2^24 - 1, 2^24 and 2^24 + 1
    bytes; a List of 5, 6 and 6 MiB and then a 3-byte member (placed above 2^24 in its command); a HASH_HT
    pair of 2^24 - 10 and 100 bytes (one lane's cost and payload above 2^24); a SET_HT of 64 members of
    300,000 bytes (the lanes' low 24 bits sum past 2^24)."""
    f = ff.Flat(46)
    at = len(f.arena)
    f.arena += _word(f.rng, SEAM + 64)
    raw = lambda off, ln: ("raw", rr.K_STR, at + off, ln, 0, 0)
    meta = {}
    for k, ln in enumerate((SEAM - 1, SEAM, SEAM + 1)):
        f.add(rr.T_STRING, 0, [raw(k, ln)])
    meta["list"] = f.add(L, 0, [raw(3, 5 * MIB), raw(5 * MIB, 6 * MIB), raw(7, 6 * MIB), raw(11, 3)])
    meta["hash"] = f.add(HH, 0, [raw(9, SEAM - 10), raw(1000, 100)])
    meta["set"] = f.add(SH, 0, [raw(37 * j, 300000) for j in range(WAVE)])
    f.add(rr.T_STRING, 0, [b"behind"])
    return _shape(f, expires=[-1, 7, -1, 8, -1, 9, -1], tail=bytes(f.arena[at + 11:at + 14]), **meta)


# ---- D. offsets past 2^32 -----------------------------------------------------------------------------------------
NBIG, BIG_LEN = 66000, 65536


def past_4gib_batch():
    """The reduced batch of the 4 GiB test: one String of BIG_LEN bytes, then one value of every aggregate
    encoding with 130 items, each with an expiry; one-byte keys.  The test repeats the String's record
    NBIG times over the same descriptor."""
    f = ff.Flat(47)
    f.add(rr.T_STRING, 0, [_word(f.rng, BIG_LEN)])
    for typ in AGGREGATES:
        add_aggregate(f, typ, 130, k=2)
    n = 1 + len(AGGREGATES)
    return _shape(f, [b"k"] + [b"%d" % i for i in range(1, n)], [-1] + [1700000000000 + i for i in range(1, n)])


def past_4gib_expect(offs1, totals1, totals_big, n_tail):
    """(offsets, totals) of NBIG copies of value 0 followed by the tail, from the reference's answer on the
    reduced batch (offs1, totals1) and on value 0 alone (totals_big)."""
    row = int(offs1[1])
    offsets = np.concatenate([np.arange(NBIG - 1, dtype=np.uint64) * np.uint64(row), offs1 + np.uint64((NBIG - 1) * row)])
    totals = {k: totals1[k] + (NBIG - 1) * totals_big[k] for k in ("n_elems", "bytes", "payload")}
    totals["n_bad"] = totals1["n_bad"]
    assert len(offsets) == NBIG + n_tail + 1
    return offsets, totals


# ---- E. wave_copy at every source x destination alignment -----------------------------------------------------------
BODY_SMALL, BODY_LONG, LONG_SRC = (33, 48, 49), (1039, 1040, 1071), (0, 1, 7, 15)
KEY_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 1039)
FILLERS = tuple(range(15)) + (25,)                        # their bulk strings' lengths: every residue of 16 once
_SET_HEAD = 13                                            # "*3\r\n$3\r\nSET\r\n"


def _pad_for(want, fixed):
    """The length p of a pad String's value with (fixed + bulk_len(p)) % 16 == want."""
    return next(p for p in range(26) if (fixed + bulk_len(p)) % 16 == want)   # 25 letters: 32 bytes


def body_alignment_batch(pads=None):
    """Bodies that wave_copy moves, in a List behind a filler item and as the value of a HASH_HT pair behind
    a filler field: source alignment (the arena padded) x the 16 FILLERS (a filler of 10 letters takes a
    second length digit, so they are not 0 .. 15).  A String behind each value brings the next value to a multiple of 16 (pads: the
    length of its value, from the sizes of a first build without them).  meta: the values' indices and the
    (source alignment, body) of each."""
    f = ff.Flat(48)
    rng = f.rng
    at, info = [], []
    combos = [(ln, a, s) for ln in BODY_SMALL for a in range(16) for s in FILLERS]
    combos += [(ln, a, s) for ln in BODY_LONG for a in LONG_SRC for s in FILLERS]
    for typ in (L, HH):
        for ln, a, s in combos:
            f.arena += bytes((a - len(f.arena)) % 16)
            body = _word(rng, ln)
            src = len(f.arena)
            f.arena += body
            at.append(f.add(typ, 0, [_word(rng, s), ("raw", rr.K_STR, src, ln, 0, 0)]))
            info.append((a, body))
            f.add(rr.T_STRING, 0, [b"p" * (pads[len(at) - 1] if pads else 0)])
    return _shape(f, [b"kk"] * len(f.values), at=at, info=info)


def body_alignment_pads(sizes, at):
    """The pads of the second build from the sizes the reference gives the first one."""
    return [_pad_for(0, int(sizes[i]) + _SET_HEAD + bulk_len(2)) for i in at]


def body_alignment():
    """body_alignment_batch with its pads: built twice, the reference sizing the first build."""
    s = body_alignment_batch()
    sizes = np.diff(reference(s)[1].astype(np.int64))
    return body_alignment_batch(body_alignment_pads(sizes, s.meta["at"]))


def key_alignment_batch():
    """A String per (key length, key source alignment, key destination alignment).  Key slices lie back to
    back, so the key of a pad String in front of each brings the key's source to its alignment, and the
    length of the pad's value brings the key's place in the output to its alignment.  meta: the values'
    indices and the (source alignment, destination alignment, key) of each."""
    f = ff.Flat(49)
    rng = f.rng
    names, at, info = [], [], []
    kpos = opos = 0
    one = f.put(b"v")
    for kl in KEY_LENGTHS:
        for a in range(16):
            for d in range(16):
                kp = (a - kpos - 1) % 16 + 1
                # the pad's command, then "*3 SET" and "$kl\r\n" of the value under test
                p = _pad_for(d, opos + _SET_HEAD + bulk_len(kp) + _SET_HEAD + 3 + ndig(kl))
                f.add(rr.T_STRING, 0, [b"p" * p])
                names.append(_word(rng, kp))
                key = _word(rng, kl)
                at.append(f.add(rr.T_STRING, 0, [("raw", rr.K_STR, one, 1, 0, 0)]))
                names.append(key)
                info.append((a, d, key))
                kpos += kp + kl
                opos += _SET_HEAD + bulk_len(kp) + bulk_len(p) + _SET_HEAD + bulk_len(kl) + bulk_len(1)
    return _shape(f, names, at=at, info=info)


# ---- F. where "$len" and "*argc" grow a digit ----------------------------------------------------------------------
MEMBER_SEAMS = (9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000)
EXPIRY_SEAMS = (-2**63, -2, 0, 999999999999, 10**12)


def digit_seam_batch():
    f = ff.Flat(50)
    rng = f.rng
    items = [x for ln in MEMBER_SEAMS for x in (_word(rng, ln), _word(rng, 2))]
    items += [-2**63, 2**63 - 1, -1, 0] + [x for k in range(1, 19) for x in (10**k, 10**k - 1)]
    f.add(L, 0, items)
    for typ in (L, SI, SH):
        for c in (7, 8, 64 + 7, 64 + 8):                  # "*9", "*10", as a value's only and as its last command
            add_aggregate(f, typ, c)
    for typ in (HH, ZS, HZ, ZZ):
        for c in (3, 4, 48, 49, 64 + 48, 64 + 49):        # "*8", "*10", "*98", "*100"
            add_aggregate(f, typ, c)
    names = [b"k%d" % i for i in range(len(f.values))]
    for kl in (999, 1000):
        f.add(rr.T_STRING, 0, [_word(rng, 5)])
        add_aggregate(f, HH, 70)
        names += [_word(rng, kl), _word(rng, kl)]
    return _shape(f, names, [EXPIRY_SEAMS[i % 5] for i in range(len(names))])


# ---- G. the intset widths' range rule ------------------------------------------------------------------------------
INTSET_PLACES = (0, 63, 70)                               # lane 0, lane 63, the second round


def intset_batch():
    """SET_INTSETs of 100 members.  For width 2 and 4 and each place: the two inclusive limits (status 0) and
    each limit's outer neighbour (RR_E_ENCODE), good and bad in turn; widths 0, 1, 3 and 16; width 8 with
    -2^63 and 2^63 - 1.  meta["bad"]: the indices that are RR_E_ENCODE."""
    f = ff.Flat(51)
    bad = []
    fill = lambda: [int(x) for x in f.rng.integers(-30000, 30000, 100)]
    for w in (2, 4):
        lim = 1 << (8 * w - 1)
        for place in INTSET_PLACES:
            for edge, off in ((-lim, -1), (lim - 1, 1)):
                for x in (edge, edge + off):
                    items = fill()
                    items[place] = x
                    i = f.add(SI, w, items)
                    if x != edge:
                        bad.append(i)
    f.add(rr.T_STRING, 0, [b"between"])
    for w in (0, 1, 3, 16):
        bad.append(f.add(SI, w, [1, 2, 3]))
    for place in INTSET_PLACES:
        items = fill()
        items[place], items[place + 1] = -2**63, 2**63 - 1
        f.add(SI, 8, items)
    return _shape(f, bad=bad)


# ---- H. status precedence across rounds ----------------------------------------------------------------------------
def precedence_batch():
    """ZSET_ZIPLISTs whose round 0 holds a refused score text and whose later round holds what RR_E_ENCODE
    is for (meta["encode"]); the same values with a good round 0 and the refused text in round 3
    (meta["cpu"]); a ZSET_SKIPLIST with a NaN in round 0 and a STR where round 1 wants a SCORE."""
    f = ff.Flat(52)
    encode, cpu, past = [], [], []

    def zz(items, refused_at, forged=None):
        ents = []
        for j in range(items):
            ents += [b"m%d" % j, b"nan" if j == refused_at else b"%d.25" % j]
        if forged:
            ents[forged[0]] = forged[1]
        return f.add(ZZ, 0, [ZL] + ents)

    for items, pos, d in ((200, 2 * (WAVE + 9), ("raw", 9, 0, 0, 0, 0)),                    # a member of round 1
                          (200, 2 * (2 * WAVE + 40) + 1, ("score", _bits(1.5))),            # a score entry of round 2
                          (256, 2 * (3 * WAVE + 63) + 1, "past"),                           # round 3, lane 63
                          (200, 2 * (3 * WAVE + 7), "past")):                               # round 3's last lane of 8
        i = zz(items, 17, (pos, b"xyz" if d == "past" else d))
        if d == "past":
            past.append(int(f.values[i][5]) + 1 + pos)
        encode.append(i)
    f.add(rr.T_STRING, 0, [b"between"])
    cpu += [zz(200, 3 * WAVE + 2), zz(256, 3 * WAVE + 63)]                                  # the mirrors
    f.add(rr.T_STRING, 0, [b"between"])
    pairs = [x for j in range(70) for x in (b"s%d" % j, ("score", 0x7FF8000000000000 if j == 5 else _bits(j / 4)))]
    pairs[2 * (WAVE + 3) + 1] = b"not a score"
    encode.append(f.add(ZS, 0, pairs))
    pairs = [x for j in range(70) for x in (b"s%d" % j, ("score", 0xFFF0000000000001 if j == 69 else _bits(j / 4)))]
    cpu.append(f.add(ZS, 0, pairs))
    f.arena += b"end"
    v, e, a = f.done()
    for k in past:                                        # a STR that ends one byte past the arena
        e["data"][k] = len(a) + 1 - int(e["len"][k])
    return Shape(v, e, a, [b"k%d" % i for i in range(len(v))], [4] * len(v), {"encode": encode, "cpu": cpu})


# ---- I. the host entry and graph replay -----------------------------------------------------------------------------
def capacity_batch():
    """An empty Set, one value of every aggregate encoding with 65 items, a String."""
    f = ff.Flat(17)
    f.add(rr.T_SET_HT, 0, [])                                 # size 0 at offset 0: fits any capacity
    for typ in AGGREGATES:
        add_aggregate(f, typ, 65)
    f.add(rr.T_STRING, 0, [b"last"])
    return _shape(f)


def refused_blobs():
    """Rock blobs of ZSET_ZIPLISTs whose score texts rr_aof_batch leaves to the CPU path, and one it takes."""
    out = []
    for items in ([b"a", b"nan"], [b"a", b"1.5", b"b", b"0x10", b"c", b"2"], [b"m", b"1e", b"n", 7], [b"ok", b"2.5", b"i", 3]):
        z = pyoracle.build_ziplist(items)
        out.append(bytes([ZZ]) + struct.pack("<IQ", 0, len(z)) + z)
    return out
