"""Score and payload generators for rr_d2string_batch and rr_rdbzset_batch past one round and one value a
wave: every biased exponent with full mantissas, the range where d2string's notation and ll2string's
window switch, a d2string batch one wave and one slot past the launch's grid cap, ZSets that make every
lane print wide, widest, short, wide in sequence, printed scores at every ziplist integer encoding's
edge and in a wave's last text slot, and a batch in which every wave converts a second ZSet.  Plain
Python and numpy, no GPU code.  tests/test_rdbzset_shapes.py holds the generators to what they claim
and the yardstick (tests/rdbzset_reference.d2string) and the host's rr_d2string to the C library on
them; tests/test_gpu_rdbzset_shapes.py holds the kernels to the reference.

The payload generators return a list of (payload, opts), one opts object for the whole list, so that a
list is one batch; every value is a ZSET_2."""
import functools
import itertools

import numpy as np

import rdbconvert_reference as cv
import rdbload_reference as ld
import rdbzset_reference as zr
from test_d2string import random_bits                     # noqa: F401  (the third score list, as it stands)
from test_rdbzset import zset

# rr_launch_d2string (csrc/rr_rdbzset.hip): at most 16384 workgroups of D2S_WPB = 4 waves of RR_WAVE lanes
D2S_GRID_CAP = 16384
D2S_WPB = 4
RR_WAVE = 64
D2S_ROUND = D2S_GRID_CAP * D2S_WPB * RR_WAVE              # scores a full grid prints in one round
N2 = D2S_ROUND + RR_WAVE + 1                              # wave 0 a full second round, wave 1 one slot of one
T = 4093                                                  # the table's length: prime, so coprime to the round
SHIFT = D2S_ROUND % T                                     # score i + D2S_ROUND is table[(i % T + SHIFT) % T]


def word_count(bits):
    """RR_D2S_WORDS of them a lane: the words rr_d2s_print's multi-word state takes for a finite non-zero
    double m * 2^e (csrc/rr_d2string_impl.h): the integer m << e, or the fraction's ceil(-e / 32)."""
    mag = bits & 0x7FFFFFFFFFFFFFFF
    bexp = mag >> 52
    assert 0 < mag and bexp != 0x7FF
    e = (bexp or 1) - 1075
    return (e + 53 + 31) >> 5 if e >= 0 else (-e + 31) >> 5


def live_words(bits):
    """The 32-bit words of that state that are not zero before the first multiplication or division."""
    mag = bits & 0x7FFFFFFFFFFFFFFF
    bexp = mag >> 52
    m = (mag & 0xFFFFFFFFFFFFF) | (1 << 52) if bexp else mag
    e = (bexp or 1) - 1075
    n = word_count(bits)
    v = m << e if e >= 0 else (m & ((1 << -e) - 1)) << (32 * n + e)
    return sum(1 for k in range(n) if (v >> (32 * k)) & 0xFFFFFFFF)


# ---- 1. every exponent, full mantissas --------------------------------------------------------------------
def stratified_bits(per=64, seed=5):
    """For every biased exponent 0 .. 2046 (no infinity, no NaN): `per` uniformly random 52-bit mantissas
    and the two extreme ones, 0x0000000000001 and 0xFFFFFFFFFFFFF, each with a random sign; exponent by
    exponent, (per + 2) * 2047 patterns.  Every word count and shift of both branches, with lo64, the
    third word and the sticky bit all decided by a full mantissa."""
    rng = np.random.default_rng(seed)
    man = rng.integers(0, 1 << 52, (2047, per + 2), dtype=np.uint64)
    man[:, per] = 1
    man[:, per + 1] = (1 << 52) - 1
    exp = np.repeat(np.arange(2047, dtype=np.uint64), per + 2)
    sign = rng.integers(0, 2, exp.size, dtype=np.uint64)
    return (sign << np.uint64(63)) | (exp << np.uint64(52)) | man.ravel()


# ---- 2. where the notation switches -------------------------------------------------------------------------
WINDOW_EDGES = (2.0**52 - 1, 2.0**52, 2.0**52 - 2, 2.0**52 - 0.5, 2.0**52 + 1, 2.0**53, 2.0**63, 1e15, 1e16, 1e17, 1e18,
                99999999999999984.0, 9.9999999999999991e-05, 0.0001, 0.001, 1e-5, 1e-6, 0.5, 1.0)


def window_bits(n=100_000, seed=7):
    """Doubles of both signs with magnitudes log-uniform over 1e-6 .. 1e18, a quarter of them each: as they
    fall; exact integers below 2^52 (ll2string's window, util.c:542-545); integers in [2^52, 2^63], which
    %.17g prints (16 to 19 digits, "e+17" and "e+18" from 1e17 on); integers below 2^51 plus 0.5.  Then
    WINDOW_EDGES, both signs: the window's two edges +-(2^52 - 1) and +-2^52 among them."""
    rng = np.random.default_rng(seed)
    q = n // 4
    as_they_fall = 10.0 ** rng.uniform(-6, 18, n - 3 * q)
    small_int = np.floor(2.0 ** rng.uniform(0, 52, q))
    big_int = np.minimum(np.floor(2.0 ** rng.uniform(52, 63, q)), 2.0**63)
    halves = np.floor(2.0 ** rng.uniform(0, 51, q)) + 0.5
    v = np.concatenate([as_they_fall, small_int, big_int, halves])
    assert (small_int < 2.0**52).all() and (big_int >= 2.0**52).all() and (halves % 1 == 0.5).all()
    v *= rng.choice([-1.0, 1.0], v.size)
    edges = np.array([s * e for e in WINDOW_EDGES for s in (1.0, -1.0)])
    return np.concatenate([v, edges]).view(np.uint64)


# ---- 3. d2string_kernel's second round ----------------------------------------------------------------------
SHORT_BITS = (0x0000000000000000, 0x3FF8000000000000, 0x7FF0000000000000, 0x7FF8000000000000,     # "0" "1.5" "inf" "nan"
              0x8000000000000000, 0xFFF0000000000000, 0xFFFFFFFFFFFFFFFF, 0x4031000000000000)     # "-0" "-inf" "nan" "17"
# the kind of table[j], by j % 4, below SHIFT and from SHIFT on: a lane of the first 65 prints kind
# FIRST[l % 4] in its first round and SECOND[l % 4] in its second
INTEGER_BEXP = (2035, 2035, 2003, 1971, 1939)            # e = 960, 928, 896, 864: the shift is 0 (see round_two_table)
KIND_FIRST = ("fraction", "short", "fraction", "integer")
KIND_SECOND = ("short", "integer", "integer", "short")


def table_kind(j):
    return KIND_FIRST[j % 4] if j < SHIFT else KIND_SECOND[(j - SHIFT) % 4]


@functools.lru_cache(maxsize=None)
def _round_two_table():
    rng = np.random.default_rng(31)
    out, shorts = [], 0
    for j in range(T):
        kind = table_kind(j)
        if kind == "short":                                # the specials in turn between distinct k + 0.5 and k / 4
            b = SHORT_BITS[shorts // 2 % len(SHORT_BITS)] if shorts % 2 == 0 else zr.to_bits(shorts // 2 + (0.5 if shorts % 4 == 1 else 0.25))
            shorts += 1
        else:
            while True:                                    # 24 bytes of text: negative, 17 digits, a 3-digit exponent
                if kind == "fraction":                     # biased exponent 0 .. 18: all RR_D2S_WORDS = 34 words
                    b = (1 << 63) | int(rng.integers(1, 19 << 52))
                else:                                      # m << e with e a multiple of 32: 29 to 32 words
                    b = (1 << 63) | (int(rng.choice(INTEGER_BEXP)) << 52) | int(rng.integers(0, 1 << 52))
                if len(zr.d2string(b)) == zr.D2STRING_MAX:
                    break
        out.append(b)
    return np.array(out, np.uint64)


def round_two_table():
    """T scores.  "fraction": a negative subnormal or a normal below 2^-1004, 34 words of state, 24 bytes
    of text; "integer": a negative double m * 2^e with e a multiple of 32 (INTEGER_BEXP), 29 to 32 words,
    24 bytes; "short": "0", "1.5", "inf", "nan", "-0", "-inf", "17" and small multiples of a quarter, at
    most 7 bytes.  Long and short alternate by table_kind, which turns over at SHIFT so that a lane's
    second score is of another kind than its first: a short text over a long one's slot, and a multi-word
    integer laid into state words a fraction's multiplications left behind.  A subnormal's print leaves
    words 11 .. 33 non-zero.  The integer branch writes the two or three words m << e occupies and relies
    on the words below them being zero; what is left there adds less than 2^-(52 + e % 32) of the value,
    so it shows in 17 digits only when e % 32 is 0 or close to it.  Hence these exponents."""
    return _round_two_table().copy()


def round_two_bits():
    """N2 scores for rr_d2string_batch: table[i % T].  The launch caps its grid at D2S_GRID_CAP workgroups,
    so the waves stride by D2S_ROUND: wave 0 of workgroup 0 prints scores 0 .. 63 and then
    D2S_ROUND .. D2S_ROUND + 63, wave 1 prints 64 .. 127 and then the one score D2S_ROUND + 64 with
    left == 1, every other wave prints one round."""
    return _round_two_table()[np.arange(N2) % T]


# ---- 4. what one lane prints in sequence inside a ZSet ---------------------------------------------------------
LANE_OPTS = ld.options(zset_max_ziplist_entries=512)
# (words of state, lengths of text) of the bands, 64 ranks each, in the skiplist's order
LANE_BANDS = ((("integer", 32, (24,)), ("fraction", 34, (23, 24)), ("short", 2, (3, 4, 5)), ("integer", 32, (23,))),
              (("short", 2, (4, 5, 6)), ("fraction", 33, (24,)), ("fraction", 34, (24,)), ("fraction", 34, (23,))))


def _take(n, length, make):
    """The first n of make(0), make(1), ... whose text has `length` bytes (%.17g drops trailing zeros)."""
    out = []
    for j in itertools.count():
        v = make(j)
        if len(zr.d2string(zr.to_bits(v))) == length and v not in out:
            out.append(v)
            if len(out) == n:
                return out


def _band_scores():
    huge_neg = _take(64, 24, lambda j: -(1.0e308 + 1.0e305 * j))                 # 32 words, "-1.0000000000000001e+308"
    tiny = _take(32, 24, lambda j: -5e-324 * (3**32 + 7**15 * j))                # negative subnormals
    tiny += _take(16, 23, lambda j: 5e-324 * (5**20 + 11**12 * j))               # positive subnormals
    tiny += _take(16, 23, lambda j: 3.0e-304 * (1 + j / 64) + j * 1e-310)        # normals below 2^-1004: still 34 words
    halves = [float(h) + 0.5 for h in list(range(0, 22)) + list(range(40, 61)) + list(range(100, 121))]
    pow1012 = _take(64, 23, lambda j: 2.0**1012 * (1 + j / 128) + 2.0**962 * j)  # m * 2^960: 32 words, the shift 0
    e300 = _take(64, 24, lambda j: -1.0e-300 * (1 + j / 128) - j * 1e-310)       # about -1e-300: 33 words
    sub_neg = _take(64, 24, lambda j: -5e-324 * (3**32 + 13**11 * j))
    sub_pos = _take(64, 23, lambda j: 5e-324 * (7**17 + 3**25 * j))
    return (huge_neg, tiny, halves, pow1012), ([-h for h in halves], e300, sub_neg, sub_pos)


def lane_sequence_zsets():
    """Two ZSets of 256 members under zset_max_ziplist_entries = 512.  zset_value's lane l prints ranks l,
    64 + l, 128 + l and 192 + l into the same state words and slot.  In the skiplist's order the first
    ZSet's ranks 0-63 are negative doubles near 1e308 (the integer branch, 32 words, 24 bytes), 64-127
    negative then positive subnormals and normals near 1e-304 (34 words, 24 and 23 bytes), 128-191 k + 0.5
    (one live word of two, 3 to 5 bytes) and 192-255 doubles in [2^1012, 2^1013) (32 words again, the lowest
    of m << 960 directly above what the fractions left, see round_two_table): wide, widest, short, wide on
    every lane.  The second starts short and ends on the
    subnormals: -(k + 0.5), doubles near -1e-300 (33 words), negative subnormals, positive subnormals.
    (No integer-branch band fits there: a double of 2^52 or more sorts outside every fraction.)  The
    payload order is a fixed shuffle, so the rank sort decides who prints what."""
    out = []
    for z, bands in enumerate(_band_scores()):
        scores = [s for band in bands for s in band]
        assert len(scores) == 256 == len(set(scores))
        items = [(b"m%03d" % (j * 97 % 256), s) for j, s in enumerate(scores)]
        perm = np.random.default_rng(40 + z).permutation(256)
        out.append((zset([items[j] for j in perm]), LANE_OPTS))
    return out


# ---- 5. printed scores that are integer entries -----------------------------------------------------------------
INT_OPTS = ld.options(zset_max_ziplist_entries=512)
INT_EDGES = (0, 12, 13,
             -1, -128, -129, 127, 128,
             32767, -32767, 32768, -32768, 32769, -32769,
             2**23 - 1, -(2**23 - 1), 2**23, -2**23, -2**23 - 1,
             2**31 - 1, -(2**31 - 1), 2**31, -2**31, -2**31 - 1,
             2**52 - 1, 2**52, -2**52, 2**53, 10**16, 99999999999999984)
STRING_SCORES = (1e17, 2.0**63)                            # "1e+17" and "9.2233720368547758e+18": no string2ll
INT_GROUPS = (INT_EDGES[:8], INT_EDGES[8:19], INT_EDGES[19:24], INT_EDGES[24:] + STRING_SCORES, INT_EDGES + STRING_SCORES,
              tuple(v for v in INT_EDGES if v < 0))
# (members, {rank: the integer-valued score there}): the rank in front of each is fractional
LAST_SLOT = ((64, {63: 7}), (64, {63: 42}), (64, {63: 99999999999999984}),
             (128, {63: 7, 127: 42}), (128, {63: 42, 127: 10**16}), (128, {63: 5, 127: 99999999999999984}))
assert len(INT_GROUPS) % 2 == 0                            # so that the pairs behind them start at an even index


def int_encoding(v):
    """zipTryEncoding's byte for an integer entry (ziplist.c:487-500)."""
    if 0 <= v <= 12:
        return 0xF1 + v
    for enc, bits in ((0xFE, 8), (0xC0, 16), (0xF0, 24), (0xD0, 32), (0xE0, 64)):
        if -(1 << (bits - 1)) <= v < 1 << (bits - 1):
            return enc


def _last_slot_zset(n, ints, seed):
    scores, lo = [], -40.0
    for r in range(n):
        if r in ints:
            lo = float(ints[r])
            scores.append(lo)
        else:
            scores.append(lo + (r % 64) * 0.5 + 0.25 if r > 63 else -40.0 + r * 0.5 + 0.25)
    assert scores == sorted(scores) and len(set(scores)) == n and all(s % 1 for r, s in enumerate(scores) if r not in ints)
    perm = np.random.default_rng(seed).permutation(n)
    return zset([(b"r%03d" % r, scores[r]) for r in perm])


def int_text_zsets():
    """Every ZSet holds a fractional score, so rr_rdbconvert_batch leaves each one RR_RDBLOAD_E_CONVERT
    and the whole list is attempted by the third stage: the compacted index of a value is its index in
    the list, and value k runs on wave k % 2 of a workgroup.
    Values 0 .. len(INT_GROUPS) - 1 hold the integer-valued scores of INT_GROUPS, the edges of the
    ziplist's integer encodings, which are printed and then found again by string2ll; 1e17 and 2^63
    print with an exponent and stay strings.  Then every LAST_SLOT ZSet twice in a row, on an even
    index and the odd one behind it, so on wave 0 and on wave 1: 64 or 128 members, rank 63 (and 127),
    the last text slot of a round, an integer-valued score of 1, 2 or 17 digits, and the rank in front
    of it fractional.  str_is_ll's 64-byte look from slot 63 runs into the next wave's sort arrays
    (wave 0) or the pad behind the last wave (wave 1)."""
    out = []
    for g, group in enumerate(INT_GROUPS):
        items = [(b"i%02d" % k, float(v)) for k, v in enumerate(group)]
        items.insert((0, len(items) // 2, len(items))[g % 3], (b"frac", 0.5 - g))
        out.append((zset(items[::-1] if g % 2 else items), INT_OPTS))
    for k, (n, ints) in enumerate(LAST_SLOT):
        out += [(_last_slot_zset(n, ints, 60 + k), INT_OPTS), (_last_slot_zset(n, ints, 80 + k), INT_OPTS)]
    return out


# ---- 6. a wave's LDS taken over by its next value -----------------------------------------------------------------
REUSE_PAIRS = 7
REUSE_STAYS = 3                                            # the big value that stays RR_RDBLOAD_E_CONVERT
REUSE_OPTS = ld.options(zset_max_ziplist_entries=512, zset_max_ziplist_value=300)


def _reuse_big():
    rng = np.random.default_rng(91)
    edge = zr.edge_scores()
    edge = edge[(edge & np.uint64(0x7FFFFFFFFFFFFFFF)) <= np.uint64(0x7FF0000000000000)]   # no NaN
    pick = lambda: zr.to_double(int(edge[int(rng.integers(0, len(edge)))]))
    sub = _take(512, 24, lambda j: -5e-324 * (3**30 + 7**14 * j))
    subs = [(b"s%03d" % k, sub[int(j)]) for k, j in enumerate(rng.permutation(512))]
    tied = [(b"t%04d" % int(k), 0.1) for k in rng.permutation(511)]
    long_members = [(bytes([97 + k % 26]) * 299 + bytes([48 + k // 26]), k / 8 + 0.0625 - 5) for k in range(100)]
    late = [(b"n%03d" % k, k + 0.5) for k in range(511)] + [(b"nan", float("nan"))]
    tiny = [(b"y%03d" % k, (-1) ** k * (5e-324 * (5**21 + 3**27 * k) if k % 3 else 2.5e-304 * (1 + k / 512))) for k in range(512)]
    wide = [(b"w%03d" % k, (-1) ** k * 2.0**1012 * (1 + (511 - k) / 512)) for k in range(512)]
    mixed = [(b"e%d" % k, pick()) for k in range(130)]
    return [zset(subs),              # 512 members, 34 words of state each, 24-byte texts
            zset(tied),              # 511 members, one score: the member bytes order
            zset(long_members),      # 300-byte members: a 5-byte prevlen on every score
            zset(late),              # stays: a NaN in the last pair, the slab half used
            zset(tiny),              # fractions of both signs that leave most of their 34 words non-zero
            zset(wide),              # m << 960 of both signs, 32 words, falling (see round_two_table)
            zset(mixed)]


def _reuse_small():
    return [zset([(b"a", 1.5)]),
            b"\x00",
            zset([(b"c", 0.25), (b"b", 0.25), (b"a", 0.25)]),
            zset([(b"q", 0.5), (b"p", 7.0)]),
            zset([(b"u", 2.0**1012 * 1.3), (b"d", -2.0**1012 * 1.7)]),           # over the fractions' remains
            zset([(b"z", -5e-324 * 3**20), (b"s", 5e-324), (b"t", 2.2250738585072014e-308)]),   # remains for m << 960
            zset([(b"i", float("inf")), (b"t", 0.1)])]


def _reuse_filler(k):
    """Value k of the rest: 2 or 3 members, fractional scores from k."""
    n = 2 + k % 3 % 2
    return zset([(b"%x" % (k * 40503 >> (3 * j) & 0xFFF), ((k >> j) % 97 - 48) / 8 + 0.0625) for j in range(n)])


def wave_reuse_batch(swap=False):
    """RR_RDBCONVERT_MAX_WAVES + 7 ZSets, all to be claimed RR_RDBLOAD_E_CONVERT: value k and value
    k + MAX_WAVES run on one wave of rdbzset_size_kernel and of rdbzset_emit_kernel.  The first seven are
    big, their partners a stride later tiny (swap: the other way round), everything between two or
    three members."""
    big, small = _reuse_big(), _reuse_small()
    first, second = (small, big) if swap else (big, small)
    vals = first + [_reuse_filler(k) for k in range(REUSE_PAIRS, cv.MAX_WAVES)] + second
    return [(p, REUSE_OPTS) for p in vals]
