"""Payload generators for rr_rdbconvert_batch's sort: the order among negative scores, signed Set order
and the width from the extremes, duplicates across the 64-lane steps of the dedup loop, integer-form
member text past its eighth byte, a wave's LDS slab taken over by its next value, a Hash at the
option's ceiling and a 5-byte prevlen inside a ZSet.  Plain Python, no GPU code: every generator
returns a list of (type, payload, opts), one opts object for the whole list, so that a list is one
batch.  tests/test_rdbconvert_shapes.py holds the generators to what they claim and the reference to a
second statement on them; tests/test_gpu_rdbconvert_sort.py holds the kernels to the reference.

The score -(2**52 - 1) cannot be in a value that converts: it is d2string's `min` itself
(util.c:542-544, value > min), prints with %.17g and so stays RR_RDBLOAD_E_CONVERT
(include/rr_rdbconvert.h).  The converting ZSets reach down to -(2**52 - 2), the lowest finite score
the rule takes, and neg_score_zsets() ends with ZSets that hold -(2**52 - 1) and must stay
RR_RDBLOAD_E_CONVERT (NEG_STAYS of them)."""
import struct

import numpy as np

import rdb_reference as ref
import rdbconvert_reference as cv
import rdbload_reference as ld
from rdbload_mutants import lz
from test_rdbconvert import HASH, SET, ZSET, dbl, raw

INF = float("inf")
BIG = 2**52 - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
num = lambda v: raw(str(v).encode())                  # an integer as its text
i32 = lambda v: b"\xC2" + struct.pack("<i", v)        # RDB_ENC_INT32, whatever the value's size


def zset(items):
    """items: (member as it stands in the payload, score)."""
    return ref.save_len(len(items)) + b"".join(m + dbl(s) for m, s in items)


def _orders(n, seed):
    perm = np.random.default_rng(seed).permutation(n).tolist()
    return list(range(n)), list(range(n - 1, -1, -1)), perm


# ---- 1. the order among negative scores ------------------------------------------------------------------
NEG_POOL = (-INF, -float(BIG - 1), -2.0, -1.0, -0.0, 0.0, 1.0, float(BIG), INF)
NEG_SMALL = {2: (-2.0, -1.0), 3: (-float(BIG - 1), -2.0, -1.0)}
NEG_STAYS = 2                                         # the last values: a score of -(2**52 - 1)


def neg_score_zsets():
    """ZSets of 2, 3, 64, 65 and 130 distinct members over NEG_POOL, each with at least two different
    negative finite scores, the payload in the converted order, in its reverse and permuted.  The
    members run against the scores, so among the scores that are zero a -0 stands before and behind a
    0 in the payload and on the other side of it in the blob."""
    o = ld.options(zset_max_ziplist_entries=512)
    out = []
    for n in (2, 3, 64, 65, 130):
        scores = NEG_SMALL.get(n) or [NEG_POOL[k % len(NEG_POOL)] for k in range(n)]
        items = [(b"m%03d" % (k * 37 % 1000), scores[k]) for k in range(n)]
        target = sorted(items, key=lambda x: (x[1], x[0]))
        for order in _orders(n, 11 + n):
            out.append((ZSET, zset([(raw(target[k][0]), target[k][1]) for k in order]), o))
    out.append((ZSET, zset([(raw(b"z"), -0.0), (raw(b"k"), -2.0), (raw(b"a"), 0.0), (raw(b"j"), -1.0)]), o))
    assert NEG_STAYS == 2
    out.append((ZSET, zset([(raw(b"a"), -2.0), (raw(b"b"), -float(BIG)), (raw(b"c"), -1.0)]), o))
    out.append((ZSET, zset([(raw(b"%d" % k), -float(BIG) if k == 64 else -float(k + 1)) for k in range(66)]), o))
    return out


# ---- 2. signed order and the width of Sets at the extremes --------------------------------------------------
EXTREMES = (I64_MIN, I64_MIN + 1, -2**31 - 1, -2**31, -32769, -32768, -1, 0, 1, 32767, 32768, 2**31 - 1, 2**31, I64_MAX)
# (width, the members that decide it or stand at its edge): by the low extreme alone, by the high one
# alone, by both, and by neither (all members inside int16 / int32, at the very edges too)
EXTREME_SPECS = ((8, (I64_MIN,)), (8, (I64_MIN + 1,)), (8, (-2**31 - 1,)), (8, (I64_MAX,)), (8, (2**31,)), (8, (I64_MIN, I64_MAX)),
                 (4, (-2**31,)), (4, (-32769,)), (4, (2**31 - 1,)), (4, (32768,)), (4, (-2**31, 2**31 - 1)), (4, (-32769, 32768)),
                 (2, (-32768,)), (2, (32767,)), (2, (-1, 0, 1)), (2, (-32768, 32767)))
LZF_MEMBER = 1111111111111111111                      # 19 digits, compressible; inside int64


def extreme_set_values(width, force, n, place, with_lzf):
    """The n members in payload order: `force` at the front, in the middle or at the end of small
    distinct integers of both signs in a fixed shuffle."""
    force = list(force[:n])
    pads = [v for v in range(-255, 257) if v not in force]
    pads = [pads[k] for k in np.random.default_rng(100 * n + width).permutation(len(pads))][:n - len(force)]
    if with_lzf and pads:
        pads[0] = LZF_MEMBER
    at = {"first": 0, "middle": len(pads) // 2, "last": len(pads)}[place]
    return pads[:at] + force + pads[at:]


def extreme_sets():
    """Sets of 2, 4, 65 and 512 members for every EXTREME_SPECS row and each place of its deciding
    members.  Members inside int32 alternate between the RDB_ENC_INT8/16/32 forms and their text; one
    member of the (INT64_MIN, INT64_MAX) Sets is an LZF string."""
    out = []
    for width, force in EXTREME_SPECS:
        for n in (2, 4, 65, 512):
            for pi, place in enumerate(("first", "middle", "last")):
                with_lzf = force == (I64_MIN, I64_MAX) and place == "middle"
                vals = extreme_set_values(width, force, n, place, with_lzf)
                body = b""
                for k, v in enumerate(vals):
                    if v == LZF_MEMBER:
                        body += lz(str(v).encode())
                    elif (k + pi) % 2 == 0:
                        body += ref.save_raw_string(str(v).encode())      # an integer form where there is one
                    else:
                        body += num(v)
                out.append((SET, ref.save_len(n) + body, None))
    return out


# ---- 3. duplicates that are neither none nor all -----------------------------------------------------------
def _seam_target(n, dup):
    """Sorted positions 0 .. n-1 -> the rank of the distinct value there; dup(p): position p repeats p - 1."""
    idx, out = -1, []
    for p in range(n):
        idx += 0 if p and dup(p) else 1
        out.append(idx)
    return out


SEAM_VARIANTS = (("pair 63|64", (65, 129, 130, 512), lambda p: p == 64),
                 ("pair 127|128", (129, 130, 512), lambda p: p == 128),
                 ("pairs 63|64 and 127|128", (130, 512), lambda p: p in (64, 128)),
                 ("every value twice", (130, 512), lambda p: p % 2 == 1),
                 ("one value from 63 on", (65, 129, 130, 512), lambda p: p > 63),
                 ("70 equal from 30", (129, 130, 512), lambda p: 30 < p < 100))
SEAM_SCALE = {2: 3, 8: (1 << 40) + 1}                 # rank -> value: (rank - half the ranks) * scale, both signs


def seam_duplicate_sets(with_targets=False):
    """Sets whose sorted order holds equal neighbours at known places (SEAM_VARIANTS), in widths 2 and 8,
    the payload a fixed permutation of the sorted target.  with_targets: (name, width, target) beside
    each value, for the test of the claims."""
    out, targets = [], []
    for vi, (name, ns, dup) in enumerate(SEAM_VARIANTS):
        for n in ns:
            ranks = _seam_target(n, dup)
            for width in (2, 8):
                target = [(r - ranks[-1] // 2) * SEAM_SCALE[width] for r in ranks]
                perm = np.random.default_rng(1000 * vi + n + width).permutation(n)
                out.append((SET, ref.save_len(n) + b"".join(num(target[k]) for k in perm), None))
                targets.append((name, width, target))
    return (out, targets) if with_targets else out


# ---- 4. integer-form member text past 8 bytes ------------------------------------------------------------------
LONG_INTS = (100000000, 123456789, 123456780, 2147483647, -100000000, -2147483648, -2147483647)
LONG_RAW = (b"12345678:", b"12345678/", b"123456788",                      # differ from an integer's text at byte 8
            b"214748364:", b"2147483640", b"-10000000/", b"-100000001",    # at byte 9
            b"-214748364/", b"-214748364:", b"-2147483649",                # at byte 10
            b"12345678", b"10000000", b"214748364", b"-214748364", b"-21474836",   # strict prefixes
            b"1234567890", b"2147483647x", b"-21474836480", b"100000000\x00",      # extensions
            b"123456780")                                                  # an integer member's text itself


def long_int_members():
    """ZSets whose scores all tie, so that sdscmp of the members alone orders them: RDB_ENC_INT32
    members of 9, 10 and 11 bytes of text among raw members that part from such a text at byte 8, 9
    or 10, stop short of it, go on beyond it, or are it."""
    ints = [(i32(v), 1.0) for v in LONG_INTS]
    raws = [(raw(m), 1.0) for m in LONG_RAW]
    out = []
    for seed in (1, 2):                               # 18 and 17 members, shuffled
        items = ints + raws[seed - 1::2] + raws[-1:] * (seed == 1)
        out.append((ZSET, zset([items[k] for k in np.random.default_rng(seed).permutation(len(items))]), None))
    out.append((ZSET, zset((raws[:10] + ints)[::-1]), None))                # 17: the integers first, descending
    neg = [x for x, m in zip(ints, LONG_INTS) if m < 0] + [x for x, m in zip(raws, LONG_RAW) if m[:1] == b"-"]
    out.append((ZSET, zset(neg + [(raw(b"-"), 1.0)]), None))               # 12: everything behind a '-'
    fill = [(raw(b"%d" % (123456700 + k)), 1.0) for k in range(43)]        # 70: six integer forms, at 64 and beyond
    out.append((ZSET, zset(raws + fill + [(raw(b"-2147483640"), 1.0)] + ints[:0:-1]), None))
    return out


# ---- 5. a wave's LDS taken over by its next value -----------------------------------------------------------
REUSE_PAIRS = 7
REUSE_HASH_PARTNER = 6                                # the one Hash: behind a big ZSet
REUSE_STAYS = 4                                       # the partner that stays RR_RDBLOAD_E_CONVERT


def _reuse_big():
    rng = np.random.default_rng(77)
    wide = [int(v) for v in rng.integers(-(1 << 62), 1 << 62, 512)]
    tied = [b"t%04d" % k for k in range(3)] + [b"t%04d" % (3 + int(k)) for k in rng.permutation(509)]
    with_ints = [(i32(1000000000 + 7 * k) if k % 2 else raw(b"10000000%02d" % (k % 100)), float(k % 3 - 1)) for k in range(130)]
    dups = [int(v) for v in rng.integers(-300, 300, 512)]
    falling = [(raw(b"f%d" % k), float(256 - k)) for k in range(512)]
    mid = [int(v) for v in rng.integers(-(1 << 31), 1 << 31, 512)]
    short = [(raw(b"%d" % (k * 7919 % 1000)), float(k % 5)) for k in range(130)]
    return [(SET, ref.save_len(512) + b"".join(num(v) for v in wide)),                     # enc 8
            (ZSET, zset([(raw(m), 7.0) for m in tied])),                                  # every score ties; ranks 0, 1, 2 first
            (ZSET, zset(with_ints)),                                                       # integer-form members
            (SET, ref.save_len(512) + b"".join(num(v) for v in dups)),                     # enc 2, duplicates
            (ZSET, zset(falling)),                                                         # descending, negative scores
            (SET, ref.save_len(512) + b"".join(ref.save_raw_string(str(v).encode()) for v in mid)),   # enc 4
            (ZSET, zset(short))]                                                           # members the window takes


def _reuse_small():
    return [(SET, b"\x02" + num(9) + num(-9)),
            (ZSET, zset([(raw(b"c"), 7.0), (raw(b"b"), 7.0), (raw(b"a"), 7.0)])),          # correct order: indices 2, 1, 0
            (SET, b"\x00"),
            (ZSET, b"\x00"),
            (SET, b"\x03" + num(5) + raw(b"x") + num(7)),                                  # stays: member 1 is no integer
            (ZSET, zset([(raw(b"q"), 2.0), (raw(b"p"), -2.0)])),
            (HASH, b"\x02" + raw(b"f") + raw(b"12") + raw(b"g") + lz(b"ab" * 20))]


def _reuse_filler(k):
    """Value k of the rest: 2 or 3 members, Set and ZSet in turn, from k."""
    n = 2 + k % 3 % 2
    if k % 2:
        return SET, ref.save_len(n) + b"".join(num((k * 2654435761 >> (5 * j)) % 200001 - 100000) for j in range(n))
    return ZSET, zset([(raw(b"%x" % (k * 40503 >> (3 * j) & 0xFFF)), float((k >> j) % 7 - 3)) for j in range(n)])


def lds_reuse_batch(swap=False):
    """RR_RDBCONVERT_MAX_WAVES + 7 values, all to be claimed RR_RDBLOAD_E_CONVERT: value k and value
    k + MAX_WAVES run on one wave.  The first seven are big Sets and ZSets, their partners a stride
    later tiny (swap: the other way round), everything between two or three members."""
    o = ld.options(zset_max_ziplist_entries=512)
    big, small = _reuse_big(), _reuse_small()
    first, second = (small, big) if swap else (big, small)
    vals = first + [_reuse_filler(k) for k in range(REUSE_PAIRS, cv.MAX_WAVES)] + second
    return [(t, p, o) for t, p in vals]


# ---- 6. a Hash at the option's ceiling --------------------------------------------------------------------------
def _hash_pairs(n):
    return ref.save_len(n) + b"".join(raw(bytes([65 + k % 26, 97 + k // 26 % 26])) + raw(b"%d" % (k % 10) if k % 3 else b"v")
                                      for k in range(n))


def hash_at_entry_cap():
    """hash_max_ziplist_entries at its cap: Hashes of 32767 pairs (zllen 65534, one below the value at
    which ziplist.c stops counting), of 32766, and of 32768, which stays RR_RDBLOAD_E_CONVERT."""
    o = ld.options(hash_max_ziplist_entries=32767)
    return [(HASH, _hash_pairs(n), o) for n in (32767, 32766, 32768)]


# ---- 7. a 5-byte prevlen inside a ZSet ---------------------------------------------------------------------------
def member_of_entry(total, fill=b"q"):
    """The member whose ziplist entry behind a short one is `total` bytes whole."""
    m = fill * (total - 1 - (1 if total - 2 < 64 else 2 if total - 3 < 16384 else 5))
    assert len(ref.zip_entry(0, m)) == total
    return m


def zset_wide_prevlen():
    """zset_max_ziplist_value 400: member entries of 253, 254 and 255 bytes in front of an integer
    score, of "inf" and of "-0", in every assignment, so that the 5-byte prevlen lands on an integer
    entry and on a string entry, and on the last entry of the ziplist."""
    o = ld.options(zset_max_ziplist_value=400)
    scores = (-0.0, 5.0, INF)
    out = []
    for k, sizes in enumerate(((253, 254, 255), (253, 255, 254), (254, 253, 255), (254, 255, 253), (255, 253, 254), (255, 254, 253))):
        items = [(raw(member_of_entry(t, bytes([97 + j]))), s) for j, (t, s) in enumerate(zip(sizes, scores))]
        out.append((ZSET, zset(items[k % 3:] + items[:k % 3]), o))
    tied = [(raw(member_of_entry(t)), -300.0) for t in (255, 253, 254)]    # equal to the shorter one's end; an int16 score
    out.append((ZSET, zset(tied), o))
    return out
