"""CPU tests of tests/rdbconvert_shapes.py: every generated value converts under the reference
(tests/rdbconvert_reference.py) unless the generator names it as staying RR_RDBLOAD_E_CONVERT; the
reference's blobs agree with a second statement of the result (sorted / set for an intset, sorted by
(float, member bytes) for a ZSet); and each generator still holds the edge it was written for.  The
GPU side is tests/test_gpu_rdbconvert_sort.py."""
import functools
import itertools
import math
import struct

import lzf_reference as lzf
import rdb_reference as ref
import rdbconvert_reference as cv
import rdbconvert_shapes as sh
import rdbload_reference as ld
from test_rdbconvert import HASH, HZL, ISET, SET, ZSET, ZZL

flt = lambda bits: struct.unpack("<d", struct.pack("<Q", bits))[0]


@functools.lru_cache(maxsize=None)
def converted(name):
    """(values, [convert_blob's result for each]) of a generator, computed once."""
    vals = getattr(sh, name)()
    assert len({id(o) for _, _, o in vals}) == 1                          # one batch, one set of options
    return vals, [cv.convert_blob(t, p, o) for t, p, o in vals]


def set_values(p):
    return [int(m) for m in ref.load(SET, lzf.expand(SET, p)[0])[1]]


def zset_items(p):
    """(python float, member bytes, is the member in an integer form) in payload order, by a walk of its own."""
    r = ld.Rd(p)
    out = []
    for _ in range(r.count()):
        intform = p[r.p] in (0xC0, 0xC1, 0xC2)
        m = r.string()
        out.append((flt(struct.unpack("<Q", r.take(8))[0]), m, intform))
    assert r.p == len(p)
    return out


def check_intset(p, res):
    """enc, len, sorted(set(values)) at the width of the extremes."""
    st, nt, blob, pay, nel = res
    vals = set_values(p)
    lo, hi = (min(vals), max(vals)) if vals else (0, 0)
    w = 8 if lo < -2**31 or hi > 2**31 - 1 else 4 if lo < -2**15 or hi > 2**15 - 1 else 2
    uniq = sorted(set(vals))
    assert (st, nt) == (0, ISET)
    assert blob[5:] == struct.pack("<II", w, len(uniq)) + b"".join(v.to_bytes(w, "little", signed=True) for v in uniq)
    assert (pay, nel) == (len(blob) - 5, len(vals))
    return w, uniq


def check_zset(p, res):
    """The ziplist's entries are sorted(items, key=(python float, member bytes)), scores as d2string prints them."""
    st, nt, blob, pay, nel = res
    items = zset_items(p)
    assert (st, nt) == (0, ZZL) and struct.unpack_from("<Q", blob, 5)[0] == len(blob) - 13
    ents = ref.walk_ziplist(blob[13:])
    want = sorted(items, key=lambda x: (x[0], x[1]))
    assert ents[0::2] == [m for _, m, _ in want]
    for text, (s, _, _) in zip(ents[1::2], want):
        assert float(text) == s and (text[:1] == b"-") == (math.copysign(1.0, s) < 0), (text, s)
        assert text in (b"inf", b"-inf", b"-0") or text == b"%d" % int(s)
    return items, want


def test_neg_score_zsets():
    vals, res = converted("neg_score_zsets")
    assert len(vals) == 5 * 3 + 1 + sh.NEG_STAYS
    sizes, crossed = set(), False
    for (t, p, o), r in zip(vals[:-sh.NEG_STAYS], res):
        assert t == ZSET and ld.load_blob(t, p, o)[0] == ld.E_CONVERT
        items, want = check_zset(p, r)
        sizes.add(len(items))
        assert len({s for s, _, _ in items if s < 0 and math.isfinite(s)}) >= 2
        assert len({m for _, m, _ in items}) == len(items) and all(len(m) < 64 for _, m, _ in items)
        zeros = [(math.copysign(1.0, s), m) for s, m, _ in items if s == 0]
        for (sa, ma), (sb, mb) in itertools.combinations(zeros, 2):      # a before b in the payload
            crossed |= sa != sb and mb < ma                               # ... and b before a in the blob
    assert sizes >= {2, 3, 64, 65, 130} and crossed
    seen = {repr(s) for _, p, _ in vals[:-sh.NEG_STAYS] for s, _, _ in zset_items(p)}   # repr: -0.0 is not 0.0
    assert seen == {repr(s) for s in sh.NEG_POOL}
    for k in (0, 3, 6, 9, 12):                                            # the three payload orders of a size
        a, b, c = (zset_items(vals[k + j][1]) for j in range(3))
        assert a == sorted(a) and b == a[::-1] and sorted(c) == a and (len(a) < 4 or c not in (a, b))
    for (t, p, o), r in zip(vals[-sh.NEG_STAYS:], res[-sh.NEG_STAYS:]):   # d2string's min itself: %.17g, left to the CPU path
        assert -float(2**52 - 1) in [s for s, _, _ in zset_items(p)]
        assert ld.load_blob(t, p, o)[0] == ld.E_CONVERT and r[0] == cv.E_CONVERT


def test_extreme_sets():
    vals, res = converted("extreme_sets")
    assert len(vals) == len(sh.EXTREME_SPECS) * 4 * 3
    seen, lzf_members, it = set(), 0, iter(zip(vals, res))
    for width, force in sh.EXTREME_SPECS:
        for n in (2, 4, 65, 512):
            for place in ("first", "middle", "last"):
                (t, p, o), r = next(it)
                assert t == SET and o is None and ld.load_blob(t, p, o)[0] == ld.E_CONVERT
                w, uniq = check_intset(p, r)
                got = set_values(p)
                assert w == width and len(got) == n == len(uniq)
                f = [v for v in force[:n]]
                rest = [v for v in got if v not in f]
                assert all(-256 < v < 257 or v == sh.LZF_MEMBER for v in rest)
                at = got.index(f[0])
                assert got[at:at + len(f)] == f and at == {"first": 0, "middle": len(rest) // 2, "last": len(rest)}[place]
                lo_forces = uniq[0] < (-2**31 if w == 8 else -2**15)
                hi_forces = uniq[-1] > (2**31 - 1 if w == 8 else 2**15 - 1)
                seen.add((w, lo_forces and w > 2, hi_forces and w > 2))
                seen |= {v for v in got if v in sh.EXTREMES}
                lzf_members += sh.LZF_MEMBER in got
    assert seen >= {(w, a, b) for w in (4, 8) for a, b in ((True, False), (False, True), (True, True))} | {(2, False, False)}
    assert seen >= set(sh.EXTREMES)
    assert lzf_members == 3 and b"\xC3" in b"".join(p for _, p, _ in vals)
    firsts = {p[1] for _, p, _ in vals if p[0] == 2}                      # the first member of the 2-member Sets
    assert firsts >= {0xC0, 0xC1, 0xC2}
    # inside int16 and inside int32 at the very edges: no wider than that
    edge = {tuple(f): w for w, f in sh.EXTREME_SPECS}
    assert edge[(-32768, 32767)] == 2 and edge[(-2**31, 2**31 - 1)] == 4


def test_seam_duplicate_sets():
    (vals, targets), res = sh.seam_duplicate_sets(True), converted("seam_duplicate_sets")[1]
    assert [v[:2] for v in vals] == [v[:2] for v in converted("seam_duplicate_sets")[0]]
    names = set()
    for (t, p, o), (name, width, target), r in zip(vals, targets, res):
        assert ld.load_blob(t, p, o)[0] == ld.E_CONVERT
        w, uniq = check_intset(p, r)
        got = set_values(p)
        n = len(got)
        assert w == width and sorted(got) == target and got != target and got != target[::-1]
        assert uniq[0] < 0 < uniq[-1]
        eq = [k for k in range(1, n) if target[k] == target[k - 1]]      # sorted positions that repeat their neighbour
        if name == "pair 63|64":
            assert eq == [64]
        elif name == "pair 127|128":
            assert eq == [128]
        elif name == "pairs 63|64 and 127|128":
            assert eq == [64, 128]
        elif name == "every value twice":
            assert eq == list(range(1, n, 2)) and len(uniq) == n // 2
        elif name == "one value from 63 on":
            assert eq == list(range(64, n)) and len(uniq) == 64
        else:
            assert name == "70 equal from 30" and eq == list(range(31, 100)) and len(uniq) == n - 69
        names.add((name, n, w))
    assert len(names) == len(vals) == 36
    assert {("every value twice", 512, w) for w in (2, 8)} <= names
    for name in ("pair 63|64", "one value from 63 on"):
        assert {n for m, n, _ in names if m == name} == {65, 129, 130, 512}


def test_long_int_members():
    vals, res = converted("long_int_members")
    lens, first_diff, dup, prefix, extend, late = set(), set(), False, False, False, False
    for (t, p, o), r in zip(vals, res):
        assert t == ZSET and o is None and ld.load_blob(t, p, o)[0] == ld.E_CONVERT
        items, want = check_zset(p, r)
        assert len({s for s, _, _ in items}) == 1 and (10 <= len(items) <= 20 or len(items) == 70)
        ints = [m for _, m, f in items if f]
        assert ints
        lens |= {len(m) for m in ints}
        for a in ints:
            for _, b, f in items:
                if f and b == a:
                    continue
                m = min(len(a), len(b))
                d = next((k for k in range(m) if a[k] != b[k]), None)
                if d is not None:
                    first_diff.add(d)
                elif len(a) == len(b):
                    dup = True                                            # a raw member that is the integer's text
                elif len(b) < len(a):
                    prefix = True
                else:
                    extend = True
        if len(items) == 70:
            late = all(k >= 64 for k, (_, _, f) in enumerate(items) if f) and len(ints) >= 6
    assert lens == {9, 10, 11} and first_diff >= {8, 9, 10} and dup and prefix and extend and late
    want_ints = {str(v).encode() for v in sh.LONG_INTS}
    assert {m for _, p, _ in vals for _, m, f in zset_items(p) if f} == want_ints


def test_lds_reuse_batch():
    for swap in (False, True):
        vals = sh.lds_reuse_batch(swap)
        n = len(vals)
        assert n == cv.MAX_WAVES + sh.REUSE_PAIRS > cv.MAX_WAVES and len({id(o) for _, _, o in vals}) == 1
        res = [cv.convert_blob(t, p, o) for t, p, o in vals]
        big, small = (vals[-7:], vals[:7]) if swap else (vals[:7], vals[-7:])
        rbig, rsmall = (res[-7:], res[:7]) if swap else (res[:7], res[-7:])
        assert [t for t, _, _ in big].count(HASH) == 0
        assert [k for k, (t, _, _) in enumerate(small) if t == HASH] == [sh.REUSE_HASH_PARTNER]
        assert big[sh.REUSE_HASH_PARTNER][0] == ZSET and rsmall[sh.REUSE_HASH_PARTNER][1] == HZL
        assert [t for t, _, _ in vals[7:-7]].count(HASH) == 0
        assert [r[0] for r in res] == [cv.E_CONVERT if k == (sh.REUSE_STAYS if swap else n - 7 + sh.REUSE_STAYS) else 0
                                       for k in range(n)]
        for (t, p, o), r in zip(vals, res):
            if r[0] == 0 and t == SET:
                check_intset(p, r)
            elif r[0] == 0 and t == ZSET:
                check_zset(p, r)
        # the big values: 512-member Set of width 8, a 512-member ZSet of one score, 130 members with integer forms
        assert (len(set_values(big[0][1])), rbig[0][2][5]) == (512, 8)
        tied = zset_items(big[1][1])
        assert len(tied) == 512 and len({s for s, _, _ in tied}) == 1
        withint = zset_items(big[2][1])
        assert len(withint) == 130 and sum(f for _, _, f in withint) >= 60
        assert all(len(p) > 1000 for _, p, _ in big)
        # the partners: 2-member Set; 3 members in the reverse of the big value's first ranks; two empty ones; the one
        # that stays, with its non-integer member at index 1; a 2-member ZSet
        assert len(set_values(small[0][1])) == 2
        order = lambda items: [items.index(x) for x in sorted(items, key=lambda x: (x[0], x[1]))]
        assert order(zset_items(small[1][1])) == [2, 1, 0] and order(tied)[:3] == [0, 1, 2]
        assert (small[2][:2], small[3][:2]) == ((SET, b"\x00"), (ZSET, b"\x00"))
        stay = ref.load(SET, small[sh.REUSE_STAYS][1])[1]
        assert ref.canonical_int(stay[0]) is not None and ref.canonical_int(stay[1]) is None
        assert small[sh.REUSE_STAYS + 1][0] == ZSET and len(zset_items(small[sh.REUSE_STAYS + 1][1])) == 2
        mid = vals[7:-7]
        assert {t for t, _, _ in mid[0::2]} | {t for t, _, _ in mid[1::2]} == {SET, ZSET}
        assert all(a[0] != b[0] for a, b in zip(mid, mid[1:]))                       # Set and ZSet in turn
        assert {p[0] for _, p, _ in mid} == {2, 3} and sum(len(p) for _, p, _ in mid) < 1 << 20


def test_hash_at_entry_cap():
    vals, res = converted("hash_at_entry_cap")
    assert vals[0][2]["hash_max_ziplist_entries"] == 32767
    pairs = []
    for (t, p, o), r in zip(vals, res):
        assert t == HASH
        strs = ref.load(HASH, p)[1]
        assert {len(s) for s in strs} == {1, 2}
        pairs.append(len(strs) // 2)
        if len(strs) // 2 <= 32767:
            assert ld.load_blob(t, p, o)[0] == ld.E_CONVERT and (r[0], r[1]) == (0, HZL)
            z = r[2][13:]
            assert struct.unpack_from("<H", z, 8)[0] == len(strs) and ref.walk_ziplist(z) == strs
        else:
            assert ld.load_blob(t, p, o)[0] == 0 and r[0] == cv.E_CONVERT            # a hash table; claimed, it stays
    assert pairs == [32767, 32766, 32768]
    assert struct.unpack_from("<H", res[0][2], 13 + 8)[0] == 65534


def test_zset_wide_prevlen():
    vals, res = converted("zset_wide_prevlen")
    assert vals[0][2]["zset_max_ziplist_value"] == 400
    wide_on, last_wide = set(), 0
    for (t, p, o), r in zip(vals, res):
        assert t == ZSET and ld.load_blob(t, p, o)[0] == ld.E_CONVERT
        assert ld.load_blob(t, p, None)[0] == 0                           # under the default the members are too long
        items, want = check_zset(p, r)
        z = r[2][13:]
        ents = ref.walk_ziplist(z)
        at, prev = 10, 0
        for k, e in enumerate(ents):                                      # the entries again, for their sizes
            entry = ref.zip_entry(prev, e)
            assert z[at:at + len(entry)] == entry
            if k % 2 == 0:
                assert len(ref.zip_entry(0, e)) in (253, 254, 255)
            elif prev >= 254:
                assert z[at] == 0xFE
                wide_on.add("int" if z[at + 5] >= 0xC0 else e)
                last_wide += k == len(ents) - 1
            at, prev = at + len(entry), len(entry)
        assert z[at] == 0xFF
    assert wide_on == {"int", b"inf", b"-0"} and last_wide >= 2
    sizes = {(len(ref.zip_entry(0, m)), s) for _, p, _ in vals[:6] for s, m, _ in zset_items(p)}
    assert len(sizes) == 9
