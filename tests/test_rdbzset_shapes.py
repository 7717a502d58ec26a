"""CPU tests of tests/rdbzset_shapes.py: the yardstick (Python's '%.17g') is held to the C library's
snprintf and the host's rr_d2string to the yardstick on every score list the GPU tests use, and each
generator still holds the edge it was written for: every exponent, the notations and ll2string's window,
a second round past rr_launch_d2string's grid cap (read from the source), the lanes' sequences of word
counts, every ziplist integer encoding as a printed score, and two values a wave.  The GPU side is
tests/test_gpu_rdbzset_shapes.py."""
import functools
import os
import re
import struct

import numpy as np

import rdb_reference as ref
import rdbconvert_reference as cv
import rdbload_reference as ld
import rdbzset_reference as zr
import rdbzset_shapes as sh
from test_d2string import check
from test_rdbzset import ZSET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def texts_of(bits):
    return [zr.d2string(b) for b in bits.tolist()]


# ---- the yardstick and the host twin on the new score lists ---------------------------------------------------
def test_yardstick_and_host_twin_on_stratified_bits():
    assert check(sh.stratified_bits()) == zr.D2STRING_MAX


def test_yardstick_and_host_twin_on_window_bits():
    assert 17 <= check(sh.window_bits()) <= zr.D2STRING_MAX


def test_yardstick_and_host_twin_on_the_round_two_table():
    assert check(sh.round_two_table()) == zr.D2STRING_MAX


# ---- the generators' claims -------------------------------------------------------------------------------------
def test_stratified_bits():
    per = 64
    b = sh.stratified_bits(per)
    exp = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    assert len(b) == 2047 * (per + 2) > 135_000
    assert (np.bincount(exp, minlength=2048)[:2047] >= per + 2).all() and exp.max() == 2046      # no 0x7FF
    man = b & np.uint64(0xFFFFFFFFFFFFF)
    for e in (0, 1, 1022, 1023, 1075, 2046):
        assert {1, (1 << 52) - 1} <= set(man[exp == e].tolist())
    neg = (b >> np.uint64(63)).astype(bool)
    assert 0.4 < neg.mean() < 0.6
    # full mantissas: on average half of the 52 bits set, where the edge list has one
    assert np.mean([bin(m).count("1") for m in man[::97].tolist()]) > 20
    # every word count of both branches, every shift of both
    counts = {(e >= 1075, sh.word_count(int(x))) for e, x in zip(exp.tolist(), b.tolist()) if x & 0x7FFFFFFFFFFFFFFF}
    assert counts == {(True, n) for n in range(2, 33)} | {(False, n) for n in range(1, 35)}
    assert {(max(e, 1) - 1075) & 31 for e in exp.tolist()} == set(range(32))


def test_window_bits():
    b = sh.window_bits()
    assert len(b) == 100_000 + 2 * len(sh.WINDOW_EDGES)
    v = b.view(np.float64)
    assert (np.abs(v) >= 1e-6).all() and (np.abs(v) <= 2.0**63).all() and 0.4 < (v < 0).mean() < 0.6
    texts = [t.lstrip(b"-") for t in texts_of(b)]
    count = lambda pat: sum(1 for t in texts if re.fullmatch(pat, t))
    # a quarter of the list falls log-uniformly over 24 decades: about 1000 a decade
    assert count(rb"0\.000[1-9]\d*") > 500                  # fixed notation, 1e-4 <= |v| < 1e-3
    assert count(rb"\d(\.\d+)?e-05") > 500                  # the first decade below it
    assert count(rb"\d(\.\d+)?e\+17") > 2000                # those and the integers in [1e17, 1e18)
    assert count(rb"\d{16}") > 1000 and count(rb"\d{17}") > 2000
    assert count(rb"\d+\.5") > 20000 and count(rb"\d{1,15}") > 20000
    whole = set(texts_of(b))
    assert {b"4503599627370495", b"-4503599627370495", b"4503599627370496", b"-4503599627370496", b"4503599627370494",
            b"4503599627370495.5", b"9.2233720368547758e+18", b"1e+17", b"-1e+17", b"99999999999999984",
            b"10000000000000000", b"9.9999999999999991e-05", b"0.0001", b"1.0000000000000001e-05"} <= whole
    # ll2string's window (util.c:542-545) from both sides: integers it prints, and integers %.17g prints
    ints = v[(v == np.floor(v))]
    assert (np.abs(ints) < 2.0**52).sum() > 20000 and (np.abs(ints) >= 2.0**52).sum() > 20000


def launch_constants():
    """D2S_WPB and the grid cap as rr_launch_d2string has them."""
    src = open(os.path.join(ROOT, "redrock_old_amd", "csrc", "rr_rdbzset.hip")).read()
    wpb = int(re.search(r"constexpr uint32_t D2S_WPB = (\d+);", src).group(1))
    body = re.search(r"rr_launch_d2string\(.*?\n}", src, flags=re.S).group(0)
    cap = re.search(r"dim3\(\(uint32_t\)\(b < (\d+) \? b : (\d+)\)\), dim3\(D2S_WPB \* RR_WAVE\)", body)
    assert cap and cap.group(1) == cap.group(2)
    wave = int(re.search(r"#define RR_WAVE\s+(\d+)", open(os.path.join(ROOT, "redrock_old_amd", "csrc", "rr_device.h")).read()).group(1))
    return wpb, int(cap.group(1)), wave


def test_round_two_bits_reach_the_second_round():
    assert launch_constants() == (sh.D2S_WPB, sh.D2S_GRID_CAP, sh.RR_WAVE) == (4, 16384, 64)
    assert sh.N2 == 16384 * 4 * 64 + 65 > 16384 * 256 and sh.D2S_ROUND % sh.T == sh.SHIFT and sh.T % 2 == 1
    assert all(sh.T % p for p in range(2, 64))                                  # prime
    table = sh.round_two_table()
    bits = sh.round_two_bits()
    assert len(table) == sh.T and len(bits) == sh.N2 and np.array_equal(bits[:sh.T], table) and bits[sh.T] == table[0]
    text = texts_of(table)
    kinds = [sh.table_kind(j) for j in range(sh.T)]
    for t, k, b in zip(text, kinds, table.tolist()):
        if k == "short":
            assert len(t) <= 7
        else:
            assert len(t) == zr.D2STRING_MAX and sh.word_count(b) in ((34,) if k == "fraction" else (29, 30, 31, 32))
    assert {b"0", b"1.5", b"inf", b"nan", b"-0", b"-inf", b"17"} <= set(text)
    short = [k == "short" for k in kinds]
    assert sum(a != b for a, b in zip(short, short[1:])) >= sh.T // 2 - 2       # long and short in turn, one or two long
    # wave 0's 64 lanes and wave 1's lane 0: the second round's score, text and kind against the first's
    shorter = after_fraction = 0
    for lane in range(65):
        a, b = lane % sh.T, (lane + sh.D2S_ROUND) % sh.T
        assert bits[lane] == table[a] and bits[lane + sh.D2S_ROUND] == table[b] and text[a] != text[b] and kinds[a] != kinds[b]
        shorter += len(text[b]) < len(text[a])
        after_fraction += kinds[a] == "fraction" and kinds[b] == "integer"      # 32 words laid over a fraction's remains
    assert shorter >= 32 and after_fraction >= 16
    assert lane + sh.D2S_ROUND == sh.N2 - 1                                     # wave 1's second round: one slot


# ---- the payload generators ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def converted(name):
    """(values, [zset_blob's result for each]) of a generator, computed once."""
    vals = getattr(sh, name)()
    assert len({id(o) for _, o in vals}) == 1                                   # one batch, one set of options
    return vals, [zr.zset_blob(p, o) for p, o in vals]


def pairs_of(p):
    """(member, score bits) in payload order, by a walk of its own."""
    r = ld.Rd(p)
    out = [(r.string(), struct.unpack("<Q", r.take(8))[0]) for _ in range(r.count())]
    assert r.p == len(p)
    return out


def entries(blob):
    """(encoding byte, prevlen bytes) of every entry of a ZSET_ZIPLIST blob's ziplist, by the header bytes alone."""
    z = blob[13:]
    p, out = 10, []
    while z[p] != 0xFF:
        pl = 1 if z[p] < 254 else 5
        e = z[p + pl]
        if e < 0xC0:
            n, h = (e & 0x3F, 1) if e >> 6 == 0 else (((e & 0x3F) << 8) | z[p + pl + 1], 2)
        else:
            n, h = {0xFE: 1, 0xC0: 2, 0xF0: 3, 0xD0: 4, 0xE0: 8}.get(e, 0), 1
        out.append((e, pl))
        p += pl + h + n
    assert p == len(z) - 1
    return out


def check_order(p, res):
    """The blob's entries are the pairs sorted by (float, member bytes), the scores as d2string prints them."""
    st, blob, pay, nel = res
    items = pairs_of(p)
    assert st == 0 and blob[0] == zr.ZSET_ZIPLIST and (pay, nel) == (len(blob) - 13, len(items))
    want = sorted(items, key=lambda x: (zr.to_double(x[1]), x[0]))
    ents = ref.walk_ziplist(blob[13:])
    assert ents[0::2] == [m for m, _ in want] and ents[1::2] == [zr.d2string(b) for _, b in want]
    return want


def test_lane_sequence_zsets():
    vals, res = converted("lane_sequence_zsets")
    assert len(vals) == 2 and vals[0][1]["zset_max_ziplist_entries"] == 512
    for (p, o), r, bands in zip(vals, res, sh.LANE_BANDS):
        assert cv.convert_blob(ZSET, p, o)[0] == cv.E_CONVERT                   # the third stage's
        want = check_order(p, r)
        assert len(want) == 256 and [b for _, b in pairs_of(p)] != [b for _, b in want]   # shuffled
        for lane in range(64):
            for rnd, (kind, words, lens) in enumerate(bands):                   # what this lane prints, in sequence
                b = want[64 * rnd + lane][1]
                e = max(b >> 52 & 0x7FF, 1) - 1075
                assert (e >= 0) == (kind == "integer") and sh.word_count(b) == words, (lane, rnd, hex(b))
                assert len(zr.d2string(b)) in lens and (kind != "short" or sh.live_words(b) == 1)
        for rnd, (kind, words, lens) in enumerate(bands):                       # every length a band names occurs
            assert {len(zr.d2string(b)) for _, b in want[64 * rnd:64 * rnd + 64]} == set(lens)
    first = [k for k, _, _ in sh.LANE_BANDS[0]]
    assert first == ["integer", "fraction", "short", "integer"] and [w for _, w, _ in sh.LANE_BANDS[0]] == [32, 34, 2, 32]
    assert [k for k, _, _ in sh.LANE_BANDS[1]] == ["short", "fraction", "fraction", "fraction"]
    sub = [b for _, b in check_order(*[vals[0][0], res[0]])[64:128]]
    assert sum(b >> 63 for b in sub[:32]) == 32 and sum(b >> 63 for b in sub[32:]) == 0      # negative, then positive
    assert sum((b & 0x7FFFFFFFFFFFFFFF) >> 52 == 0 for b in sub) == 48                       # subnormals, and 16 normals


def test_int_text_zsets():
    vals, res = converted("int_text_zsets")
    groups = len(sh.INT_GROUPS)
    assert len(vals) == groups + 2 * len(sh.LAST_SLOT) and groups % 2 == 0
    seen, strings = set(), set()
    for (p, o), r in zip(vals, res):
        assert cv.convert_blob(ZSET, p, o)[0] == cv.E_CONVERT                   # a fractional score: left by the second stage
        want = check_order(p, r)
        assert sum(1 for _, b in want if zr.to_double(b) % 1) >= 1
        encs = entries(r[1])
        assert len(encs) == 2 * len(want)
        for (m, b), (e, pl) in zip(want, encs[1::2]):
            v = zr.to_double(b)
            if v in sh.STRING_SCORES or v % 1:
                assert e < 0xC0
                strings.add(zr.d2string(b))
            else:
                assert e == sh.int_encoding(int(v)), (v, hex(e))
                seen.add(e if e < 0xF1 or e == 0xFE else 0xF1)
    assert seen == {0xF1, 0xFE, 0xC0, 0xF0, 0xD0, 0xE0}
    assert {b"1e+17", b"9.2233720368547758e+18"} <= strings
    edge_scores = {zr.to_double(b) for (p, _) in vals[:groups] for _, b in pairs_of(p)}
    assert {float(v) for v in sh.INT_EDGES} | set(sh.STRING_SCORES) <= edge_scores
    assert all(sh.int_encoding(v) != sh.int_encoding(w) for v, w in ((12, 13), (-128, -129), (127, 128), (32767, 32768), (-32768, -32769),
                                                                    (2**23 - 1, 2**23), (-2**23, -2**23 - 1), (2**31 - 1, 2**31), (-2**31, -2**31 - 1)))
    # the last text slot of a round: the same ZSet on an even index and on the odd one behind it
    digits = set()
    for k, (n, ints) in enumerate(sh.LAST_SLOT):
        i = groups + 2 * k
        assert i % 2 == 0 and pairs_of(vals[i][0]) != pairs_of(vals[i + 1][0])
        for j in (i, i + 1):
            want = check_order(vals[j][0], res[j])
            encs = entries(res[j][1])
            assert len(want) == n
            for rank, v in ints.items():
                assert rank % 64 == 63 and zr.to_double(want[rank][1]) == float(v) and encs[2 * rank + 1][0] == sh.int_encoding(v)
                assert zr.to_double(want[rank - 1][1]) % 1 and encs[2 * rank - 1][0] < 0xC0
                digits.add(len(zr.d2string(want[rank][1])))
            assert sorted(want) == sorted(check_order(vals[i][0], res[i]))
    assert digits == {1, 2, 17}


def test_wave_reuse_batch():
    for swap in (False, True):
        vals = sh.wave_reuse_batch(swap)
        n = len(vals)
        assert n == cv.MAX_WAVES + sh.REUSE_PAIRS > cv.MAX_WAVES and len({id(o) for _, o in vals}) == 1
        o = vals[0][1]
        res = [zr.zset_blob(p, o) for p, _ in vals]
        stay = n - 7 + sh.REUSE_STAYS if swap else sh.REUSE_STAYS
        assert [r[0] for r in res] == [zr.E_CONVERT if k == stay else 0 for k in range(n)]
        big, small = (vals[-7:], vals[:7]) if swap else (vals[:7], vals[-7:])   # exactly MAX_WAVES apart
        assert all(len(p) > 1500 for p, _ in big) and all(len(p) < 40 for p, _ in small)
        assert vals.index(big[0]) % cv.MAX_WAVES == vals.index(small[0]) % cv.MAX_WAVES == 0
        bp = [pairs_of(p) for p, _ in big]
        assert [len(x) for x in bp[:2]] == [512, 511] and all(sh.word_count(b) == 34 for _, b in bp[0])
        assert {len(zr.d2string(b)) for _, b in bp[0]} == {24} and len({b for _, b in bp[1]}) == 1
        assert {sh.word_count(b) for _, b in bp[4]} == {34} and {(sh.word_count(b), (b >> 52 & 0x7FF) - 1075) for _, b in bp[5]} == {(32, 960)}
        blob = res[vals.index(big[2])][1]
        assert all(len(m) == 300 for m, _ in bp[2]) and {pl for _, pl in entries(blob)[1::2]} == {5}
        late = bp[sh.REUSE_STAYS]
        assert len(late) == 512 and late[-1][1] == zr.to_bits(float("nan")) and all(zr.to_double(b) == zr.to_double(b) for _, b in late[:-1])
        assert len(bp[4]) == len(bp[5]) == 512
        sp = [pairs_of(p) for p, _ in small]
        assert sp[0] == [(b"a", zr.to_bits(1.5))] and sp[1] == [] and small[1][0] == b"\x00"
        assert [m for m, _ in sp[2]] == [b"c", b"b", b"a"] and {zr.to_double(b) for _, b in sp[2]} == {0.25}
        assert sorted(zr.to_double(b) for _, b in sp[3]) == [0.5, 7.0]
        assert {(b >> 52 & 0x7FF) - 1075 for _, b in sp[4]} == {960} and {sh.word_count(b) for _, b in sp[5]} == {34}
        mid = vals[7:-7]
        assert {p[0] for p, _ in mid} == {2, 3} and sum(len(p) for p, _ in mid) < 1 << 20
        for (p, _), r in list(zip(vals, res))[:7] + list(zip(vals, res))[-7:] + list(zip(vals, res))[7:-7:97]:
            if r[0] == 0:
                check_order(p, r)
        assert all(zr.to_double(b) % 1 for p, _ in mid[::53] for _, b in pairs_of(p))
